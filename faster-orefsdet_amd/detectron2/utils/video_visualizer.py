"""d2z:utils/video_visualizer.py for box detections, by the render contract of detectron2.utils.visualizer."""
from .visualizer import ColorMode, _BOXES_ONLY, draw_boxes, draw_heat, thing_classes

__all__ = ["VideoVisualizer"]


class VideoVisualizer:
    """VideoVisualizer(metadata, instance_mode=ColorMode.IMAGE).draw_instance_predictions(frame_rgb, predictions) -> VisImage.
    Colours are by class in every mode, so a track keeps its colour from frame to frame: the constant palette stands in for the
    upstream heuristic that matches instances between frames to reuse their colours.  channel_order="BGR" (an extension) tells that
    the frames are BGR.

    track=True (an extension) follows the instances from frame to frame instead: an orehip.BoxTracker (association contract "track
    v1"; built on first use, on the device of the first device Instances or on the host for host Instances) gives every instance an id
    that persists, predictions.track_ids is set, and colour and label follow the id ("overlay v1, track colouring").  track= may also
    be a BoxTracker of the caller's.  The ids are the package's own association, not upstream's colour heuristic."""

    def __init__(self, metadata, instance_mode=ColorMode.IMAGE, *, channel_order="RGB", track=False):
        if instance_mode not in (ColorMode.IMAGE, ColorMode.SEGMENTATION):
            raise NotImplementedError(f"VideoVisualizer: {instance_mode} needs instance masks; " + _BOXES_ONLY)
        self.metadata = metadata
        self.channel_order = channel_order
        self._instance_mode = instance_mode
        self.tracker = None if track is None or isinstance(track, bool) else track
        self._track = bool(track)                             # False / None: colours by class, as ever
        if self.tracker is not None and not callable(getattr(self.tracker, "update", None)):
            raise ValueError("VideoVisualizer: track is False, True or an orehip.BoxTracker")

    def draw_instance_predictions(self, frame, predictions):
        names = thing_classes(self.metadata)
        if not self._track:
            return draw_boxes(frame, predictions, channel_order=self.channel_order, names=names, color_by="class")
        if self.tracker is None:
            import orehip
            boxes = predictions.pred_boxes
            boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
            self.tracker = orehip.BoxTracker(boxes.device if getattr(boxes, "is_cuda", False) else "cpu")
        ids = self.tracker.update(predictions)                # sets predictions.track_ids
        return draw_boxes(frame, predictions, channel_order=self.channel_order, names=names, color_by="track", ids=ids)

    def draw_heatmap(self, frame, source, **style):
        """A heat map of a detection pass over the frame (detectron2.utils.visualizer.draw_heat) -> VisImage; hand its .img to
        draw_instance_predictions to put the boxes on top."""
        return draw_heat(frame, source, channel_order=self.channel_order, **style)

    def draw_sem_seg(self, *args, **kwargs):
        raise NotImplementedError("draw_sem_seg: " + _BOXES_ONLY)

    def draw_panoptic_seg_predictions(self, *args, **kwargs):
        raise NotImplementedError("draw_panoptic_seg_predictions: " + _BOXES_ONLY)
