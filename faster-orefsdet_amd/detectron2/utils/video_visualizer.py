"""d2z:utils/video_visualizer.py for box detections, by the render contract of detectron2.utils.visualizer."""
from .visualizer import ColorMode, _BOXES_ONLY, draw_boxes, draw_heat, thing_classes

__all__ = ["VideoVisualizer"]


class VideoVisualizer:
    """VideoVisualizer(metadata, instance_mode=ColorMode.IMAGE).draw_instance_predictions(frame_rgb, predictions) -> VisImage.
    Colours are by class in every mode, so a track keeps its colour from frame to frame: the constant palette stands in for the
    upstream heuristic that matches instances between frames to reuse their colours.  channel_order="BGR" (an extension) tells that
    the frames are BGR."""

    def __init__(self, metadata, instance_mode=ColorMode.IMAGE, *, channel_order="RGB"):
        if instance_mode not in (ColorMode.IMAGE, ColorMode.SEGMENTATION):
            raise NotImplementedError(f"VideoVisualizer: {instance_mode} needs instance masks; " + _BOXES_ONLY)
        self.metadata = metadata
        self.channel_order = channel_order
        self._instance_mode = instance_mode

    def draw_instance_predictions(self, frame, predictions):
        return draw_boxes(frame, predictions, channel_order=self.channel_order, names=thing_classes(self.metadata), color_by="class")

    def draw_heatmap(self, frame, source, **style):
        """A heat map of a detection pass over the frame (detectron2.utils.visualizer.draw_heat) -> VisImage; hand its .img to
        draw_instance_predictions to put the boxes on top."""
        return draw_heat(frame, source, channel_order=self.channel_order, **style)

    def draw_sem_seg(self, *args, **kwargs):
        raise NotImplementedError("draw_sem_seg: " + _BOXES_ONLY)

    def draw_panoptic_seg_predictions(self, *args, **kwargs):
        raise NotImplementedError("draw_panoptic_seg_predictions: " + _BOXES_ONLY)
