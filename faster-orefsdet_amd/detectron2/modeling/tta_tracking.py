"""Tracking behind the TTA merge: the GeneralizedRCNNWithTTA that detectron2.modeling exports.  It is test_time_augmentation's wrapper
with one more argument, track=, and nothing else changed: the tracker's update (association contract "track v1", include/ore_hip.h) is
queued behind orehip.tta_merge, on the merged record's views and its device-side count, before the image's one host wait.  With
track=None it is the base class call for call."""
from . import test_time_augmentation as _tta

__all__ = ["GeneralizedRCNNWithTTA"]


class _Pending(_tta._Pending):
    """The base's pending image, and the ids of the record's rows (None without a tracker)."""
    __slots__ = ("ids",)


class GeneralizedRCNNWithTTA(_tta.GeneralizedRCNNWithTTA):
    __doc__ = _tta.GeneralizedRCNNWithTTA.__doc__ + """

    track=True follows the merged detections from image to image in the order of the calls: an orehip.BoxTracker while
    TEST.DETECTIONS_PER_IMAGE fits its rows, an orehip.WideBoxTracker beyond; or pass a tracker of either class, on the model's device.
    The result's Instances then carries track_ids and track_stats() counts the tracks started; the image still has one host wait."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3, track=None):
        super().__init__(cfg, model, tta_mapper=tta_mapper, batch_size=batch_size)
        import orehip
        from fewx.modeling.tiled_inference import merge_tracker
        rows = self.topk + (self.topk & 1)
        if track is True and rows <= int(orehip.lib().ore_det_record_rows()):
            track = orehip.BoxTracker(self.model.device)      # the one-pass sizes stay with the one-launch tracker
        self.tracker = merge_tracker("GeneralizedRCNNWithTTA", track, rows, self.model.device)

    def track_stats(self):
        """BoxTracker.stats() of the images so far: tracks, started, frames, dropped.  One host sync."""
        if self.tracker is None:
            return {"tracks": 0, "started": 0, "frames": 0, "dropped": 0}
        return self.tracker.stats()

    def _merge(self, pool, out_hw):
        from fewx.modeling.tiled_inference import enqueue_track
        base = super()._merge(pool, out_hw)
        p = _Pending()
        for name in _tta._Pending.__slots__:
            setattr(p, name, getattr(base, name))
        p.ids = enqueue_track(self.tracker, p) if self.tracker is not None else None
        return p

    def _finish(self, p):
        out = super()._finish(p)
        if p.ids is not None:
            out["instances"].track_ids = p.ids[:len(out["instances"].scores)]
        return out
