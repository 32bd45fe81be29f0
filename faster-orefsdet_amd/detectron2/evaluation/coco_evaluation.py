"""COCOEvaluator (d2z:evaluation/coco_evaluation.py) for task "bbox": COCO box AP with pycocotools' COCOeval semantics, its per-image
matching and its accumulation on the device (orehip.coco_eval, csrc/ore_coco_eval.hip).  pycocotools is not needed: the ground truth
is read with the json module, the 12 summary numbers are computed from the precision / recall arrays here.

The detections stay on the device from `model()` to the result: `process()` keeps the output tensors and adds no synchronisation;
`evaluate()` gathers them to rank 0 (`comm.gather`), groups them by (category, image) on the device and runs the evaluation there.

An output that carries "proposals" is also scored with proposal recall, results["box_proposals"] = AR@100 .. ARl@1000
(ref:fewx/evaluation/coco_evaluation.py:126-128, 207-244, 453-561), on the device as well (orehip.proposal_recall,
csrc/ore_proposal_recall.hip)."""
import copy
import itertools
import json
import logging
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch

from detectron2.data import DatasetCatalog, MetadataCatalog
from detectron2.utils import comm

from . import DatasetEvaluator

# COCOeval Params (iouType "bbox"): the exact doubles pycocotools computes
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
# proposal recall (the reference's _eval_box_proposals): limits x areas, keys in its order
PROPOSAL_LIMITS = [100, 1000]
PROPOSAL_AREAS = {"all": "", "small": "s", "medium": "m", "large": "l"}


def proposal_iou_thrs():
    """The reference's default thresholds: torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=float32)."""
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def proposal_recalls(counts, num_pos):
    """The reference's last two fp32 steps from the integer counts of overlaps >= threshold: recalls = count / num_pos, ar = mean."""
    recalls = torch.as_tensor(counts, dtype=torch.int64).reshape(-1).float() / float(num_pos)       # num_pos 0: NaN, as there
    return recalls, recalls.mean()


def coco_gt_from_dataset_dicts(dataset_dicts, metadata):
    """What d2z:data/datasets/coco.py convert_to_coco_json writes for boxes: categories from thing_classes (dataset ids through
    thing_dataset_id_to_contiguous_id when the metadata has it), annotation ids 1..N, bbox XYWH rounded to 3 decimals, area = the
    unrounded box's area in fp32 (Boxes.area).  A record's segmentation is not read: the area is always the box area."""
    id_map = metadata.get("thing_dataset_id_to_contiguous_id")
    reverse = {v: k for k, v in id_map.items()} if id_map else None
    names = metadata.get("thing_classes")
    if names is None:
        n = 1 + max([a["category_id"] for d in dataset_dicts for a in d.get("annotations", [])], default=0)
        names = [str(i) for i in range(n)]
    rid = (lambda c: reverse[c]) if reverse else (lambda c: c)
    cats = [{"id": int(rid(i)), "name": name} for i, name in enumerate(names)]
    images, annos = [], []
    for idx, d in enumerate(dataset_dicts):
        img_id = d.get("image_id", idx)
        images.append({"id": img_id, "width": d.get("width"), "height": d.get("height"), "file_name": d.get("file_name")})
        for a in d.get("annotations", []):
            b = [float(v) for v in a["bbox"]]
            if a.get("bbox_mode", 1) == 0:                   # XYXY_ABS -> XYWH_ABS in fp32, as BoxMode.convert on a tensor
                x0, y0, x1, y1 = np.float32(b)
                b = [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]
            x, y, w, h = np.float32(b)
            area = float((np.float32(x + w) - x) * (np.float32(y + h) - y))   # XYWH -> XYXY, then (x1 - x0) * (y1 - y0), fp32
            b = [round(float(v), 3) for v in b]                # the json stores the box rounded to 3 decimals, the area unrounded
            annos.append({"id": len(annos) + 1, "image_id": img_id, "bbox": b, "area": area, "iscrowd": int(a.get("iscrowd", 0)),
                          "category_id": int(rid(a["category_id"]))})
    return {"images": images, "annotations": annos, "categories": cats}


class CocoGT:
    """The ground truth of one dataset as the device evaluation reads it: images and categories in ascending id order, annotations
    grouped by (category, image) pair, json order inside a pair (pycocotools' getAnnIds walks the images, then their annotations)."""

    def __init__(self, gt_json, contiguous_to_dataset_id=None):
        self.img_ids = sorted(im["id"] for im in gt_json["images"])
        cats = sorted(gt_json["categories"], key=lambda c: c["id"])
        self.cat_ids = [c["id"] for c in cats]
        self.cat_names = [c.get("name", str(c["id"])) for c in cats]
        self.img_index = {im: i for i, im in enumerate(self.img_ids)}
        self.cat_index = {c: k for k, c in enumerate(self.cat_ids)}
        # contiguous class id (what the model predicts) -> dataset category id; default: position in the id-sorted categories
        self.contiguous_to_dataset_id = dict(contiguous_to_dataset_id) if contiguous_to_dataset_id else dict(enumerate(self.cat_ids))
        I = len(self.img_ids)
        by_img = {}
        for a in gt_json.get("annotations", []):
            by_img.setdefault(a["image_id"], []).append(a)
        rows = [a for im in self.img_ids for a in by_img.get(im, []) if a["category_id"] in self.cat_index]
        pair = np.array([self.cat_index[a["category_id"]] * I + self.img_index[a["image_id"]] for a in rows], dtype=np.int64)
        order = np.argsort(pair, kind="stable")
        rows = [rows[i] for i in order]
        self.boxes = np.array([[float(v) for v in a["bbox"]] for a in rows], dtype=np.float64).reshape(-1, 4)
        self.area = np.array([float(a["area"]) for a in rows], dtype=np.float64)
        self.crowd = np.array([int(a.get("iscrowd", 0)) for a in rows], dtype=np.int32)
        self.ids = np.array([int(a["id"]) for a in rows], dtype=np.int64)
        cnt = np.bincount(pair[order], minlength=len(self.cat_ids) * I) if len(rows) else np.zeros(len(self.cat_ids) * I, np.int64)
        self.off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        # the per-image view (proposal recall): every annotation of an image in json order, whatever its category
        rows = [a for im in self.img_ids for a in by_img.get(im, [])]
        self.img_boxes = np.array([[float(v) for v in a["bbox"]] for a in rows], dtype=np.float64).reshape(-1, 4)
        self.img_area = np.array([float(a["area"]) for a in rows], dtype=np.float64)
        self.img_crowd = np.array([int(a.get("iscrowd", 0)) for a in rows], dtype=np.int32)
        self.img_off = np.concatenate([[0], np.cumsum([len(by_img.get(im, [])) for im in self.img_ids])]).astype(np.int32)
        self._dev = {}
        self._dev_img = {}

    def device(self, device):
        key = str(device)
        if key not in self._dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev[key] = {"boxes": t(self.boxes), "area": t(self.area), "crowd": t(self.crowd), "id": t(self.ids), "off": t(self.off)}
        return self._dev[key]

    def device_images(self, device):
        """The per-image view on the device: "boxes" XYWH fp64, "area" fp64, "crowd" int32, "off" [I + 1] int32."""
        key = str(device)
        if key not in self._dev_img:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev_img[key] = {"boxes": t(self.img_boxes), "area": t(self.img_area), "crowd": t(self.img_crowd), "off": t(self.img_off)}
        return self._dev_img[key]


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """COCOeval.summarize for bbox: the 12 numbers and their log lines, in pycocotools' wording."""
    lines = []

    def _s(ap=1, iouThr=None, areaRng="all", maxDets=100):
        iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
        titleStr = "Average Precision" if ap == 1 else "Average Recall"
        typeStr = "(AP)" if ap == 1 else "(AR)"
        iouStr = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
        aind = [i for i, a in enumerate(AREA_LBL) if a == areaRng]
        mind = [i for i, m in enumerate(max_dets) if m == maxDets]
        if ap == 1:
            s = precision
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
        return mean_s

    stats = np.zeros((12,))
    stats[0] = _s(1)
    stats[1] = _s(1, iouThr=.5, maxDets=max_dets[2])
    stats[2] = _s(1, iouThr=.75, maxDets=max_dets[2])
    stats[3] = _s(1, areaRng="small", maxDets=max_dets[2])
    stats[4] = _s(1, areaRng="medium", maxDets=max_dets[2])
    stats[5] = _s(1, areaRng="large", maxDets=max_dets[2])
    stats[6] = _s(0, maxDets=max_dets[0])
    stats[7] = _s(0, maxDets=max_dets[1])
    stats[8] = _s(0, maxDets=max_dets[2])
    stats[9] = _s(0, areaRng="small", maxDets=max_dets[2])
    stats[10] = _s(0, areaRng="medium", maxDets=max_dets[2])
    stats[11] = _s(0, areaRng="large", maxDets=max_dets[2])
    return stats, lines


def derive_coco_results(stats, precision, class_names=None):
    """d2z:evaluation/coco_evaluation.py _derive_coco_results for bbox: percent, NaN where COCO gives -1, AP-<name> per category when
    there is more than one (precision at all IoUs and recalls, area "all", maxDets 100)."""
    if stats is None:
        return {m: float("nan") for m in METRICS}
    results = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    for k, name in enumerate(class_names):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        ap = np.mean(p) if p.size else float("nan")
        results["AP-" + str(name)] = float(ap * 100)
    return results


class COCOEvaluator(DatasetEvaluator):
    """COCO box AP of a dataset registered with a COCO json (MetadataCatalog json_file) or, without one, of its DatasetCatalog records.
    Task "bbox" only; `use_fast_impl` is accepted and has no effect (the evaluation always runs on the device)."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, use_fast_impl=True, kpt_oks_sigmas=()):
        self._logger = logging.getLogger(__name__)
        if tasks is not None and not isinstance(tasks, (str, list, tuple, set)):
            self._logger.warning("COCOEvaluator: a config as `tasks` is deprecated; evaluating 'bbox'")
            tasks = None
        tasks = ("bbox",) if tasks is None else ((tasks,) if isinstance(tasks, str) else tuple(tasks))
        other = [t for t in tasks if t != "bbox"]
        if other:
            raise ValueError(f"COCOEvaluator evaluates task 'bbox' only; {other} (segm / keypoints) are not supported")
        self._tasks = ("bbox",)
        self._distributed = distributed
        self._output_dir = output_dir
        self._use_fast_impl = use_fast_impl
        self._dataset_name = dataset_name
        self._metadata = MetadataCatalog.get(dataset_name)
        json_file = self._metadata.get("json_file")
        if json_file is not None:
            with open(json_file) as f:
                gt_json = json.load(f)
            id_map = self._metadata.get("thing_dataset_id_to_contiguous_id")
            self._gt = CocoGT(gt_json, {v: k for k, v in id_map.items()} if id_map else None)
        else:
            self._logger.info(f"'{dataset_name}' has no json_file: building COCO records from DatasetCatalog")
            gt_json = coco_gt_from_dataset_dicts(DatasetCatalog.get(dataset_name), self._metadata)
            id_map = self._metadata.get("thing_dataset_id_to_contiguous_id")
            self._gt = CocoGT(gt_json, {v: k for k, v in id_map.items()} if id_map else {i: c["id"] for i, c in enumerate(gt_json["categories"])})
        self._workspace = None
        self._proposal_workspace = None
        self.precision = self.recall = self.scores = None
        self.proposal_stats = None
        self.reset()

    def reset(self):
        self._predictions = []
        self._proposals = []

    def process(self, inputs, outputs):
        """Keeps (image_id, boxes XYXY, scores, classes) of every output that has "instances" and (image_id, proposal boxes XYXY,
        objectness logits) of every output that has "proposals", as they are -- device tensors, no copy, no sync."""
        for inp, out in zip(inputs, outputs):
            if "instances" in out:
                inst = out["instances"]
                self._predictions.append((inp["image_id"], inst.pred_boxes.tensor, inst.scores, inst.pred_classes))
            if "proposals" in out:
                prop = out["proposals"]
                self._proposals.append((inp["image_id"], prop.proposal_boxes.tensor, prop.objectness_logits))

    def _gather_predictions(self):
        """All ranks' predictions on the main process, rank after rank (comm.gather to rank 0); [] on the other ranks."""
        if not self._distributed or comm.get_world_size() == 1:
            return list(self._predictions)
        comm.synchronize()
        mine = [(i, b.detach().cpu(), s.detach().cpu(), c.detach().cpu()) for i, b, s, c in self._predictions]
        preds = comm.gather(mine, dst=0)
        preds = list(itertools.chain(*preds))
        return preds if comm.is_main_process() else []

    def _gather_proposals(self):
        """As _gather_predictions, for the proposals."""
        if not self._distributed or comm.get_world_size() == 1:
            return list(self._proposals)
        mine = [(i, b.detach().cpu(), s.detach().cpu()) for i, b, s in self._proposals]
        props = comm.gather(mine, dst=0)
        props = list(itertools.chain(*props))
        return props if comm.is_main_process() else []

    def _coco_results(self, preds):
        """instances_to_coco_json of every prediction, in order, with dataset category ids: the results json rows."""
        out = []
        for img_id, b, s, c in preds:
            b = b.detach().cpu().numpy().astype(np.float32, copy=True).reshape(-1, 4)
            b[:, 2] -= b[:, 0]
            b[:, 3] -= b[:, 1]
            s = s.detach().cpu().numpy().astype(np.float32).tolist()
            c = c.detach().cpu().numpy().tolist()
            for k in range(len(s)):
                out.append({"image_id": img_id, "category_id": self._dataset_cat(c[k]), "bbox": b[k].tolist(), "score": s[k]})
        return out

    def _dataset_cat(self, contiguous):
        try:
            return self._gt.contiguous_to_dataset_id[int(contiguous)]
        except KeyError:
            raise KeyError(f"predicted class {int(contiguous)} is not a category of dataset '{self._dataset_name}'") from None

    def evaluate(self):
        preds = self._gather_predictions()
        props = self._gather_proposals()
        if self._distributed and not comm.is_main_process():
            return {}
        if len(preds) == 0 and len(props) == 0:
            self._logger.warning("[COCOEvaluator] Did not receive valid predictions.")
            return {}
        unknown = sorted({p[0] for p in preds + props if p[0] not in self._gt.img_index})
        if unknown:
            raise ValueError(f"Results do not correspond to current coco set: image ids {unknown[:5]} are not in '{self._dataset_name}'")
        self._results = OrderedDict()
        if props:
            self._results["box_proposals"] = self._eval_box_proposals(props)
        if len(preds) == 0:
            return copy.deepcopy(self._results)
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            path = os.path.join(self._output_dir, "coco_instances_results.json")
            self._logger.info("Saving results to {}".format(path))
            with open(path, "w") as f:
                json.dump(self._coco_results(preds), f)
        n_det = sum(int(p[2].numel()) for p in preds)
        if n_det == 0:
            self._logger.warning("No predictions from the model!")
            self._results["bbox"] = derive_coco_results(None, None)
            return copy.deepcopy(self._results)
        self._results["bbox"] = self._eval_device(preds)
        return copy.deepcopy(self._results)

    def _device_of(self, tensors):
        dev = next((t.device for t in tensors if t.is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("COCOEvaluator evaluates on the GPU (orehip); no GPU is available")
            dev = torch.device("cuda", torch.cuda.current_device())
        return dev

    def _proposal_recall(self, props):
        """The device call: every (limit, area) chain of every entry at once; the workspace is kept between evaluations.  Returns the
        CPU copies of "num_pos" [L * A], "counts" [L * A, T] and "status"."""
        import orehip
        gt = self._gt
        dev = self._device_of([p[1] for p in props])
        counts = [int(p[2].numel()) for p in props]
        img_idx = [gt.img_index[p[0]] for p in props]
        boxes = torch.cat([p[1].reshape(-1, 4).to(dev, torch.float32) for p in props])
        logits = torch.cat([p[2].reshape(-1).to(dev, torch.float32) for p in props])
        S, cells = orehip.proposal_recall_sizes(counts, img_idx, gt.img_off, PROPOSAL_LIMITS)
        wsb = orehip.lib().ore_proposal_recall_workspace_bytes(len(counts), int(logits.numel()), S, cells, len(PROPOSAL_AREAS), len(PROPOSAL_LIMITS))
        ws = self._proposal_workspace
        if ws is None or ws.device != dev or ws.numel() < wsb:
            ws = self._proposal_workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
        out = orehip.proposal_recall(boxes, logits, counts, img_idx, gt.device_images(dev), gt.img_off, AREA_RNG, PROPOSAL_LIMITS,
                                     proposal_iou_thrs().numpy(), workspace=ws)
        return {k: out[k].cpu() for k in ("num_pos", "counts", "status")}

    def _eval_box_proposals(self, props):
        """The reference's _eval_box_proposals: box_proposals.pkl (with an output_dir), then AR at limits 100 / 1000 over the area
        ranges all / small / medium / large, each float(ar) * 100, in the reference's key order."""
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            ids, boxes, logits = [], [], []
            for img_id, b, s in props:
                ids.append(img_id)
                boxes.append(b.detach().cpu().numpy().reshape(-1, 4))
                logits.append(s.detach().cpu().numpy().reshape(-1))
            data = {"boxes": boxes, "objectness_logits": logits, "ids": ids, "bbox_mode": 0}      # BoxMode.XYXY_ABS
            with open(os.path.join(self._output_dir, "box_proposals.pkl"), "wb") as f:
                pickle.dump(data, f)
        self._logger.info("Evaluating bbox proposals ...")
        out = self._proposal_recall(props)
        if int(out["status"][0]) != 0:
            raise RuntimeError(f"proposal recall: the device call skipped entries (status {int(out['status'][0])})")
        res, stats = {}, {}
        A = len(PROPOSAL_AREAS)
        for l, limit in enumerate(PROPOSAL_LIMITS):
            for a, suffix in enumerate(PROPOSAL_AREAS.values()):
                c = l * A + a
                num_pos = int(out["num_pos"][c])
                recalls, ar = proposal_recalls(out["counts"][c], num_pos)
                key = "AR{}@{:d}".format(suffix, limit)
                res[key] = float(ar.item() * 100)
                stats[key] = {"ar": ar, "recalls": recalls, "num_pos": num_pos}
        self.proposal_stats = stats
        self._logger.info("Proposal metrics: \n" + " | ".join(f"{k} {v:.3f}" for k, v in res.items()))
        return res

    def _eval_device(self, preds):
        import orehip
        dev = next((p[1].device for p in preds if p[1].is_cuda), None)
        if dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("COCOEvaluator evaluates on the GPU (orehip.coco_eval); no GPU is available")
            dev = torch.device("cuda", torch.cuda.current_device())
        gt = self._gt
        counts = [int(p[2].numel()) for p in preds]
        boxes = torch.cat([p[1].reshape(-1, 4).to(dev, torch.float32) for p in preds])
        scores = torch.cat([p[2].reshape(-1).to(dev, torch.float32) for p in preds])
        classes = torch.cat([p[3].reshape(-1).to(dev, torch.int64) for p in preds])
        img_idx = torch.repeat_interleave(torch.tensor([gt.img_index[p[0]] for p in preds], dtype=torch.int32),
                                          torch.tensor(counts)).to(dev)
        # contiguous class -> category index; an unknown class is refused below, as detectron2's reverse id mapping would
        n_lut = max(gt.contiguous_to_dataset_id) + 1 if gt.contiguous_to_dataset_id else 1
        lut_h = np.full(n_lut, -1, dtype=np.int32)
        for c, did in gt.contiguous_to_dataset_id.items():
            if c >= 0 and did in gt.cat_index:
                lut_h[c] = gt.cat_index[did]
        lut = torch.from_numpy(lut_h).to(dev)
        ok = (classes >= 0) & (classes < n_lut)
        cat_idx = torch.where(ok, lut[classes.clamp(0, n_lut - 1)], torch.full_like(classes, -1, dtype=torch.int32))
        bad = cat_idx < 0
        if bool(bad.any()):
            raise KeyError(f"predicted class {int(classes[bad][0])} is not a category of dataset '{self._dataset_name}'")
        wsb = orehip.lib().ore_coco_eval_workspace_bytes(len(gt.cat_ids), len(gt.img_ids), len(scores), len(gt.ids), len(IOU_THRS),
                                                         len(AREA_RNG), MAX_DETS[-1])
        if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < wsb:
            self._workspace = torch.empty(wsb, dtype=torch.uint8, device=dev)
        out = orehip.coco_eval(boxes, scores, img_idx, cat_idx, gt.device(dev), len(gt.img_ids), len(gt.cat_ids), IOU_THRS, REC_THRS,
                               AREA_RNG, MAX_DETS, workspace=self._workspace)
        self.precision = out["precision"].cpu().numpy()
        self.recall = out["recall"].cpu().numpy()
        self.scores = out["scores"].cpu().numpy()
        stats, lines = summarize(self.precision, self.recall)
        self.stats = stats
        self._logger.info("Evaluation results for bbox:\n" + "\n".join(lines))
        res = derive_coco_results(stats, self.precision, gt.cat_names)
        self._logger.info("Evaluation results for bbox: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
        return res
