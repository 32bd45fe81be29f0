"""inference_on_dataset: the reference's evaluation / FPS protocol (d2z:evaluation/evaluator.py:101-221): model.eval(), one
`model(inputs)` per batch, device sync after every batch, the first min(5, n-1) iterations excluded from the timing.
COCOEvaluator (coco_evaluation.py): COCO box AP on the device; DatasetEvaluators and print_csv_format as d2z exports them."""
import datetime
import logging
import time
from collections import OrderedDict
from collections.abc import Mapping
from contextlib import contextmanager

import torch


class DatasetEvaluator:
    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    """d2z:evaluation/evaluator.py: several evaluators as one; their result dicts are merged (keys must not collide)."""

    def __init__(self, evaluators):
        super().__init__()
        self._evaluators = evaluators

    def reset(self):
        for evaluator in self._evaluators:
            evaluator.reset()

    def process(self, inputs, outputs):
        for evaluator in self._evaluators:
            evaluator.process(inputs, outputs)

    def evaluate(self):
        from detectron2.utils.comm import is_main_process
        results = OrderedDict()
        for evaluator in self._evaluators:
            result = evaluator.evaluate()
            if is_main_process() and result is not None:
                for k, v in result.items():
                    assert k not in results, "Different evaluators produce results with the same key {}".format(k)
                    results[k] = v
        return results


def print_csv_format(results):
    """d2z:evaluation/testing.py: each task's metrics as copy-paste CSV lines in the log (per-category "AP-..." keys left out)."""
    logger = logging.getLogger(__name__)
    for task, res in results.items():
        if isinstance(res, Mapping):
            important_res = [(k, v) for k, v in res.items() if "-" not in k]
            logger.info("copypaste: Task: {}".format(task))
            logger.info("copypaste: " + ",".join([k[0] for k in important_res]))
            logger.info("copypaste: " + ",".join(["{0:.4f}".format(k[1]) for k in important_res]))
        else:
            logger.info(f"copypaste: {task}={res}")


@contextmanager
def inference_context(model):
    was = model.training
    model.eval()
    yield
    model.train(was)


def inference_on_dataset(model, data_loader, evaluator):
    logger = logging.getLogger(__name__)
    total = len(data_loader)
    if evaluator is None:
        evaluator = DatasetEvaluator()
    evaluator.reset()
    num_warmup = min(5, total - 1)
    start_time = time.perf_counter()
    total_compute_time = 0.0
    with inference_context(model), torch.no_grad():
        for idx, inputs in enumerate(data_loader):
            if idx == num_warmup:
                start_time = time.perf_counter()
                total_compute_time = 0.0
            t0 = time.perf_counter()
            outputs = model(inputs)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            total_compute_time += time.perf_counter() - t0
            evaluator.process(inputs, outputs)
    n = max(total - num_warmup, 1)
    total_time = time.perf_counter() - start_time
    logger.info("Total inference time: {} ({:.6f} s / img per device)".format(str(datetime.timedelta(seconds=int(total_time))), total_time / n))
    logger.info("Total inference pure compute time: {} ({:.6f} s / img per device)".format(
        str(datetime.timedelta(seconds=int(total_compute_time))), total_compute_time / n))
    results = evaluator.evaluate()
    inference_on_dataset.last_timing = {"images": n, "seconds_per_image": total_time / n, "compute_seconds_per_image": total_compute_time / n}
    return {} if results is None else results


from .coco_evaluation import COCOEvaluator  # noqa: E402  (needs DatasetEvaluator above)
