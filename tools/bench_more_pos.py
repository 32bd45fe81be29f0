#!/usr/bin/env python3
"""The MORE_POS launch beside the launch it replaces: `k_cn_more_pos` and `k_cn_pos_inds` on the same inputs.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o more_pos -- python tools/bench_more_pos.py --images 16 --objects 8
    python tools/bench_more_pos.py --stats OUT/.../more_pos_kernel_stats.csv ...     # -> one JSON line with the two kernels' times

Inputs: `--images` images of 640 x 640 (levels 80x80, 40x40, 20x20), `--objects` boxes per image, head rows that regress a third of the
objects well (the k-th value binds there, the 0.2 clamp elsewhere).  Each form is launched `--reps` times back to back; kernel time comes
from the trace of a run of its own, never from host timers around a launch of a few microseconds."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "faster-orefsdet_amd"))


def stats(path):
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in ("k_cn_more_pos", "k_cn_pos_inds", "k_cn_targets"):
                if k + "(" in r["Name"]:
                    out[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                              "max_us": float(r["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--objects", type=int, default=8, help="boxes per image")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--stats", default=None, help="a kernel_stats.csv of rocprofv3: print the kernels' times instead of running")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps({"images": a.images, "objects_per_image": a.objects, "size": a.size, "kernels": stats(a.stats)}))
        return
    import torch
    import orehip
    g = torch.Generator().manual_seed(a.images * 1000 + a.objects)
    B, N, S = a.images, a.objects, a.size
    strides = (8, 16, 32)
    shapes = [(S // s, S // s) for s in strides]
    ctr = torch.rand(B, N, 2, generator=g) * S
    wh = torch.exp(torch.rand(B, N, 2, generator=g) * 2.5 + 3.0)
    gt = (torch.cat([ctr - wh / 2, ctr + wh / 2], 2).clamp(0, S) * 8).round() / 8
    cnt = torch.full((B,), N, dtype=torch.int32)
    rows = sum(B * h * w for h, w in shapes)
    head = torch.rand(rows, 16, generator=g) * 6.0
    # a third of the objects regressed well: their centre cells' rows hold the centre regression
    row0 = 0
    for s, (H, W) in zip(strides, shapes):
        cx, cy = ((gt[..., 0] + gt[..., 2]) / 2 / s).long().clamp(0, W - 1), ((gt[..., 1] + gt[..., 3]) / 2 / s).long().clamp(0, H - 1)
        for b in range(B):
            for n in range(0, N, 3):
                x, y = int(cx[b, n]), int(cy[b, n])
                gx, gy = x * s + s // 2, y * s + s // 2
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if 0 <= x + dx < W and 0 <= y + dy < H:
                            t = torch.tensor([gx + dx * s - gt[b, n, 0], gy + dy * s - gt[b, n, 1], gt[b, n, 2] - gx - dx * s, gt[b, n, 3] - gy - dy * s]) / s
                            head[row0 + b * H * W + (y + dy) * W + x + dx, :4] = t.clamp(min=0)
        row0 += B * H * W
    gt, cnt, head = gt.cuda().contiguous(), cnt.cuda(), head.cuda()
    for mp in (None, (head, 0.2, 9)):
        for _ in range(a.reps):
            o = orehip.centernet_targets(None, shapes, strides, padded=(gt, cnt), more_pos=mp)
        torch.cuda.synchronize()
        print(json.dumps({"more_pos": mp is not None, "images": B, "objects_per_image": N, "positives": int(o["pos_count"].item()),
                          "capacity": o["pos_inds"].numel()}))


if __name__ == "__main__":
    main()
