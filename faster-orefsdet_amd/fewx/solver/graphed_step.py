"""One whole training iteration -- forward, the five losses, backward, value clip + SGD -- as ONE replayed hipGraph.

The reference's loop (d2z:engine/train_loop.py:258-294: `loss_dict = model(data); losses.backward(); optimizer.step()`) issues about a
thousand kernel launches per iteration; at the reference's IMS_PER_BATCH = 1 the GPU finishes them faster than the host can issue them
(7.0 ms of kernels in a 9.4 ms step).  Every stage of the training forward is sync-free and fixed-shape already (train_forward.py), the
optimizer is one kernel that can read its schedule factor from the device -- so after a few eager iterations the iteration is captured
once and replayed: per step the host stages the inputs into the graph's fixed buffers, writes the LR factor, replays.

Opt-in (`GraphedTrainStep(model, optimizer)`; the trainer's plain step stays the default).  Falls back to the eager step -- and says why
in `.error` -- when the capture fails or the inputs do not fit the captured shapes (mixed image sizes, more ground-truth boxes than the
capacity: a new capture is made for a larger capacity).  Single-process only: a data-parallel wrapper's gradient exchange is issued from
backward hooks on its own stream and stays eager.

With its defaults the class keeps ONE graph and captures again whenever the input shapes change.  The reference's schedule changes them
all the time (MIN_SIZE_TRAIN draws one of seven sizes per image), so two options, both off by default, serve it:

`max_graphs` >= 2 (with `recur`): up to that many graphs stay alive, one per key (input shapes + dtypes + ground-truth capacity).  A
  key without a graph runs eagerly until its shapes have run eagerly `recur` times -- so everything that is sized lazily (the weight-
  gradient workspace, the packed-weight job tables, the sampler's kernel attributes) exists before the capture -- and is captured then.
  Nothing is evicted: once the cache is full, further keys run eagerly for good, `.error` stays None and `stats()["full"]` says so.
  (`max_graphs` = 1 is the single graph that is captured again on every change.  A cache wants `recur` >= 1, and `warmup` >= 2 whatever
  the options: the job table of the one-launch weight repack is made in the model's second step.)
`mixed_sizes`: a batch whose images differ in size is packed into one pinned buffer (orehip.batch_canvas_plan), uploaded with one copy
  into the graph's fixed slab, and the graph starts with the one launch that builds both canvases (orehip.batch_canvas) in front of
  `dense_part(model, xq, xs)`.  The key is the canvas: every batch with the same batch maximum replays the same graph.  Batches of one
  size keep the raw path (the preprocessing fused into stem_1).  Host images only; a mixed batch of device images runs eagerly.

A graph's record (`.record`, `.records`) keeps every device tensor alive that its kernels' arguments point at and that something else
may drop: the weight-gradient workspace and the packed-weight job tables of the time of its capture (orehip replaces the first when a
larger one is asked for and clears the second past 64 entries), its static inputs and its loss buffers.  With `share_pool` (default)
the graphs of a cache allocate from one memory pool: a replay is a whole iteration, nothing but its loss buffers (which stay allocated)
is read afterwards, and replays are ordered on one stream -- so the activations of one graph may live where another's did."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch


class _GraphRecord:
    """One captured iteration: the graph, its key, its fixed input and loss buffers, and `keep`: references that hold the memory its
    kernels' arguments point at ("wgrad_ws": the tensor orehip._WGWS held, "pack_tables": the tensors orehip._PACK_TABLES held)."""

    def __init__(self, graph, key, hkey, static, losses, geom, keep, reserved_bytes):
        self.graph, self.key, self.hkey, self.static, self.losses, self.geom = graph, key, hkey, static, losses, geom
        self.keep, self.reserved_bytes, self.replays = keep, int(reserved_bytes), 0


def _keep_alive(dev) -> Dict:
    import orehip
    return {"wgrad_ws": orehip._WGWS.get(str(dev)), "pack_tables": list(orehip._PACK_TABLES.values())}


class GraphedTrainStep:
    def __init__(self, model, optimizer, warmup: int = 3, gt_capacity: int = 64, max_graphs: int = 1, recur: int = 0,
                 mixed_sizes: bool = False, share_pool: bool = True):
        self.model, self.opt = model, optimizer
        self.warmup = int(warmup)
        self.gt_capacity = int(gt_capacity)
        self.max_graphs, self.recur, self.mixed_sizes, self.share_pool = max(1, int(max_graphs)), int(recur), bool(mixed_sizes), bool(share_pool)
        # the graph used last (with one graph: the graph)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.key = None
        self.static: Optional[Dict[str, torch.Tensor]] = None
        self.losses: Optional[Dict[str, torch.Tensor]] = None
        self.record: Optional[_GraphRecord] = None
        self.error: Optional[str] = None
        self.eager_steps = 0
        self.replays = 0
        self.captures = 0
        self.records: Dict[tuple, _GraphRecord] = {}
        self._pool = None
        self._seen: Dict[tuple, int] = {}                    # eager runs per input signature
        self._per_key: Dict[tuple, Dict[str, int]] = {}

    # ---- bookkeeping
    def _count(self, sig, what):
        if sig is not None:
            d = self._per_key.setdefault(sig, {"captures": 0, "replays": 0, "eager_steps": 0})
            d[what] += 1

    def stats(self) -> Dict:
        """Captures, replays and eager steps, in all and per input signature; `full`: the cache holds `max_graphs` graphs, keys without
        one run eagerly from now on; `reserved_bytes`: the device memory the allocator reserved during each capture, in capture order."""
        return {"captures": self.captures, "replays": self.replays, "eager_steps": self.eager_steps, "graphs": len(self.records),
                "full": self.max_graphs > 1 and len(self.records) >= self.max_graphs,
                "reserved_bytes": [r.reserved_bytes for r in self.records.values()],
                "keys": {k: dict(v) for k, v in self._per_key.items()}}

    def _use(self, rec: Optional[_GraphRecord]):
        self.record = rec
        self.graph, self.key, self.static, self.losses = (rec.graph, rec.key, rec.static, rec.losses) if rec is not None else (None,) * 4

    # ---- the iteration, eager
    def _eager(self, batched_inputs, sig=None):
        losses = self.model(batched_inputs)
        self.opt.zero_grad()
        sum(losses.values()).backward()
        self.opt.step()
        self.eager_steps += 1
        if sig is not None:
            self._seen[sig] = self._seen.get(sig, 0) + 1
            self._count(sig, "eager_steps")
        # detached: a loss that keeps its autograd graph alive keeps the parameters' AccumulateGrad nodes alive, and those remember the
        # stream they were made on -- a later capture would have to wait on that (uncaptured) stream
        return {k: v.detach() for k, v in losses.items()}

    def _signature(self, batched_inputs):
        """What of a batch decides its graph, read from the host: ("same", ...) for images of one size (the raw path), ("mixed", ...,
        canvases) for several sizes under `mixed_sizes`; None when the batch cannot be replayed (it runs eagerly)."""
        q = [(tuple(i["image"].shape), str(i["image"].dtype)) for i in batched_inputs]
        s = [(tuple(i["support_images"].shape), str(i["support_images"].dtype)) for i in batched_inputs]
        if all(x == q[0] for x in q) and all(x[0] == s[0][0] for x in s):
            return ("same", len(q), q[0], s[0][0], tuple(x[1] for x in s))
        if not self.mixed_sizes:
            return None
        if any(getattr(i[k], "is_cuda", False) for i in batched_inputs for k in ("image", "support_images")):
            return None
        u8f32 = ("torch.uint8", "torch.float32")
        if any(x[1] != q[0][1] for x in q) or any(x[1] != s[0][1] for x in s) or q[0][1] not in u8f32 or s[0][1] not in u8f32:
            return None
        div = self.model.backbone.size_divisibility
        up = lambda n: (n + div - 1) // div * div           # noqa: E731
        qc = tuple(up(max(x[0][d] for x in q)) for d in (1, 2))
        sc = tuple(up(max(x[0][d] for x in s)) for d in (2, 3))
        return ("mixed", len(q), qc, q[0][1], sum(x[0][0] for x in s), sc, s[0][1])

    def _stage(self, batched_inputs, sig=None):
        """Uploads of this call and the fixed-shape view of them; None when the batch does not fit one graph (mixed sizes)."""
        from fewx.modeling.fsod.train_forward import stage_inputs
        if sig is not None and sig[0] == "mixed":
            import orehip
            st = stage_inputs(self.model, batched_inputs, gt_capacity=self.gt_capacity, images=False)
            plan = orehip.batch_canvas_plan([i["image"] for i in batched_inputs], [i["support_images"] for i in batched_inputs],
                                            div=self.model.backbone.size_divisibility, full_slab=True)
            rec = self.records.get((sig, self.gt_capacity))
            if rec is not None:                              # the step's one image upload, straight into the graph's slab
                assert plan.geom == rec.geom
                rec.static["canvas_buf"][:plan.used].copy_(plan.host[:plan.used], non_blocking=True)
                cur = dict(gtp=st["gtp"], gt_n=st["gt_n"], sbx=st["sbx"].contiguous())
            else:
                buf = torch.empty(plan.geom.table_bytes + plan.geom.slab_bytes, dtype=torch.uint8, device=self.model.device)
                buf[:plan.used].copy_(plan.host[:plan.used], non_blocking=True)
                cur = dict(canvas_buf=buf, gtp=st["gtp"], gt_n=st["gt_n"], sbx=st["sbx"].contiguous())
            key = (("canvas", tuple(plan.geom)),) + tuple((k, tuple(v.shape), str(v.dtype)) for k, v in cur.items() if k != "canvas_buf")
            return cur, key, plan.geom
        st = stage_inputs(self.model, batched_inputs, gt_capacity=self.gt_capacity)
        imgs, sups = st["imgs"], st["sups"]
        if not (all(i.shape == imgs[0].shape and i.dtype == imgs[0].dtype for i in imgs) and all(s.shape == sups[0].shape for s in sups)):
            return None, None, None
        xq = torch.stack(imgs) if len(imgs) > 1 else imgs[0][None]
        xs = torch.cat(sups, 0) if len(sups) > 1 else sups[0]
        cur = dict(xq=xq.contiguous(), xs=xs.contiguous(), gtp=st["gtp"], gt_n=st["gt_n"], sbx=st["sbx"].contiguous())
        key = tuple((k, tuple(v.shape), str(v.dtype)) for k, v in cur.items())
        return cur, key, None

    def _capture(self, cur, key, hkey=None, geom=None):
        from fewx.modeling.fsod.train_forward import train_core
        from orehip import autograd as A
        opt = self.opt
        dev = cur["gtp"].device                              # (with its index: the key of orehip's per-device workspace)
        # (a mixed-size step's slab was allocated for this capture: it IS the static buffer)
        static = {k: (v if k == "canvas_buf" else v.clone()) for k, v in cur.items()}
        st = dict(static, canvas_geom=geom) if geom is not None else static
        if opt.lr_dev is None:
            opt.lr_dev = torch.full((1,), float(opt.lr_factor), device=dev)
        _w = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
        if _w is not None:                                   # (see train_forward.graphed_dense_part: the engine orders the streams itself)
            _w(False)
        saved_graph_flag = getattr(self.model, "train_graph", False)
        self.model.train_graph = False                       # no capture inside the capture
        g = torch.cuda.CUDAGraph()
        keep = _keep_alive(dev)
        try:
            import gc
            gc.collect()                                     # (no autograd graph of an earlier iteration may survive into the capture)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()                         # (torch.cuda.graph does the same on entry: the baseline of `reserved_bytes`)
            reserved = torch.cuda.memory_reserved(dev)
            pool = self._pool if (self.share_pool and self.max_graphs > 1) else None
            with torch.cuda.graph(g, pool=pool):
                losses = train_core(self.model, st, static=True)
                opt.zero_grad()
                sum(losses.values()).backward()
                opt.step()
            if self.share_pool and self.max_graphs > 1 and self._pool is None:
                self._pool = g.pool()
            # what the capture's kernels point at besides their own pool: the workspace and the job tables as they are NOW (and were
            # before the capture, should the capture itself have replaced them)
            after = _keep_alive(dev)
            ids = {id(t) for t in after["pack_tables"]}
            keep = {"wgrad_ws": after["wgrad_ws"], "wgrad_ws_before": keep["wgrad_ws"],
                    "pack_tables": after["pack_tables"] + [t for t in keep["pack_tables"] if id(t) not in ids]}
            rec = _GraphRecord(g, key, hkey, static, {k: v.detach() for k, v in losses.items()}, geom, keep,
                               torch.cuda.memory_reserved(dev) - reserved)
            if self.max_graphs == 1:
                self.records.clear()                         # the single graph: the new capture replaces the old one
            self.records[hkey if hkey is not None else key] = rec
            self.captures += 1
            self._use(rec)
            return rec
        except Exception as ex:                              # noqa: BLE001 -- the capture is an optimisation, never a requirement
            self.error = repr(ex)[:500]
            if self.max_graphs == 1:
                self.records.clear()
                self._use(None)
            torch.cuda.synchronize()
            A.weights_changed()
            return None
        finally:
            self.model.train_graph = saved_graph_flag
        # the capture itself ran nothing: whatever the eager steps left in the caches is still right; the first replay repacks

    def __call__(self, batched_inputs):
        if self.error is not None:
            return self._eager(batched_inputs)
        sig = self._signature(batched_inputs)
        if self.eager_steps < self.warmup or sig is None:
            return self._eager(batched_inputs, sig)
        n_gt = max(int(len(item["instances"])) for item in batched_inputs)
        while n_gt > self.gt_capacity:
            self.gt_capacity *= 2
        hkey = (sig, self.gt_capacity)
        rec = self.records.get(hkey)
        if rec is None:
            # no graph for these shapes: not yet (they have to run eagerly `recur` times first), or never (the cache is full)
            if self._seen.get(sig, 0) < self.recur or (self.max_graphs > 1 and len(self.records) >= self.max_graphs):
                return self._eager(batched_inputs, sig)
        cur, key, geom = self._stage(batched_inputs, sig)
        if cur is None:
            return self._eager(batched_inputs, sig)
        if rec is None:
            rec = self._capture(cur, key, hkey, geom)
            if rec is None:
                return self._eager(batched_inputs, sig)
            self._count(sig, "captures")
        self._use(rec)
        for k, v in cur.items():
            if rec.static[k] is not v:
                rec.static[k].copy_(v, non_blocking=True)
        self.opt.lr_dev.fill_(float(self.opt.lr_factor))
        rec.graph.replay()
        self.opt.after_step()                                # version counters / packed-weight caches: host-side, not in the graph
        self.replays += 1
        rec.replays += 1
        self._count(sig, "replays")
        return rec.losses
