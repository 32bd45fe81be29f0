"""fewx.solver.GraphedTrainStep on a schedule whose image sizes change: a bounded cache of graphs (`max_graphs`, `recur`), batches of
mixed sizes staged through orehip.batch_canvas_plan into a graph's fixed slab (`mixed_sizes`), and the references a graph's record keeps
to the memory its kernels point at.  The bar is that of test_hip_train.py::test_whole_step_graph_matches_eager: the same sampling keys,
the LR factor moving every step; parameters within 1e-6 of the largest weight, momentum within 1e-5, losses within 1e-5 relative --
equality to the last bit is the expectation."""
import pytest
import torch

from test_hip_train import _train_model

pytestmark = pytest.mark.gpu

SHOTS = 4


@pytest.fixture(scope="module")
def oh():
    import orehip
    orehip.lib()
    return orehip


def _item(seed, hw, n_gt):
    from oracle import ref_train as T
    from detectron2.structures import Boxes, Instances
    img, gt, sup, sbox = T.synth_train_inputs(seed, hw, n_gt=n_gt, shots=SHOTS, support_hw=96)
    inst = Instances(hw)
    inst.gt_boxes, inst.gt_classes = Boxes(gt), torch.zeros(len(gt), dtype=torch.int64)
    return {"image": img, "instances": inst, "support_images": sup, "support_bboxes": sbox.numpy()}


def _fix_sampling_keys(monkeypatch, B):
    keys = torch.rand(B, 16384, generator=torch.Generator().manual_seed(3)).cuda()
    real_rand = torch.rand

    def fixed_rand(*shape, **kw):                           # the fg / bg subsample draws its keys here: the same for both runs
        if len(shape) == 2 and kw.get("device") is not None and torch.device(kw["device"]).type == "cuda":
            return keys[:shape[0], :shape[1]].clone()
        return real_rand(*shape, **kw)

    monkeypatch.setattr(torch, "rand", fixed_rand)


def _run(batches, make_stepper):
    """The batches through plain eager steps (make_stepper = None) or a stepper; (losses per step, parameters, momentum, stepper)."""
    from fewx.solver import build_optimizer
    m, sd, cfg = _train_model(SHOTS)
    opt = build_optimizer(cfg, m)
    stepper = make_stepper(m, opt) if make_stepper is not None else None
    log = []
    for it, items in enumerate(batches):
        opt.set_lr_factor(0.02 * (1.0 + 0.25 * it))         # a schedule that moves every iteration
        if stepper is not None:
            losses = stepper(items)
        else:
            losses = m(items)
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
        log.append({k: float(v.detach()) for k, v in losses.items()})
    torch.cuda.synchronize()
    return log, opt.bucket.params.detach().clone(), opt.bucket.momentum.detach().clone(), stepper


def _assert_same_training(eager, graph):
    for it, (le, lg) in enumerate(zip(eager[0], graph[0])):
        for k, v in le.items():
            assert abs(v - lg[k]) <= 1e-5 * max(abs(v), 1e-3), (it, k, v, lg[k])
    pe, pg = eager[1], graph[1]
    assert float((pe - pg).abs().max()) <= 1e-6 * float(pe.abs().max()), float((pe - pg).abs().max())
    assert float((eager[2] - graph[2]).abs().max()) <= 1e-5 * float(eager[2].abs().max())


def test_alternating_sizes_replay_from_a_cache_of_graphs(oh, monkeypatch):
    """One image per step, (256, 320) and (224, 320) in turn: two eager steps, ONE capture per size, everything else a replay -- the
    two graphs (sharing one memory pool) replayed in turn leave the parameters of ten plain eager steps."""
    from fewx.solver import GraphedTrainStep
    _fix_sampling_keys(monkeypatch, 1)
    a, b = _item(2, (256, 320), 5), _item(3, (224, 320), 6)
    batches = [[a] if it % 2 == 0 else [b] for it in range(10)]
    eager = _run(batches, None)
    graph = _run(batches, lambda m, opt: GraphedTrainStep(m, opt, warmup=2, max_graphs=4, recur=1))
    st = graph[3]
    assert st.error is None, st.error
    s = st.stats()
    assert s["captures"] == 2 and st.captures == 2 and s["graphs"] == 2 and not s["full"], s
    assert st.eager_steps == 2 and st.replays == 8, s
    assert sorted((v["captures"], v["replays"], v["eager_steps"]) for v in s["keys"].values()) == [(1, 4, 1), (1, 4, 1)], s
    assert len(s["reserved_bytes"]) == 2 and all(isinstance(v, int) for v in s["reserved_bytes"])
    assert st.graph is st.record.graph and st.record in st.records.values() and st.losses is st.record.losses
    _assert_same_training(eager, graph)


def test_mixed_size_batch_replays_one_graph(oh, monkeypatch):
    """Two images of different sizes per step, swapping places from step to step (the canvas stays): with mixed_sizes the batch is
    staged as one slab and replayed from ONE graph, and trains as the plain eager steps do (train_core's mixed-size branch).  A default
    stepper runs the same batches eagerly, as it always has."""
    from fewx.solver import GraphedTrainStep
    _fix_sampling_keys(monkeypatch, 2)
    a, b = _item(2, (256, 320), 5), _item(3, (224, 320), 6)
    batches = [[a, b] if it % 2 == 0 else [b, a] for it in range(6)]
    eager = _run(batches, None)
    graph = _run(batches, lambda m, opt: GraphedTrainStep(m, opt, warmup=2, mixed_sizes=True))
    st = graph[3]
    assert st.error is None, st.error
    assert st.captures == 1 and st.eager_steps == 2 and st.replays == 4, st.stats()
    assert st.record.geom.q_canvas == (256, 320) and st.record.geom.n_query == 2 and st.record.geom.n_support == 2 * SHOTS
    _assert_same_training(eager, graph)
    default = _run(batches[:4], lambda m, opt: GraphedTrainStep(m, opt, warmup=1))
    st = default[3]
    assert st.error is None and st.eager_steps == 4 and st.replays == 0 and st.captures == 0 and st.graph is None
    for le, ld in zip(eager[0], default[0]):                                            # (and reports the eager steps' losses)
        assert all(abs(v - ld[k]) <= 1e-5 * max(abs(v), 1e-3) for k, v in le.items()), (le, ld)


def test_full_cache_keeps_further_sizes_eager(oh):
    """max_graphs = 2 and three sizes in rotation: once every size has run eagerly (recur = 1), the first two to come up are captured,
    the third never is -- it runs eagerly every time, which is no error -- and stats() says that the cache is full."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    m, sd, cfg = _train_model(SHOTS)
    opt = build_optimizer(cfg, m)
    opt.set_lr_factor(0.02)
    st = GraphedTrainStep(m, opt, warmup=1, max_graphs=2, recur=1)
    sizes = [(256, 320), (224, 320), (192, 320)]
    for it in range(12):                                    # 0 .. 2 eager (every size once), 3 and 4 captured, 5 finds the cache full
        losses = st([_item(50 + it, sizes[it % 3], 4 + it % 3)])
        assert all(bool(torch.isfinite(v)) for v in losses.values()), (it, losses)
    s = st.stats()
    assert st.error is None and s["full"] and s["graphs"] == 2 and s["captures"] == 2, s
    assert st.eager_steps == 6 and st.replays == 6, s
    third = [v for k, v in s["keys"].items() if k[2][0] == (3, 192, 320)]
    assert third == [{"captures": 0, "replays": 0, "eager_steps": 4}], s
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_graph_record_keeps_its_workspace_and_tables_alive(oh):
    """By identity: the record of a capture holds the very weight-gradient workspace orehip._WGWS held then and the packed-weight job
    tables present then; when a larger workspace replaces the first, the record still holds the old tensor."""
    from fewx.solver import GraphedTrainStep, build_optimizer
    m, sd, cfg = _train_model(SHOTS)
    opt = build_optimizer(cfg, m)
    opt.set_lr_factor(0.02)
    st = GraphedTrainStep(m, opt, warmup=2, max_graphs=2, recur=1)       # (the job table of the one-launch repack exists from step 2 on)
    for it in range(4):
        st([_item(70 + it, (224, 320), 4)])
    assert st.error is None and st.captures == 1 and st.replays == 2
    rec = st.record
    dev = str(rec.static["gtp"].device)
    old = oh._WGWS[dev]
    assert rec.keep["wgrad_ws"] is old
    tables = list(oh._PACK_TABLES.values())
    assert tables and all(any(t is k for k in rec.keep["pack_tables"]) for t in tables)
    assert all(rec.static[k].is_cuda for k in ("xq", "xs", "gtp", "gt_n", "sbx")) and all(v.is_cuda for v in rec.losses.values())
    new = oh._wgrad_ws(old.device, old.numel() + 1)
    oh._PACK_TABLES.clear()
    assert new is not old and oh._WGWS[dev] is new and rec.keep["wgrad_ws"] is old and rec.keep["wgrad_ws"].data_ptr() == old.data_ptr()
    assert len(rec.keep["pack_tables"]) >= len(tables) and not oh._PACK_TABLES
    losses = st([_item(73, (224, 320), 5)])                                            # the graph's arguments still point at live memory
    torch.cuda.synchronize()
    assert st.replays == 3 and all(bool(torch.isfinite(v)) for v in losses.values())


def test_default_trainer_with_graph_step_options(oh, tmp_path):
    """trainer.graph_step_options reaches the stepper: a loader that alternates two sizes, {"max_graphs": 4, "recur": 1} -- the trainer
    finishes its iterations, reports finite losses, and has captured exactly two graphs."""
    import os
    from conftest import PKG
    from detectron2.engine import DefaultTrainer
    from fewx.config import get_cfg

    def batches():
        i = 0
        while True:
            yield [_item(40 + i % 5, (256, 320) if i % 2 == 0 else (224, 320), 3 + i % 4)]
            i += 1

    class Trainer(DefaultTrainer):
        @classmethod
        def build_train_loader(cls, cfg):
            return batches()

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(PKG, "configs", "fsod", "finetune_vovnet.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "INPUT.FS.SUPPORT_SHOT", SHOTS, "SOLVER.MAX_ITER", 9, "SOLVER.CHECKPOINT_PERIOD", 100,
                         "OUTPUT_DIR", str(tmp_path), "MODEL.WEIGHTS", ""])
    cfg.freeze()
    torch.manual_seed(0)
    tr = Trainer(cfg)
    tr.resume_or_load(resume=False)
    tr.graph_step = True
    tr.graph_step_options = {"max_graphs": 4, "recur": 1}
    seen = []
    orig = tr._write_metrics

    def spy(loss_dict, data_time, prefix=""):
        seen.append({k: float(v) for k, v in loss_dict.items()})
        return orig(loss_dict, data_time, prefix)

    tr._write_metrics = spy
    tr.train()
    g = tr._graphed
    assert g.error is None, g.error
    assert g.max_graphs == 4 and g.recur == 1
    assert tr.iter == 8 and g.captures == 2 and g.eager_steps == 3 and g.replays == 6, g.stats()
    assert len(seen) == 9 and all(all(v == v and abs(v) < 1e6 for v in d.values()) for d in seen)
