"""The bench line the driver parses: checked on the committed artifact of the last GPU run (profiles/r03_bench.json) so that a change
of bench.py's output format is caught on the CPU.  (The numbers themselves are produced on the MI355X.)"""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [l for l in f.read().strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "bench.py prints ONE JSON line"
    return json.loads(lines[0])


def test_bench_line_has_the_contract_fields():
    d = _line("r03_bench.json")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["n_gpus"] == 1
    assert "workload" in d["config"] and "model" not in d["config"] and "bs=1" in d["config"]["workload"]
    assert "torch.cuda.synchronize() per image" in d["config"]["workload"] and d["config"]["images_in_flight_per_gpu"] == 1
    assert d["config"]["timed_region_s"] >= 1.0 and d["config"]["timed_steps"] >= d["steps"]    # the timed region has a minimum duration
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - d["n_gpus"]) < 0.02 * d["n_gpus"]          # value = images / time of the timed steps
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["peak"] == 157.3
    assert r["traffic"] is None or r["traffic"] > 1e8
    with open(os.path.join(ROOT, "profiles", "r03_pmc_traffic.json")) as f:      # the PMC file carries the library version it was taken with
        assert "ore_version" in json.load(f)
    assert d["config"]["hipgraph"] is True and "extra_legs_hipgraph" in d["config"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    assert "both stages" in c["sample"]
    # the protocol figure is the headline; the engine-level and in-flight figures are extras and can only be higher
    assert d["engine_sequential"]["images_per_s"] >= d["value"] * 0.97 and d["in_flight"]["images_per_s"] >= d["value"]
    assert d["train_step_bs16"]["batch_per_gpu"] == 16 and d["train_step_bs16"]["images_per_s"] > 0


def test_two_rank_rehearsal_line_carries_the_dp_train_leg():
    """bench.py --gpus 2 (rehearsed over gloo on one card: the timings are not RCCL's, the code path is the driver's): the line holds
    the eval figure of both ranks and the DP train leg with the exchange measured alone and the share hidden behind backward."""
    d = _line("r02_bench_2rank_gloo_rehearsal.json")
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and "dp2" in d["config"]["parallelism"]
    t = d["train_step"]
    for k in ("images_per_s", "global_batch", "allreduce_ms", "overlap_frac", "ms_per_step_without_exchange", "rccl_ranks_seen", "exchanged_bytes_per_step"):
        assert k in t, k
    assert t["global_batch"] == 32 and t["rccl_ranks_seen"] == 2 and t["exchanged_bytes_per_step"] == 16365568


def test_self_launched_two_rank_line():
    """`python bench.py --gpus 2` with NO launcher, GPU legs included (two ranks sharing the one card of a gpurun box, exchange over gloo):
    the line of rank 0 carries both ranks' eval figure, the DP train leg and -- new in round 3 -- a cpu_baseline for N > 1."""
    d = _line("r03_bench_2rank_selflaunch_gloo_rehearsal.json")
    assert d["n_gpus"] == 2 and "dp2" in d["config"]["parallelism"] and d["train_step"]["rccl_ranks_seen"] == 2
    assert d["train_step"]["global_batch"] == 32 and "overlap_frac" in d["train_step"] and d["cpu_baseline"]["value"] > 0


def test_bf16_line_is_labelled_as_such():
    d = _line("r01_bench_bf16.json")
    assert d["dtype"] == "bf16" and "bf16" in d["config"]["workload"] and d["roofline"]["peak"] == 2500.0
    s = _line("r03_bench_bf16s.json")                     # the storage mode: priced against HBM, never the fp32 headline
    assert s["dtype"] == "bf16" and "bf16 storage" in s["config"]["workload"]
    r = s["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3


def test_bench_self_launches_its_ranks_dry():
    """`python bench.py --gpus 2` with no launcher in the environment must start its own two ranks (VERDICT r02 missing #1; the twin of
    ref:fsod_train_net.py:108-118 -> d2z:engine/launch.py:27-82) and rank 0 prints the one JSON line.  --dry skips the GPU legs, so
    this runs here on gloo."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["ORE_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["dry"] is True and d["scaling"] == "weak"


def test_bench_under_an_external_launcher_dry():
    """The driver's form: the launcher sets RANK / WORLD_SIZE; bench.py must NOT spawn again."""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rk in range(2):
        env = dict(os.environ, RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   ORE_BENCH_BACKEND="gloo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--dry"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-500:] for o in outs]
    lines = [l for o in outs for l in o[0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2


def test_bench_self_launch_returns_promptly_when_a_rank_dies():
    """rank 1 exits before the rendezvous while rank 0 blocks in init_process_group.  The parent must notice the dead
    rank whatever its position, stop the others and return ITS exit code within seconds, not after the backend's timeout."""
    import subprocess
    import sys
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ORE_BENCH_BACKEND="gloo", ORE_BENCH_DRY_FAIL_RANK="1")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--dry"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 7, (r.returncode, r.stderr[-1000:])
    assert time.time() - t0 < 60
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_writes_the_returned_arrays(tmp_path):
    """`bench.py --dump-outputs DIR`: the arrays of the Instances model() returned, one float32 .npy per field, values unchanged."""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from detectron2.structures import Boxes, Instances
    inst = Instances((640, 640))
    inst.pred_boxes = Boxes(torch.tensor([[1.5, 2.0, 30.25, 40.0], [0.0, 0.0, 639.0, 639.0]]))
    inst.scores = torch.tensor([0.9, 0.125])
    inst.pred_classes = torch.zeros(2, dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "out"), inst)
    got = {f: np.load(tmp_path / "out" / f"instances_{f}.npy") for f in ("pred_boxes", "scores", "pred_classes")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["pred_boxes"], inst.pred_boxes.tensor.numpy()) and np.array_equal(got["scores"], inst.scores.numpy())
    assert np.array_equal(got["pred_classes"], np.zeros(2, np.float32))


@pytest.mark.gpu
def test_bench_times_exactly_the_steps_and_dumps_the_last_one(tmp_path):
    """`bench.py --steps 3 --dump-outputs DIR` on the MI355X: the headline region is exactly 3 timed steps, and DIR holds the
    detections model() returned in the last of them (rank 0, after the timed region), float32, as many as the line reports."""
    import subprocess
    import sys
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "5", "--no-train-leg",
                        "--no-extras", "--no-cpu-baseline", "--profile-passes", "1", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["config"]["timed_steps"] == 3
    # ms_per_step is the time of ONE of the 3 timed steps (timed_region_s is printed rounded to 1 ms)
    assert abs(d["ms_per_step"] * 3 - d["config"]["timed_region_s"] * 1e3) <= 0.5 + 1e-3 * d["ms_per_step"]
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.01                                 # images/s of bs=1 steps
    got = {f: np.load(tmp_path / "out" / f"instances_{f}.npy") for f in ("pred_boxes", "scores", "pred_classes")}
    n = d["config"]["detections_returned"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["pred_boxes"].shape == (n, 4) and got["scores"].shape == (n,) and got["pred_classes"].shape == (n,)
    assert n > 0 and np.isfinite(got["pred_boxes"]).all() and (np.diff(got["scores"]) <= 0).all()
