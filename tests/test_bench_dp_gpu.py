"""bench.py's multi-rank branch on ONE GPU: two ranks over gloo (ADT_DIST_BACKEND=gloo) through the driver's launch line
(python -m torch.distributed.run ... bench.py --gpus 2).  One JSON line, world_size 2, both scalings in it, and the strong-scaling loss (global
batch 256 split over two ranks) equal to the loss one rank computes on the same global batches after the same number of steps
(sasrec/main.py:146-173 is the step; SURVEY 8e the exactness rules).  Also what a plain one-rank run (no --full) prints and dumps."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env):
    p = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line on stdout, got %d: %r" % (len(lines), lines[:3])
    return json.loads(lines[0])


def test_bench_two_gloo_ranks_one_gpu():
    env = dict(os.environ, ADT_BENCH_BLOCKS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    common = ["--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-ndcg", "--no-roofline"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + common, env)
    assert one["n_gpus"] == 1 and one["config"]["world_size"] == 1 and one["scaling"] == "weak"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(port), "bench.py", "--gpus", "2"] + common, dict(env, ADT_DIST_BACKEND="gloo"))
    assert two["n_gpus"] == 2 and two["config"]["world_size"] == 2 and two["config"]["backend"] == "gloo"
    assert two["scaling"] == "weak" and two["config"]["global_batch"] == 512
    assert "strong" in two and two["strong"]["global_batch"] == 256 and two["strong"]["sequences_per_gpu"] == 128
    for key in ("value", "ms_per_step", "value_incl_h2d", "ms_per_step_incl_h2d"):
        assert two[key] > 0 and two["strong"][key] > 0
    assert two["timing"]["blocks"] == 2
    # the same global batches, the same number of steps: two ranks on half the rows each reproduce the one-rank loss (bf16 kernels; the
    # table-gradient and loss partial sums are split differently over one rank and two, and the loss slots are float atomics: 2e-3)
    assert abs(two["strong"]["loss_last_step"] - one["loss_last_step"]) < 2e-3, (two["strong"]["loss_last_step"], one["loss_last_step"])


def test_plain_run_times_steps_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full): the headline figures only, `steps` as given, and --dump-outputs writes the last timed step's loss,
    gradient norm, weights, Adam moments and logits as float32 .npy files -- the same bits in a second run with the same arguments, and
    in a run with one warm-up step fewer and one timed step more (the run is warmup + steps training steps, however they are split)."""
    out, again, moved = tmp_path / "outputs", tmp_path / "again", tmp_path / "moved"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--dump-outputs"]
    res = _run(cmd + [str(out), "--steps", "3", "--warmup", "2"], dict(os.environ))
    _run(cmd + [str(again), "--steps", "3", "--warmup", "2"], dict(os.environ))
    res_moved = _run(cmd + [str(moved), "--steps", "4", "--warmup", "1"], dict(os.environ))
    assert res_moved["steps"] == 4 and res_moved["warmup"] == 1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 3 and res["warmup"] == 2 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["config"]["table_gradients"].startswith("sorted")
    for key in ("timing", "value_incl_h2d", "ndcg", "roofline", "scatter_mode", "deterministic_mode", "cpu_baseline"):
        assert key not in res, key
    arrays = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(arrays) == {"loss", "grad_norm", "params", "adam_m", "adam_v", "pos_logits", "neg_logits"}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert arrays["pos_logits"].shape == (256, 200) and arrays["params"].shape == arrays["adam_m"].shape == arrays["adam_v"].shape
    assert abs(float(arrays["loss"][0]) - res["loss_last_step"]) < 1e-4
    assert float(np.abs(arrays["adam_m"]).max()) > 0.0
    for other in (again, moved):
        for name, a in arrays.items():      # the loss scalar is summed in float-atomic partial slots (it feeds nothing back): to rounding
            b = np.load(other / (name + ".npy"))
            assert np.allclose(a, b, rtol=1e-6, atol=0) if name == "loss" else np.array_equal(a, b), (other.name, name)
