"""bench.py's plain line and --dump-outputs: a plain run times exactly --steps steps and carries only the headline fields;
--dump-outputs writes what the last timed step computed, as float32 .npy files within the 64 MB budget, from seeded
inputs that are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures: none of it may appear in (or cost time in) a plain run
FULL_ONLY = ("step_ms", "box", "serialised", "roofline", "roofline_wgrad", "roofline_single", "cpu_baseline",
             "allreduce_exposed_ms_per_step", "allreduce_buckets")


def test_dump_outputs_writes_float32_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = torch.arange(8 * 100, dtype=torch.float64).reshape(8, 100)     # 3200 B as float32
    bench.dump_outputs(str(tmp_path), {"loss": torch.tensor(0.5), "big": big, "more": torch.ones(4, 100)})
    loss, b, more = (np.load(tmp_path / f"{n}.npy") for n in ("loss", "big", "more"))
    assert loss.dtype == b.dtype == more.dtype == np.float32
    assert loss.shape == () and float(loss) == 0.5
    assert np.array_equal(b, big.float().numpy())
    # what is left of the budget (4096 - 4 - 3200 B) holds the first two rows of the last array
    assert more.shape == (2, 100)
    assert sum(a.nbytes for a in (loss, b, more)) <= 4096


def test_param_sample_is_fixed():
    ps = [torch.arange(1000, dtype=torch.float32), torch.arange(1000, 1500, dtype=torch.float32).reshape(20, 25)]
    a, b = bench.param_sample(ps, n=64), bench.param_sample(ps, n=64)
    assert torch.equal(a, b) and a.numel() == 64
    assert torch.equal(a, torch.sort(a).values)            # sorted indices into arange: sorted values
    assert float(a.max()) < 1500 and float(a.min()) >= 0


def _bench(args, tmp_path):
    env = dict(os.environ, BUCTD_BENCH_NO_FIRST_TOUCH="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_plain_line(out, steps, images):
    assert out["steps"] == steps and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(images * 1000.0 / out["ms_per_step"], rel=2e-3)
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in out
    assert not [k for k in FULL_ONLY if k in out]


@pytest.mark.gpu
def test_plain_train_line_and_dumps_repeat(dev, tmp_path):
    args = ["--gpus", "1", "--workload", "train_c2", "--batch", "2", "--steps", "3", "--warmup", "1"]
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _bench(args + ["--dump-outputs", str(d)], tmp_path)
        _check_plain_line(out, 3, 2)
        arrays = {n: np.load(d / f"{n}.npy") for n in ("output", "loss", "preds", "params_sample")}
        assert all(a.dtype == np.float32 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["output"].shape == (2, 17, 64, 48) and arrays["preds"].shape == (2, 17, 2)
        assert arrays["params_sample"].shape == (1 << 20,) and np.isfinite(arrays["params_sample"]).all()
        assert arrays["loss"].shape == () and 0 < float(arrays["loss"]) < 1
        runs.append(arrays)
    # same arguments, same seeded inputs: the two runs compute the same step
    for n in runs[0]:
        np.testing.assert_allclose(runs[0][n], runs[1][n], rtol=1e-4, atol=1e-6, err_msg=n)


@pytest.mark.gpu
def test_plain_infer_line_and_dumps(dev, tmp_path):
    d = tmp_path / "dump"
    out = _bench(["--gpus", "1", "--workload", "infer_c5", "--batch", "2", "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(d)], tmp_path)
    _check_plain_line(out, 2, 2)
    joints, hm = np.load(d / "joints.npy"), np.load(d / "heatmaps.npy")
    assert joints.dtype == hm.dtype == np.float32
    assert joints.shape == (2, 17, 2) and hm.shape == (2, 17, 64, 48)
    assert (joints >= 0).all() and (joints[..., 0] < 192).all() and (joints[..., 1] < 256).all()
