"""bench.py command-line contract, checked without a GPU except where marked: `--gpus N` must never time
a smaller world under the label n_gpus = N; `--dump-outputs DIR` writes the last timed step's outputs."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus_2_refuses_when_fewer_gpus_are_visible():
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has two GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and "GPU(s) visible" in r.stderr
    assert r.stdout.strip() == ""             # no JSON line for a run that did not happen


def test_gpus_flag_must_agree_with_world_size():
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "contradicts WORLD_SIZE=2" in r.stderr
    assert r.stdout.strip() == ""


def test_steps_must_be_positive():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
    assert r.stdout.strip() == ""


class _StubEngine:
    """What dump_outputs reads from a UnitEngine: `ops`, `logs()` (per-iteration total, rec+task, round) and `alpha_of`."""

    def __init__(self, seed, shapes, iters):
        g = torch.Generator().manual_seed(seed)
        self.ops = {n: None for n in shapes}
        self._alpha = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
        self._logs = [torch.rand(iters, generator=g) for _ in range(3)]

    def logs(self):
        return tuple(self._logs)

    def alpha_of(self, name):
        return self._alpha[name]


def test_dump_outputs_writes_float32_arrays_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import bench
    engines = [("g_a.0", _StubEngine(1, {"conv1": (8, 3, 3, 3), "conv2": (8, 8, 3, 3)}, 10)),
               ("h_s.2.0", _StubEngine(2, {"layer": (16, 8, 5, 5)}, 10))]
    # everything fits: whole alphas in the logical order, the loss row of the requested iteration
    bench.dump_outputs(str(tmp_path / "full"), engines, 6, rank=0)
    names = sorted(p.name for p in (tmp_path / "full").iterdir())
    assert names == ["g_a.0.conv1.alpha.npy", "g_a.0.conv2.alpha.npy", "g_a.0.loss.npy", "h_s.2.0.layer.alpha.npy", "h_s.2.0.loss.npy"]
    for uname, e in engines:
        row = np.load(tmp_path / "full" / f"{uname}.loss.npy")
        assert row.dtype == np.float32 and row.tolist() == [float(t[6]) for t in e.logs()]
        for op in e.ops:
            a = np.load(tmp_path / "full" / f"{uname}.{op}.alpha.npy")
            assert a.dtype == np.float32 and np.array_equal(a, e.alpha_of(op).reshape(-1).numpy())
    # over the budget: every op keeps the same fraction, a fixed sample that depends on the shapes alone
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    total = sum(e.alpha_of(op).numel() for _, e in engines for op in e.ops)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), engines, 9, rank=0)
    nbytes = 0
    for uname, e in engines:
        for op in e.ops:
            a1, a2 = (np.load(tmp_path / d / f"{uname}.{op}.alpha.npy") for d in ("s1", "s2"))
            full = e.alpha_of(op).reshape(-1)
            assert np.array_equal(a1, a2) and a1.size == max(1, full.numel() * 1000 // total)
            assert np.isin(a1, full.numpy()).all()
            nbytes += a1.nbytes
    assert nbytes <= 4 * 1000
    # ranks other than 0 write nothing
    bench.dump_outputs(str(tmp_path / "rank1"), engines, 9, rank=1)
    assert not (tmp_path / "rank1").exists()


@pytest.mark.gpu
def test_dump_outputs_of_a_short_run(tmp_path):
    """`--dump-outputs`: one loss row per unit and every op's alpha of the last timed step, float32 and finite, at most 64 MB; the
    line reports the requested steps and the milliseconds of one of them."""
    import json
    import numpy as np
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--images", "8", "--no-extras", "--no-cpu-baseline", "--sustain-steps", "0",
              "--recon-iters", "0", "--dump-outputs", str(out)], timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert abs(d["value"] - 29 * 4 * 3 / (d["ms_per_step"] * 3 / 1e3)) <= 1e-3 * d["value"]
    files = sorted(out.iterdir())
    assert len([f for f in files if f.name.endswith(".loss.npy")]) == 29
    assert len([f for f in files if f.name.endswith(".alpha.npy")]) >= 29
    assert sum(f.stat().st_size for f in files) <= 64 * 10 ** 6
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), f.name
