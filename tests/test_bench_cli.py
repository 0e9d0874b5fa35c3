"""bench.py command-line contract, checked without a GPU except where marked: `--gpus N` must never time
a smaller world under the label n_gpus = N; `--dump-outputs DIR` writes the last timed step's outputs; `--full` measures more after the
same timed steps."""
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


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full"])
    assert bench.parse().full is True


def test_roofline_of_the_event_probe():
    """`roofline` prices the conv family with the most time per step against the peak of its pipe; `kernels` lists every family,
    longest first."""
    import bench
    per_tag = {"conv_fwd_h2_halo": [12, 1.2, 12 * 40e9, 12 * 100e6],        # [launches, ms, flops, bytes] per step
               "conv_wgrad_64x64": [39, 1.8, 39 * 2e9, 39 * 50e6],
               "ada_step_gather": [105, 1.5, 0.0, 4e9]}
    roof, kernels = bench.roofline_of(per_tag)
    assert list(kernels) == ["conv_wgrad_64x64", "ada_step_gather", "conv_fwd_h2_halo"]
    assert roof["kernel"] == "conv_wgrad_64x64" and roof["launches_per_step"] == 39 and roof["avg_launch_ms"] == round(1.8 / 39, 4)
    assert roof["peak"] == bench.PEAK_F32_MFMA_TFLOPS and roof["achieved"] == round(39 * 2e9 / 1.8e-3 / 1e12, 2)
    assert roof["frac"] == round(39 * 2e9 / 1.8e-3 / 1e12 / bench.PEAK_F32_MFMA_TFLOPS, 4) and roof["power_limited_peak_measured"] is None
    assert kernels["ada_step_gather"]["bound"] == "hbm" and kernels["conv_fwd_h2_halo"]["bound"] == "mfma"
    per_tag["conv_fwd_h2_halo"][1] = 2.0
    roof, _ = bench.roofline_of(per_tag)
    assert roof["kernel"] == "conv_fwd_h2_halo" and roof["peak"] == round(bench.PEAK_BF16_MFMA_TFLOPS / 3.0, 1)
    assert roof["power_limited_peak_measured"] == round(bench.MEASURED_F16_MFMA_SUSTAINED_TFLOPS / 3.0, 1)


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


@pytest.mark.gpu
def test_full_measures_after_the_same_timed_steps(tmp_path):
    """A plain run reports the headline and nothing of `--full`; `--full` adds its measurements after a timed region that computes
    the same: on the headline's workload both dump the same outputs of the last timed step.  The engines of both are recorded for the
    same schedule, so the round loss is off in the same iterations (a schedule recorded for fewer iterations would switch it on
    within these 21 and change every loss row); float atomics may move the last bits from run to run."""
    import json
    import numpy as np
    args = ["--gpus", "1", "--steps", "20", "--warmup", "1", "--no-extras", "--no-cpu-baseline", "--sustain-steps", "100", "--recon-iters", "0"]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full"])):
        r = _run(args + extra + ["--dump-outputs", str(tmp_path / mode)], timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, full = lines["plain"], lines["full"]
    for d in (plain, full):
        assert d["steps"] == 20 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["metric"].startswith("calibration images/sec")
    assert not {"roofline", "kernels", "sustained_ms_per_step", "dp", "recon_model_images_per_s", "extra", "cpu_baseline"} & set(plain)
    assert full["roofline"]["kernel"] in full["kernels"] and full["sustained_steps"] == 100
    names = sorted(f.name for f in (tmp_path / "plain").iterdir())
    assert len(names) > 29 and names == sorted(f.name for f in (tmp_path / "full").iterdir())
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        if n.endswith(".loss.npy"):                  # [total, rec+task, round] of the last timed step
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-9, err_msg=n)
        else:
            assert np.linalg.norm(a - b) <= 1e-4 * np.linalg.norm(b), n
