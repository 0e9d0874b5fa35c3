#!/usr/bin/env python3
"""Benchmark of the RDO-PTQ calibration hot path on MI355X (BASELINE.json metric: calibration images/sec).

Workload (BASELINE.json configs[1]): Cheng2020-anchor N=192, W8 channel-wise `max` init, task-oriented RDO-PTQ calibration,
256 synthetic 256x256 calibration images per GPU, mini-batch B (default 4 = the reference's `--batch_size`, main2.py:31),
input_prob 0.5, round-loss weight 0.01, warmup 0.2, b 20->2 (main2.py:50-62).

A *step* is one calibration iteration (gather -> QDrop -> forward -> round+rec+task loss -> backward -> Adam on alpha;
layer_opt.py:287-309) of EVERY one of the 29 reconstruction units of the model; calibration images/s = units * B * steps /
wall time.  Caches (cached_inps / cached_outs of every unit, built by the product's `save_inp_oup_data`) are resident in
HBM before the timed region.

A plain run does what its headline needs and nothing else: set-up (model, caches, engines), warm-up, the timed steps, the arrays of
`--dump-outputs`, and the JSON line -- `value` / `ms_per_step` = the timed loops, `config` = the workload, library and tuning.
`--full` measures everything else after the timed region and adds it to the line: `sustained_*` (1 000 more steps in windows of
100); `kernels` (per kernel family, event probe) and `roofline`; `dp` (N > 1: wall per iteration and collective time of every unit);
`recon_model_images_per_s` (+ `recon_model_iters_per_unit`, `recon_model_cache_s`) = SURVEY 8d's literal metric, wall of the whole
`recon_model` through the public API with cache building and plan recording inside; `extra` (batch 32 / 64 / 256, one number each
for BASELINE configs 3-5, `dp_overhead_one_rank`: the data-parallel op sequence -- gradient bucket -> RCCL all-reduce -> apply -- on
ONE rank, host-driven and captured, against the single-GPU step); `cpu_baseline`.  The timed steps are the same in both modes.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--images n] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-extras] [--recon-iters n] [--sustain-steps n]]

`--dump-outputs DIR` writes what the timed loops computed in their last step as DIR/*.npy (see `dump_outputs`): with the same
arguments the inputs are the same from run to run, so two builds can be compared output for output.

N > 1: one rank per GPU, each with its own calibration shard and mini-batch (weak scaling), the per-unit alpha-gradient bucket
all-reduced over RCCL every iteration; rank 0 prints ONE JSON line.  Either launched by `python -m torch.distributed.run
--nproc-per-node N bench.py --gpus N ...` (RANK / LOCAL_RANK / WORLD_SIZE in the environment), or plainly as `python bench.py --gpus N`:
this process then starts the N ranks itself as fresh child processes BEFORE it touches a GPU (it never initialises HIP) and exits
with their status.  `--gpus N` with fewer than N visible GPUs, or a WORLD_SIZE that contradicts it, is refused.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rdo-ptq_amd"))

PEAK_F32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0    # same guide, "Peak BF16/FP16 MFMA" (dense)
PEAK_HBM_GBS = 8000.0


MEASURED_F16_MFMA_SUSTAINED_TFLOPS = 1709.0   # tools/micro/mfma_power.hip on MI355X, 16x16x32 f16, random operand bits, every CU busy


ACHIEVABLE_HBM_GBS = 6300.0       # same guide: 6.29 TB/s measured with a float4 copy (79 % of the 8 TB/s specification)

# Kernel FAMILY (prefix of the executor's op tag) -> the MFMA arithmetic it executes.  By family, not by substring: "linear_h2" and
# "linear_wgrad_h2" END in "_h2" and were priced against the fp32 peak by the substring test of rounds 2-5.
_H2 = (PEAK_BF16_MFMA_TFLOPS / 3.0, "fp16 dense MFMA peak 2500 TFLOP/s / 3 products per fp32-equivalent MAC")
_X6 = (PEAK_BF16_MFMA_TFLOPS / 6.0, "bf16 dense MFMA peak 2500 TFLOP/s / 6 products per fp32-equivalent MAC")
_F32 = (PEAK_F32_MFMA_TFLOPS, "fp32 MFMA peak")
KERNEL_FAMILIES = (("conv_fwd_h2", _H2), ("conv_wgrad_h2", _H2), ("linear_h2", _H2), ("linear_wgrad_h2", _H2), ("win_attn_h2", _H2), ("unit1x1_h2", _H2),
                   ("conv_fwd_x6", _X6), ("conv_wgrad_x6", _X6))


def kernel_peak(tag):
    """Dense MFMA peak for the arithmetic a kernel family executes, in ALGORITHMIC (fp32-equivalent) TFLOP/s: the *_x6 kernels issue 6
    bf16 MFMA products per fp32 product (exact 3-way operand split), the *_h2 kernels 3 fp16 products (two-way fp16 split of the
    power-of-two-scaled operands, include/rdo_ptq_hip.h); everything else multiplies on fp32 MFMA."""
    for prefix, peak in KERNEL_FAMILIES:
        if tag == prefix or tag.startswith(prefix + "_"):
            return peak
    return _F32


def kernel_row(tag, launches, ms, flops, nbytes):
    """One row of the line's `kernels` table.  A kernel whose algorithmic intensity (FLOP per algorithmic byte) lies below the ridge
    of ITS pipe -- peak FLOP/s over the achievable HBM rate -- is memory-side: it is reported against bytes (`bound: "hbm"`, fraction
    of the 8 TB/s specification and of the 6.3 TB/s a copy achieves), not against an MFMA peak it cannot reach."""
    row = {"launches_per_step": launches, "ms_per_step": round(ms, 4),
           "tflops": round(flops / (ms * 1e-3) / 1e12, 2) if flops else None,
           "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1) if nbytes else None}
    peak = kernel_peak(tag)[0]
    ridge = peak * 1e12 / (ACHIEVABLE_HBM_GBS * 1e9)
    if flops and nbytes and flops / nbytes >= ridge:
        row.update(bound="mfma", frac_of_peak=round(flops / (ms * 1e-3) / 1e12 / peak, 4), peak_tflops=round(peak, 1))
    elif nbytes:
        gbs = nbytes / (ms * 1e-3) / 1e9
        row.update(bound="hbm", frac_of_peak=round(gbs / PEAK_HBM_GBS, 4), frac_of_achievable_hbm=round(gbs / ACHIEVABLE_HBM_GBS, 4))
        if flops:
            row.update(flop_per_byte=round(flops / nbytes, 1), ridge_flop_per_byte=round(ridge, 1),
                       frac_of_mfma_peak=round(flops / (ms * 1e-3) / 1e12 / peak, 4))
    else:
        row.update(bound=None, frac_of_peak=None)
    return row


def roofline_of(per_tag):
    """The line's `roofline` (the dominant conv kernel against the peak of its pipe) and `kernels` (every family, `kernel_row`) from
    the event probe's {tag: [launches, ms, flops, bytes]} per step."""
    conv = {t: v for t, v in per_tag.items() if t.startswith("conv_")}
    dom = max(conv, key=lambda t: conv[t][1])
    cnt, ms, fl, _ = conv[dom]
    achieved = fl / (ms * 1e-3) / 1e12
    peak, peak_note = kernel_peak(dom)
    kernels = {t: kernel_row(t, *v) for t, v in sorted(per_tag.items(), key=lambda kv: -kv[1][1])}
    traffic, traffic_src = None, None
    for tf in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"):   # HBM-side bytes per launch of the dominant kernel, last committed --pmc passes
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", tf)))
            if dom in tj:
                traffic = round((2 * tj[dom]["fetch_mib_raw"] + tj[dom]["write_mib"]) * 1048576)
                traffic_src = f"profiles/{tf} (rocprofv3 --pmc FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, bytes per launch)"
                break
        except Exception:
            pass
    roofline = {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": round(peak, 1),
                "peak_note": peak_note, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
                "traffic_source": traffic_src,
                "launches_per_step": cnt, "avg_launch_ms": round(ms / cnt, 4),
                "algorithmic_gflop_per_launch": round(fl / cnt / 1e9, 3),
                # what the board's power limit lets nothing-but-MFMA code reach on random fp16 operands (tools/micro/mfma_power.hip,
                # DESIGN 3): 1709 TFLOP/s of v_mfma_f32_16x16x32_f16 at 1.72 GHz -- informative, `frac` stays against the nominal peak
                "power_limited_peak_measured": round(MEASURED_F16_MFMA_SUSTAINED_TFLOPS / 3.0, 1) if kernel_peak(dom) is _H2 else None,
                "frac_of_power_limited_peak": round(achieved / (MEASURED_F16_MFMA_SUSTAINED_TFLOPS / 3.0), 4) if kernel_peak(dom) is _H2 else None}
    return roofline, kernels


def log(*a):
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def usable_cores():
    """Cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = max(1, min(n, q // per))
        except Exception:
            pass
    return n


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--images", type=int, default=256, help="calibration images per GPU")
    ap.add_argument("--N", type=int, default=192, help="Cheng2020 channel width")
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure everything beyond the headline: sustained rate, per-kernel roofline probe, "
                         "data-parallel per-unit probe (N > 1), recon_model wall, extra configurations and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without cpu_baseline")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--cpu-iters", type=int, default=20, help="timed oracle iterations per unit for cpu_baseline")
    ap.add_argument("--recon-iters", type=int, default=2000,
                    help="--full, after the timed region (N = 1 only): wall time of the whole `recon_model` schedule through the public "
                         "layer_/block_reconstruction API with this many iterations per unit (SURVEY 8d's definition of the metric: cache "
                         "building + plan recording + loops); 0: skip")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the extra measurements after the timed region (N = 1 only): batch 32 / 64 / 256 throughput of the "
                         "same workload and one number each for BASELINE configs 3, 4, 5 (tools/bench_configs.py)")
    ap.add_argument("--sustain-steps", type=int, default=1000,
                    help="steps run AFTER the timed region in windows of 100 to report a sustained rate (--full; 0: skip).  The engines "
                         "are recorded for them in every run: the AdaRound schedule spans all of an engine's iterations")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed loops computed in their last step to DIR/<name>.npy (float32, at most 64 MB in all)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


# ----------------------------------------------------------------------------- product side
def seeded_model(N, seed, device, arch="anchor"):
    import lic
    torch.manual_seed(seed)
    model = lic.Cheng2020Attention(N=N) if arch == "attn" else lic.Cheng2020Anchor(N=N)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                       # non-degenerate GDN parameters (default init has gamma = 0.1*I)
        for name, p in model.named_parameters():
            if name.endswith("gamma"):
                c = p.shape[0]
                p.copy_(torch.sqrt(0.1 * torch.eye(c) + 0.002 * torch.rand(c, c, generator=g) + 2.0 ** -36))
    return model.to(device).eval()


def unit_list(qnn):
    """(name, unit) in the order main2.py's recon_model visits them (main2.py:227-253)."""
    from quantization import BaseQuantBlock, QuantModule
    out = []

    def walk(mod, prefix):
        for n, c in mod.named_children():
            if isinstance(c, (QuantModule, BaseQuantBlock)):
                out.append((prefix + n, c))
            else:
                walk(c, prefix + n + ".")
    walk(qnn.model, "")
    return [(n, u) for n, u in out if not (isinstance(u, QuantModule) and u.org_weight is None)]


def build_caches(qnn, units, cali, bs):
    """The caches of every unit through the PRODUCT's cache builder -- `quantization.utils.save_inp_oup_data` with asym=True, the call
    layer_/block_reconstruction make (utils.py:195-258 of the reference): full-precision rows (x_fp, target) and the
    rows behind the quantised prefix (x_q).  The prefix of a unit is what has been calibrated before it; the bench calibrates nothing
    before the timed region, so every unit in front counts as trained at its initial (nearest) rounding -- the values the hooks of
    rounds 1-4 produced with whole-model W8 passes, now through the code path the real flow takes."""
    from quantization import BaseQuantBlock, QuantModule
    from quantization.quant_layer import _nhwc
    from quantization.utils import _FpMemo, save_inp_oup_data
    store = {}
    marked = []
    try:
        for name, u in units:
            (inp_q, inp_fp), out_fp = save_inp_oup_data(qnn, u, cali, asym=True, act_quant=False, batch_size=bs, input_prob=True)
            store[name] = [_nhwc(inp_q), _nhwc(inp_fp), _nhwc(out_fp)]
            for m in u.modules():
                if isinstance(m, (QuantModule, BaseQuantBlock)):
                    m.trained = True
                    marked.append(m)
    finally:
        for m in marked:
            m.trained = False
        _FpMemo.clear()
        qnn.set_quant_state(True, False)
    return store


DUMP_BUDGET_BYTES = 48 * 2 ** 20     # alphas of every unit; the loss rows add a few KB: the whole dump stays under 64 MB
DUMP_SEED = 1005


def dump_outputs(out_dir, engines, last, rank):
    """What a caller of the timed loops receives after their last step (iteration `last` of every engine), as float32 .npy files:

      <unit>.loss.npy          [total, rec+task, round] of that iteration (`UnitEngine.logs`, averaged over the ranks)
      <unit>.<op>.alpha.npy    the op's trained rounding parameters (`UnitEngine.alpha_of`), flattened in the logical weight order

    When all alphas together exceed DUMP_BUDGET_BYTES, every op keeps the same fraction of its elements: the first k of
    randperm(numel) under the generator seed DUMP_SEED, in ascending index order -- a function of the shapes alone.  Collective under
    data parallelism (`logs` all-reduces): every rank calls it, rank 0 writes."""
    rows, alphas = {}, {}
    for uname, e in engines:
        tot, rt, rd = e.logs()
        rows[uname] = torch.stack([tot[last], rt[last], rd[last]]).float()
        for op in e.ops:
            alphas[f"{uname}.{op}"] = e.alpha_of(op).detach().reshape(-1).float().cpu()
    if rank != 0:
        return
    total = sum(v.numel() for v in alphas.values())
    budget = DUMP_BUDGET_BYTES // 4
    os.makedirs(out_dir, exist_ok=True)
    import numpy as np
    nbytes = 0
    for uname, r in rows.items():
        np.save(os.path.join(out_dir, f"{uname}.loss.npy"), r.numpy())
        nbytes += r.numel() * 4
    for key, v in alphas.items():
        if total > budget:
            k = max(1, v.numel() * budget // total)
            pick = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(DUMP_SEED))[:k].sort().values
            v = v[pick]
        np.save(os.path.join(out_dir, f"{key}.alpha.npy"), v.numpy())
        nbytes += v.numel() * 4
    log(f"outputs of step {last} written to {out_dir}: {len(rows) + len(alphas)} arrays, {nbytes / 2 ** 20:.1f} MiB"
        + (f" (alphas sampled: {budget} of {total} elements)" if total > budget else ""))


def gpu_leg(a, rank, world, device):
    from quantization import QuantModel
    from quantization.engine import UnitEngine
    from quantization.recon import _unit_modules
    model = seeded_model(a.N, 1005, device)
    wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
    aq = {"n_bits": 8, "channel_wise": True, "scale_method": "max", "leaf_param": False}
    qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=aq, is_cheng=True).to(device).eval()
    qnn.set_first_last_layer_to_8bit()
    qnn.disable_network_output_quantization()
    g = torch.Generator().manual_seed(1005 + rank)
    cali = torch.rand(a.images, 3, a.crop, a.crop, generator=g).to(device)
    units = unit_list(qnn)
    log(f"model + QuantModel ready, {len(units)} units; building caches for {a.images} images")
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:a.batch])                      # lazy scale init of every weight quantiser (the first forward of main2.py:209-211)
    t0 = time.time()
    caches = build_caches(qnn, units, cali, bs=min(32, a.images))
    torch.cuda.synchronize()
    t_cache = time.time() - t0
    log(f"caches built in {t_cache:.1f}s; recording engines")
    force_dp = bool(os.environ.get("RDO_BENCH_FORCE_DP"))    # exercise the grad -> RCCL all-reduce -> apply sequence on 1 rank
    unit_wall = bool(os.environ.get("RDO_BENCH_UNIT_WALL"))   # diagnostic (--full): per-unit wall time of graph replays after the timed region
    sustain = (a.sustain_steps // 100) * 100
    dp_probe = 10 if (world > 1 or force_dp) else 0             # per-unit wall / collective probe after the timed region (N > 1)
    # The engines have room for everything --full runs after the timed region, in a plain run too: the AdaRound schedule (round-loss
    # warm-up, temperature decay) is laid out over all `iters`, so the timed steps compute the same with and without --full.
    iters = a.warmup + a.steps + sustain + 1 + (a.steps if unit_wall else 0) + dp_probe   # +1: the event-profiled iteration after the timed region
    gi = torch.Generator().manual_seed(77 + rank)
    engines = []
    for name, u in units:
        kind, mods = _unit_modules(u)
        cq, cf, co = caches[name]
        idx = torch.stack([torch.randperm(a.images, generator=gi)[:a.batch] for _ in range(iters)])
        engines.append((name, UnitEngine(kind, mods, cq, cf, co, batch_size=a.batch, iters=iters, weight=0.01,
                                         b_range=(20, 2), warmup=0.2, input_prob=0.5, seed=1005 + rank, idx_table=idx,
                                         use_graph=not a.no_graph, force_dp_split=force_dp)))
    dist = torch.distributed if (world > 1 or force_dp) else None

    def barrier():
        for _, e_ in engines:
            e_.dp_drain()                        # captured data-parallel replays: wait on the heartbeat (stall deadline), then synchronise
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
            torch.cuda.synchronize()

    log("engines recorded; warm-up")
    for _, e in engines:
        e.run(a.warmup)
        e.prepare(a.steps)                       # graph capture of the timed call's replay units is set-up, like the recording
    barrier()
    log("timed region")
    t0 = time.perf_counter()
    for _, e in engines:
        e.run(a.steps)
    barrier()
    dt = time.perf_counter() - t0
    if dist:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    log(f"timed region done: {dt:.3f}s for {a.steps} steps")
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, engines, a.warmup + a.steps - 1, rank)
    if not a.full:                               # the headline is complete: everything below is --full
        check_finite(engines, a.warmup + a.steps)
        return leg_result(engines, dt=dt, t_cache=t_cache)
    # ---- sustained rate: the driver-sized timed region lasts a fraction of a second on a part whose clock moves with load and
    # temperature; run on for `sustain` more steps in windows of 100 (each closed by the same barrier) and report them
    windows = []
    for _ in range(sustain // 100):
        t1 = time.perf_counter()
        for _, e in engines:
            e.run(100)
        barrier()
        w = time.perf_counter() - t1
        if dist:
            tw = torch.tensor([w], device=device, dtype=torch.float64)
            dist.all_reduce(tw, op=dist.ReduceOp.MAX)
            w = float(tw.item())
        windows.append(w / 100 * 1e3)
    if windows:
        log(f"sustained: {sum(windows) / len(windows):.3f} ms/step over {sustain} steps (windows {min(windows):.3f} .. {max(windows):.3f})")
    # ---- N > 1: where a step's time goes, unit by unit -- wall per iteration of the data-parallel loop and the cost of the unit's
    # collective(s) alone (the same persistent bucket, back to back) -- so that a scaling run explains itself
    dp_units = {}
    if dp_probe:
        for uname, e in engines:
            barrier()
            t1 = time.perf_counter()
            e.run(dp_probe)
            torch.cuda.synchronize()
            it_us = (time.perf_counter() - t1) / dp_probe * 1e6
            barrier()
            t1 = time.perf_counter()
            for _ in range(dp_probe):
                e.bucket.reduce()
            torch.cuda.synchronize()
            ar_us = (time.perf_counter() - t1) / dp_probe * 1e6
            dp_units[uname] = {"bucket_kb": round(e.bucket.nbytes() / 1024, 1), "collectives_per_iter": 1 if e.bucket.back is None else 2,
                               "iter_us": round(it_us, 1), "allreduce_us": round(ar_us, 1)}
        log("data-parallel per unit (rank 0): " + "; ".join(f"{n} {d['iter_us']:.0f}us (coll {d['allreduce_us']:.0f}us, {d['bucket_kb']:.0f} KB)"
                                                              for n, d in dp_units.items()))
    if unit_wall:
        for uname, e in engines:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            e.run(a.steps)
            torch.cuda.synchronize()
            log(f"  unit {uname:24s} wall {(time.perf_counter() - t1) / a.steps * 1e3:7.3f} ms/iteration ({e.plan_a.num_ops} ops)")
    # ---- roofline probe: one more iteration of every unit, each op bracketed by hipEvents on the launch stream
    per_tag = {}
    for uname, e in engines:
        info, ms = e.plan_a.op_info(), e.plan_a.profile()
        if os.environ.get("RDO_BENCH_PER_UNIT"):
            agg = {}
            for (tag, fl, by), m in zip(info, ms):
                agg[tag] = agg.get(tag, 0.0) + m
            log(f"  unit {uname:24s} {sum(ms):7.3f} ms  " + " ".join(f"{k}={v:.3f}" for k, v in sorted(agg.items(), key=lambda kv: -kv[1])[:5]))
        e._done += 1
        if getattr(e, "plan_a2", None) is not None:
            info += e.plan_a2.op_info()
            ms += e.plan_a2.profile()
        if e.plan_b is not None:
            if torch.distributed.is_initialized():
                e.bucket.reduce()
            info += e.plan_b.op_info()
            ms += e.plan_b.profile()
        for (tag, fl, by), m in zip(info, ms):
            d = per_tag.setdefault(tag, [0, 0.0, 0.0, 0.0])
            d[0] += 1; d[1] += m; d[2] += fl; d[3] += by
    log("roofline probe done")
    check_finite(engines, a.warmup + a.steps + sustain)
    # ---- "throughput" configurations of SURVEY 8d (outside the timed region): the same schedule at mini-batch 32 and 64
    batch_extra = {}
    if world == 1 and not force_dp and not a.no_extras:
        for bb in (32, 64):
            if bb > a.images:
                continue
            try:
                steps_b = 6
                eb = []
                for name, u in units:
                    kind, mods = _unit_modules(u)
                    cq, cf, co = caches[name]
                    idx = torch.stack([torch.randperm(a.images, generator=gi)[:bb] for _ in range(steps_b + 2)])
                    eb.append(UnitEngine(kind, mods, cq, cf, co, batch_size=bb, iters=steps_b + 2, weight=0.01, b_range=(20, 2), warmup=0.2,
                                         input_prob=0.5, seed=1005, idx_table=idx, use_graph=not a.no_graph))
                for e in eb:
                    e.run(2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for e in eb:
                    e.run(steps_b)
                torch.cuda.synchronize()
                tb = time.perf_counter() - t1
                batch_extra[f"batch{bb}"] = {"images_per_s": round(len(eb) * bb * steps_b / tb, 1), "ms_per_step": round(tb / steps_b * 1e3, 3),
                                             "steps": steps_b}
                log(f"batch {bb}: {tb / steps_b * 1e3:.2f} ms/step = {len(eb) * bb * steps_b / tb:.0f} images/s")
                del eb
                torch.cuda.empty_cache()
            except Exception as ex:      # an extra must never cost the headline
                batch_extra[f"batch{bb}"] = {"error": repr(ex)[:300]}
        # mini-batch 256 (BASELINE.md section 2's largest throughput configuration): the activations of 29 engines at that batch do not fit
        # next to each other, so the units run ONE AT A TIME -- engine built, 1 warm-up + `steps_b` timed iterations between two device
        # synchronisations, engine and its buffers released -- and the rate is units * B * steps / (sum of the units' timed intervals)
        if 256 <= a.images:
            try:
                bb, steps_b, tsum = 256, 3, 0.0
                for name, u in units:
                    kind, mods = _unit_modules(u)
                    cq, cf, co = caches[name]
                    idx = torch.stack([torch.randperm(a.images, generator=gi)[:bb] for _ in range(steps_b + 1)])
                    e = UnitEngine(kind, mods, cq, cf, co, batch_size=bb, iters=steps_b + 1, weight=0.01, b_range=(20, 2), warmup=0.2,
                                   input_prob=0.5, seed=1005, idx_table=idx, use_graph=not a.no_graph)
                    e.run(1)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    e.run(steps_b)
                    torch.cuda.synchronize()
                    tsum += time.perf_counter() - t1
                    if not torch.isfinite(e.logs()[0]).all():
                        raise RuntimeError(f"non-finite loss in unit {name} at batch {bb}")
                    del e
                    torch.cuda.empty_cache()
                batch_extra["batch256_units_in_sequence"] = {"images_per_s": round(len(units) * bb * steps_b / tsum, 1),
                                                              "ms_per_step": round(tsum / steps_b * 1e3, 3), "steps": steps_b,
                                                              "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
                log(f"batch 256 (units in sequence): {tsum / steps_b * 1e3:.2f} ms/step = {len(units) * bb * steps_b / tsum:.0f} images/s")
            except Exception as ex:      # an extra must never cost the headline
                batch_extra["batch256_units_in_sequence"] = {"error": repr(ex)[:300]}
                torch.cuda.empty_cache()
    return leg_result(engines, dt=dt, t_cache=t_cache, per_tag=per_tag, windows=windows, batch_extra=batch_extra, dp_units=dp_units)


def check_finite(engines, n):
    """sanity: the losses of the first `n` iterations of every unit are finite (collective under data parallelism, like `logs`)"""
    for name, e in engines:
        tot, _, _ = e.logs()
        if not torch.isfinite(tot[:n]).all():
            raise RuntimeError(f"non-finite loss in unit {name}")


def leg_result(engines, *, dt, t_cache, per_tag=None, windows=(), batch_extra=None, dp_units=None):
    """What `main` reports of the GPU leg; the measurements after the timed region (--full) are empty in a plain run."""
    h2_units = [n for n, e in engines if getattr(e, "h2_plan", None)]
    # which data-parallel loop ran: "graph" (iteration + collectives replayed from one graph) or "host" (plan / all-reduce / plan)
    dp_paths = sorted({e.dp_path for _, e in engines if e.dp_path is not None})
    dp_fallbacks = sum(e.dp_fallbacks for _, e in engines)
    return dict(dt=dt, n_units=len(engines), per_tag=per_tag or {}, t_cache=t_cache, windows=list(windows), h2_units=h2_units, dp_paths=dp_paths,
                dp_fallbacks=dp_fallbacks, batch_extra=batch_extra or {}, dp_units=dp_units or {})


def dp_overhead_one_rank(a, device, single_ms, steps=12):
    """What the data-parallel op sequence costs BEFORE any second rank exists: every unit recorded with the
    gradient bucket -> all-reduce -> apply split (`force_dp_split`), a one-rank RCCL process group, the same step timed with the
    host-driven loop and with the captured loop (kernels and collectives of an iteration in one graph).  Runs after everything else:
    it creates a process group in this process."""
    from quantization import QuantModel
    from quantization.engine import UnitEngine
    from quantization.recon import _unit_modules
    dist = torch.distributed
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", device_id=device, rank=0, world_size=1)
    res = {"single_gpu_ms_per_step": single_ms, "steps": steps}
    try:
        model = seeded_model(a.N, 1005, device)
        wq = {"n_bits": 8, "channel_wise": True, "scale_method": "max"}
        qnn = QuantModel(model=model, weight_quant_params=wq, act_quant_params=dict(wq, leaf_param=False), is_cheng=True).to(device).eval()
        qnn.set_first_last_layer_to_8bit()
        qnn.disable_network_output_quantization()
        n_img = min(a.images, 32)
        cali = torch.rand(n_img, 3, a.crop, a.crop, generator=torch.Generator().manual_seed(1005)).to(device)
        units = unit_list(qnn)
        qnn.set_quant_state(True, False)
        with torch.no_grad():
            qnn(cali[:a.batch])
        caches = build_caches(qnn, units, cali, bs=min(32, n_img))
        gi = torch.Generator().manual_seed(78)
        for mode in ("host", "graph"):
            os.environ["RDO_DP_GRAPH"] = "1" if mode == "graph" else "0"
            iters = steps + 4
            engines = []
            for name, u in units:
                kind, mods = _unit_modules(u)
                cq, cf, co = caches[name]
                idx = torch.stack([torch.randperm(n_img, generator=gi)[:a.batch] for _ in range(iters)])
                engines.append(UnitEngine(kind, mods, cq, cf, co, batch_size=a.batch, iters=iters, weight=0.01, b_range=(20, 2), warmup=0.2,
                                          input_prob=0.5, seed=1005, idx_table=idx, force_dp_split=True))
            for e in engines:
                e.run(4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in engines:
                e.run(steps)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            paths = sorted({e.dp_path for e in engines if e.dp_path})
            res[mode] = {"ms_per_step": round(ms, 3), "over_single_gpu": round(ms / single_ms - 1.0, 4), "loop": "+".join(paths)}
            log(f"data-parallel sequence on one rank, {mode} loop ({'+'.join(paths)}): {ms:.3f} ms/step = {100 * (ms / single_ms - 1):+.1f} % over {single_ms:.3f}")
            del engines
            torch.cuda.empty_cache()
    finally:
        os.environ.pop("RDO_DP_GRAPH", None)
    return res


# ----------------------------------------------------------------------------- CPU baseline (oracle = "port")
def cpu_leg(a):
    from oracle import lic_oracle as L
    from oracle import rdo_oracle as O
    from oracle.cheng_units import capture_io, schedule
    torch.manual_seed(1005)
    cores = usable_cores()
    torch.set_num_threads(cores)
    log(f"cpu baseline on {cores} threads (os.cpu_count()={os.cpu_count()})")
    model = L.Cheng2020Anchor(N=a.N).eval()
    sched = schedule(model)
    n = a.batch
    x = torch.rand(n, 3, a.crop, a.crop, generator=torch.Generator().manual_seed(1005))
    io = capture_io(model, sched, x)
    iters = 1 + a.cpu_iters
    t_total, img_iters = 0.0, 0
    for name, kind, ops, _ in sched:
        inp, out = io[name]
        inp_q = inp + 1e-3 * torch.randn_like(inp)
        idx = [list(range(n))] * iters
        times = []

        def hook(_grads, times=times):
            times.append(time.perf_counter())
        t0 = time.perf_counter()
        O.reconstruct_unit(kind, ops, inp_q, inp, out, iters=iters, batch_size=n, idx_stream=idx,
                           mask_fn=lambda i, shape: torch.rand(shape) < 0.5, input_prob=0.5, weight=0.01,
                           b_range=(20, 2), warmup=0.2, grad_hook=hook)
        t1 = time.perf_counter()
        # iteration 0 (incl. AdaRound init) is warm-up: time from its grad hook to the end, i.e. `cpu_iters` iterations
        t_total += t1 - times[0]
        img_iters += a.cpu_iters * n
        log(f"  cpu {name}: {(t1 - times[0]) / a.cpu_iters:.2f} s/iter")
    return dict(value=img_iters / t_total, unit="calibration images/s", cores=cores, kind="port",
                sample=f"oracle/rdo_oracle.py reconstruct_unit on torch-CPU fp32, all {len(sched)} units x {a.cpu_iters} timed "
                       f"iteration(s) after 1 warm-up, B={n}, {a.crop}x{a.crop}, {cores} threads")


def visible_gpu_count():
    """GPUs this process would see, counted WITHOUT touching the HIP runtime: KFD topology nodes with compute units
    (/sys/class/kfd/kfd/topology/nodes/*/properties, `simd_count` > 0), capped by ROCR_VISIBLE_DEVICES and HIP_/CUDA_VISIBLE_DEVICES.
    None when the topology is not readable (then every rank checks its own device when it starts).  torch.cuda.device_count() is
    NOT used here: on ROCm without amdsmi it is hipGetDeviceCount, i.e. it opens the runtime in the process that must stay clean."""
    base = "/sys/class/kfd/kfd/topology/nodes"
    if not os.path.isdir("/sys/class/kfd"):
        return 0                                  # no KFD driver: no AMD GPU
    try:
        n = 0
        for node in os.listdir(base):
            props = dict(l.split(None, 1) for l in open(os.path.join(base, node, "properties")).read().splitlines() if " " in l)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except Exception:
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip() != ""]))
    return n


STALL_STATUS = 86                 # a rank whose captured data-parallel loop stopped making progress exits with this (engine.DpStallError)
DEADLINE_S = float(os.environ.get("RDO_BENCH_DEADLINE_S", 1500))   # overall limit of an N > 1 run (the driver's own is 1 800 s)


def _stall_marker(port):
    return f"/tmp/rdo_bench_stall_{port}"


def _watch(procs, deadline, what):
    """Wait for the child processes: the first non-zero exit (or the deadline) stops the others -- they would wait in a collective for
    ever.  Returns the worst status (signal s -> 128 + s; deadline -> 124)."""
    rc = 0
    try:
        while procs:
            for p in list(procs):
                c = p.poll()
                if c is None:
                    continue
                procs.remove(p)
                if c != 0:
                    rc = rc or (c if c > 0 else 128 - c)      # killed by signal s: Popen reports -s
                    print(f"[bench] {what} {p.pid} ended with status {c}: stopping the other ranks", file=sys.stderr, flush=True)
                    for q in procs:
                        q.terminate()
            if procs and time.monotonic() > deadline:
                print(f"[bench] deadline of {DEADLINE_S:.0f} s reached: stopping {len(procs)} {what}(s), no result line", file=sys.stderr, flush=True)
                rc = rc or 124
                for q in procs:
                    q.terminate()
                t_kill = time.monotonic() + 10
                while any(q.poll() is None for q in procs) and time.monotonic() < t_kill:
                    time.sleep(0.2)
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def _die_with_parent():
    """preexec_fn of the rank children: the kernel sends them SIGKILL when the launcher / supervisor that started them dies (a
    supervisor killed with SIGKILL cannot forward anything) -- no orphaned rank keeps a GPU.  Runs between fork and exec in a
    process that never touched the GPU."""
    import ctypes
    import signal
    try:
        ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, signal.SIGKILL)          # PR_SET_PDEATHSIG
    except Exception:
        pass


def _forward_signals(procs):
    """SIGTERM / SIGINT to the launcher or supervisor (torch.distributed.run stops its workers that way) end the rank children too."""
    import signal

    def handler(signum, frame):
        for p in procs:
            if p.poll() is None:
                p.terminate()
        time.sleep(1.0)
        for p in procs:
            if p.poll() is None:
                p.kill()
        os._exit(128 + signum)
    for sig in (signal.SIGTERM, signal.SIGINT):
        try:
            signal.signal(sig, handler)
        except ValueError:           # not the main thread (tests): the parent-death signal still covers the children
            pass


def _rank_cmd():
    """the command of one rank process (a function so that the tests of the launcher can stand a stub in)"""
    return [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]


def launch_ranks(a):
    """`python bench.py --gpus N` without a launcher: start N ranks as fresh child processes (one per GPU, rendezvous on 127.0.0.1)
    and return the worst exit status.  The parent never initialises HIP (a process that has may neither fork GPU children safely
    nor be replaced by exec): devices are counted from sysfs (`visible_gpu_count`).  It is also the watchdog: when one rank exits
    non-zero (or is killed) the others -- which would wait in a collective for ever -- are terminated and the status is non-zero;
    an overall deadline (RDO_BENCH_DEADLINE_S) ends a run that hangs where no rank exits; and when a rank reports that its CAPTURED
    data-parallel loop stalled (status 86) the whole world is started once more, as fresh children, on the host-driven loop
    (RDO_DP_GRAPH=0) -- never a re-exec of a process that touched the GPU.
    Only a single-rank `bench.py` may be run under rocprofv3 (the profiler's preload initialises the GPU in every process it starts).
    RDO_BENCH_SHARE_GPU=1 (tests only, with RDO_BENCH_BACKEND=gloo): every rank uses cuda:0 -- RCCL refuses two ranks on one device,
    gloo with device tensors does not -- so the N-rank code runs on a one-GPU box."""
    import socket
    import subprocess
    share = os.environ.get("RDO_BENCH_SHARE_GPU") == "1"
    have = visible_gpu_count()
    if not share and have is not None and have < a.gpus:
        raise SystemExit(f"bench.py --gpus {a.gpus}: only {have} GPU(s) visible on this box -- refusing to run a smaller world "
                         f"under the label n_gpus={a.gpus}")
    deadline = time.monotonic() + DEADLINE_S
    rc = 0
    for attempt in (0, 1):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        procs = []
        for r in range(a.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK="0" if share else str(r), WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), RDO_BENCH_CHILD="1")
            if attempt:
                env["RDO_DP_GRAPH"] = "0"
            procs.append(subprocess.Popen(_rank_cmd(), env=env, preexec_fn=_die_with_parent))
        _forward_signals(procs)
        rc = _watch(procs, deadline, "rank process")
        stalled = rc == STALL_STATUS or os.path.exists(_stall_marker(port))
        try:
            os.remove(_stall_marker(port))
        except OSError:
            pass
        if rc == 0 or not stalled or attempt or os.environ.get("RDO_DP_GRAPH", "1") != "1":
            break
        print("[bench] the captured data-parallel loop stalled: starting the ranks again on the host-driven loop (RDO_DP_GRAPH=0)",
              file=sys.stderr, flush=True)
    return rc


def supervise_rank():
    """Launched by torch.distributed.run (RANK / WORLD_SIZE in the environment, N > 1): this process stays OFF the GPU and runs the
    actual rank as a fresh child, so that a hang has a way out that is not a re-exec: the child's captured data-parallel loop is
    watched by a heartbeat (engine.UnitEngine._hb_wait); when it stalls, the rank leaves a marker file and exits with status 86;
    every rank's loop stalls with it (a collective blocks all of them) or its child is ended by torch's collective timeout.  Each
    supervisor that finds the marker starts its rank ONCE more on the host-driven loop (RDO_DP_GRAPH=0) with the rendezvous port
    moved by a fixed offset (all supervisors compute the same one).  An overall deadline ends a child that hangs anywhere else."""
    import subprocess
    port = int(os.environ.get("MASTER_PORT", "29517"))
    deadline = time.monotonic() + DEADLINE_S
    rc = 0
    for attempt in (0, 1):
        env = dict(os.environ, RDO_BENCH_CHILD="1")
        if attempt:
            env["RDO_DP_GRAPH"] = "0"
            env["MASTER_PORT"] = str(1024 + (port + 101 - 1024) % (65536 - 1024))
        child = subprocess.Popen(_rank_cmd(), env=env, preexec_fn=_die_with_parent)
        _forward_signals([child])
        rc = _watch([child], deadline, "rank process")
        if rc == 0 or attempt or os.environ.get("RDO_DP_GRAPH", "1") != "1":
            break
        t_wait = time.monotonic() + 30                # another rank may be the one that saw the stall: give its marker a moment
        while rc != STALL_STATUS and not os.path.exists(_stall_marker(port)) and time.monotonic() < t_wait:
            time.sleep(0.5)
        if rc != STALL_STATUS and not os.path.exists(_stall_marker(port)):
            break
        print(f"[bench] rank {os.environ.get('RANK')}: the captured data-parallel loop stalled: starting this rank again on the host-driven "
              "loop (RDO_DP_GRAPH=0)", file=sys.stderr, flush=True)
        time.sleep(3.0)                               # every supervisor reads the marker before rank 0 removes it
    if os.environ.get("RANK", "0") == "0":
        try:
            os.remove(_stall_marker(port))
        except OSError:
            pass
    return rc


def main():
    a = parse()
    if a.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} contradicts WORLD_SIZE={world} (launch with --nproc-per-node {a.gpus})")
    if world > 1 and os.environ.get("RDO_BENCH_CHILD") != "1":
        sys.exit(supervise_rank())                   # launched by torch.distributed.run: the rank itself is a fresh child (see there)
    # The ONE JSON line goes to the real stdout; everything else that lands on fd 1 -- RCCL prints a version banner there when the
    # first communicator is created -- is sent to stderr.
    json_out = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    if torch.cuda.device_count() <= local:
        raise SystemExit(f"bench.py: rank {rank} wants cuda:{local} but only {torch.cuda.device_count()} GPU(s) are visible")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1 or os.environ.get("RDO_BENCH_FORCE_DP"):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        # RDO_BENCH_BACKEND=gloo exists for the tests (two ranks on ONE GPU: RCCL refuses that); measurements use nccl = RCCL
        backend = os.environ.get("RDO_BENCH_BACKEND", "nccl")
        # a collective that does not complete in 180 s ends the process (torch's watchdog): a mismatch on first contact must not cost
        # the whole of the driver's time limit; collectives replayed from a captured graph are watched by the engine's heartbeat instead
        import datetime
        tmo = datetime.timedelta(seconds=float(os.environ.get("RDO_BENCH_COLL_TIMEOUT_S", 180)))
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=device, rank=rank, world_size=world, timeout=tmo)
        else:
            torch.distributed.init_process_group(backend, rank=rank, world_size=world, timeout=tmo)
        from quantization import engine as _engine

        def _stalled(exc_type, exc, tb, _prev=sys.excepthook):
            """A stalled captured loop cannot be torn down (every synchronisation would hang with it): leave the marker for the
            launcher / supervisors and end the process at once."""
            if isinstance(exc, _engine.DpStallError):
                print(f"[bench] {exc}", file=sys.stderr, flush=True)
                try:
                    open(_stall_marker(os.environ.get("MASTER_PORT", "29517")), "w").close()
                except OSError:
                    pass
                os._exit(STALL_STATUS)
            _prev(exc_type, exc, tb)
        sys.excepthook = _stalled
    res = gpu_leg(a, rank, world, device)
    log("gpu leg done")
    n_units, dt = res["n_units"], res["dt"]
    value = n_units * a.batch * a.steps * world / dt
    if rank == 0:
        out = {
            "metric": "calibration images/sec (Cheng2020 W8A8 task-oriented RDO-PTQ, image-iterations over all units)",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"Cheng2020-anchor N={a.N} W8 channel-wise max-init RDO-PTQ calibration, {n_units} units, "
                                   f"{a.images} calib images {a.crop}x{a.crop} per GPU, batch {a.batch} per GPU",
                       "units": n_units, "batch_per_gpu": a.batch, "images_per_gpu": a.images,
                       "parallelism": f"dp{world}", "hipgraph": not a.no_graph,
                       "scaling_note": "weak scaling: every rank calibrates its own shard of `images_per_gpu` images with mini-batch `batch_per_gpu` "
                                       "(global mini-batch = n_gpus x 4) and the per-unit alpha-gradient bucket is all-reduced every iteration; STRONG "
                                       "scaling of the reference's global mini-batch of 4 is not measured (quantization/recon.py refuses a batch that does "
                                       "not split evenly over the ranks: 4 over 8 GPUs)",
                       "gemm_arithmetic": "fp32-EQUIVALENT, not fp32: the convs of every block unit from 32^2 up run on fp16 MFMA with a two-way fp16 "
                                          "split of the power-of-two-scaled operands (3 products, fp32 accumulate, 22 significant operand bits; "
                                          "operands pre-split by their producers = H2 tensors), other large convs on bf16 MFMA with the exact "
                                          "3-way split (6 products), all others on fp32 MFMA",
                       "gemm_error_bound": {"asserted_max_abs_error_over_output_range": 4e-6,
                                            "asserted_vs_exact_fp32_kernel": "<= 2 x the error of the bf16 six-product (exact fp32) kernel on the same inputs",
                                            "measured_vs_fp64": 7.4e-7, "fp32_fma_chain_vs_fp64": 1.5e-6,
                                            "where": "tests/test_gpu_h2.py:80-92 (assert), DESIGN.md section 5 round 3 (measurement)"},
                       "cache_build_s": round(res["t_cache"], 2)},
        }
        if a.full:
            out["roofline"], out["kernels"] = roofline_of(res["per_tag"])
        if res["windows"]:
            w = res["windows"]
            out["sustained_ms_per_step"] = round(sum(w) / len(w), 3)
            out["sustained_steps"] = 100 * len(w)
            out["sustained_value"] = round(n_units * a.batch * world / (sum(w) / len(w) * 1e-3), 2)
            out["sustained_window_ms"] = {"min": round(min(w), 3), "max": round(max(w), 3), "windows_of": 100}
        out["config"]["h2_units"] = res["h2_units"]
        # which library produced the number: a diagnostic build (make DIAG=1: ablation masks and stamps compiled in) is marked, and the
        # kernel-variant switches in force are listed (include/rdo_ptq_hip.h: rdo_get_tuning)
        from hipops import _lib as _L
        ver = _L.lib().rdo_version().decode()
        out["build_mode"] = "diag" if "DIAG" in ver else "release"
        out["config"]["library"] = ver
        out["config"]["tuning"] = {k: int(_L.lib().rdo_get_tuning(k.encode())) for k in
                                   ("conv_x6", "xcd", "graph_unroll", "x6p_halo", "wgrad_p3_row", "h2_stagger", "h2_k32", "h2_n48", "wgrad_sub")}
        if res["dp_paths"]:
            out["dp_graph"] = res["dp_paths"] == ["graph"]
            out["config"]["dp_loop"] = "+".join(res["dp_paths"])
            out["config"]["dp_capture_fallbacks"] = res["dp_fallbacks"]      # units whose capture the ranks agreed to drop (host loop there)
            out["config"]["dp_graph_env"] = os.environ.get("RDO_DP_GRAPH", "1")   # "0": the launcher's retry after a stalled captured loop
        if res["dp_units"]:
            du = res["dp_units"]
            out["dp"] = {"backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
                         "sum_iter_ms": round(sum(d["iter_us"] for d in du.values()) / 1e3, 3),
                         "sum_allreduce_ms": round(sum(d["allreduce_us"] for d in du.values()) / 1e3, 3),
                         "note": "rank 0, after the timed region: wall per iteration of each unit's data-parallel loop and of its collective(s) alone",
                         "units": du}
        if a.full and world == 1 and a.recon_iters > 0 and not os.environ.get("RDO_BENCH_FORCE_DP"):
            # outside the timed region: the metric by SURVEY 8d's literal definition -- wall time of recon_model (main2.py:227-253)
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from full_schedule import run_schedule
            log(f"recon_model wall: {a.recon_iters} iterations x {n_units} units through layer_/block_reconstruction")
            rs = run_schedule(images=a.images, iters=a.recon_iters, batch=a.batch, log=log, quality=False)
            # first-class: SURVEY 8d's LITERAL metric -- image-iterations / wall time of recon_model, caches + recording + loops -- next to
            # `value` (loops only, the driver's timed region) so that the two are never confused; at the reference's 20 000 iterations
            # per unit the set-up amortises further (profiles/r0N_full_schedule.log)
            out["recon_model_images_per_s"] = round(rs["images_per_s"], 1)
            out["recon_model_iters_per_unit"] = a.recon_iters
            out["recon_model_cache_s"] = round(rs["cache_s"], 3)
            out["recon_model"] = {"iters_per_unit": a.recon_iters, "wall_s": round(rs["recon_model_wall_s"], 3),
                                  "cache_s": round(rs["cache_s"], 3), "record_s": round(rs["record_s"], 3), "loop_s": round(rs["loop_s"], 3),
                                  "images_per_s": round(rs["images_per_s"], 1),
                                  "note": "whole schedule through the public API incl. asymmetric cache building and plan recording; the "
                                          "reference's 20000-iteration schedule is timed by tools/full_schedule.py (profiles/)"}
        if a.full and world == 1 and not a.no_extras and not os.environ.get("RDO_BENCH_FORCE_DP"):
            extra = dict(res["batch_extra"])
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_configs
            for key, fn in (("config3_attn_w10", bench_configs.attn_w10), ("config4_lu2022_g_a1", bench_configs.lu2022_unit),
                            ("config4_lu2022_schedule", bench_configs.lu2022_schedule), ("config5_mbt2018_w8a8_eval", bench_configs.mbt2018_eval),
                            ("rd_mode", bench_configs.rd_mode)):
                try:
                    torch.cuda.empty_cache()
                    extra[key] = fn(log=log)
                except Exception as ex:      # an extra must never cost the headline
                    extra[key] = {"error": repr(ex)[:300]}
            try:
                torch.cuda.empty_cache()
                extra["dp_overhead_one_rank"] = dp_overhead_one_rank(a, device, out["ms_per_step"])
            except Exception as ex:          # an extra must never cost the headline
                extra["dp_overhead_one_rank"] = {"error": repr(ex)[:300]}
            out["extra"] = extra
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_leg(a)
            out["cpu_baseline"]["value"] = round(out["cpu_baseline"]["value"], 3)
        print(json.dumps(out), file=json_out, flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
