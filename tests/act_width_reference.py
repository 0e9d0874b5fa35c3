"""A restatement of `rdo_actquant_width_scan` (include/rdo_ptq_actbits.h) for the tests: `_score_ref` of test_gpu_actquant_auto.py with the
grid fixed and the width varied.  aq_quant of csrc/actquant.hip one fp32 operation at a time (torch rounds each on its own), the
residual and its square in fp32 as the kernel forms them, only the sums in float64.  Runs on whatever device x is on."""
import torch


def width_scan_ref(x, rng, widths):
    """x [npix, C], rng [2C] = lo | hi (fp32, any device), widths: whole numbers -> (err float64 [C, K], energy float64 [C]) on the CPU"""
    C = x.shape[1]
    lo, hi = rng[:C], rng[C:]
    r = torch.clamp(hi - lo, min=1e-6)
    err = torch.zeros(C, len(widths), dtype=torch.float64)
    for k, b in enumerate(widths):
        R = torch.tensor(float(2 ** b - 1), dtype=torch.float32, device=x.device)
        q = torch.round(torch.clamp((x - lo) / r, 0, 1) * R)
        d = x - ((q / R) * r + lo)
        err[:, k] = (d * d).double().sum(0).cpu()
    return err, (x * x).double().sum(0).cpu()


def rel_err(got, ref):
    """largest relative difference; where the reference is zero the value must be zero"""
    nz = ref != 0
    assert bool((got[~nz] == 0).all())
    return float(((got[nz] - ref[nz]).abs() / ref[nz]).max()) if bool(nz.any()) else 0.0
