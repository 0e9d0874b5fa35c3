"""Float64 reference and float32 restatement of the two kernels of csrc/attn_tape.hip (include/rdo_ptq_attnq.h), on top of
oracle/attention_oracle.py's geometry (`Geom`, `gather`, `scatter`), its `worst_ratio` and its unit roundoff U.  No tests here:
tests/test_attn_tape_args.py (CPU) and tests/test_gpu_attn_tape.py (GPU) share it.

Both kernels take the probabilities, and `probs_bwd` their gradient too, as GIVEN float32 data: they are operands, not results, so the
oracle's error units apply with their given-data terms (dp, ddP) dropped.  u = 2^-24, every unit formed from float64 quantities only:

  pv_bwd      dP_ij   u sum_d |dO_id v_jd|
              dV_jd   u sum_i |pq_ij dO_id|
  probs_bwd   D_i     dD_i   = u sum_j |p_ij g_ij|
              dS_ij   ddS_ij = p_ij dD_i + u p_ij (|g_ij| + |D_i|)
              dQ_id   scale sum_j (ddS_ij |k_jd| + u |dS_ij k_jd|) + u |dQ_id|          (the trailing u: the multiplication by scale)
              dK_jd   sum_i (ddS_ij |scale q_id| + 2u |dS_ij scale q_id|)                (2u: scale q is itself rounded)

Every result also gets an additive floor of 2^-120 x the largest operand magnitude of the call: a sum here has at most 64 products, and
a hardware path may flush each one that falls below 2^-126 (2^-120 = 64 x 2^-126; the operand magnitude scales it to the data).

Float32 restatements (`pv_bwd32`, `probs_bwd32`): torch on the CPU in float32 in the kernels' order -- q scaled first, D and dS from the
float32 p and g, dQ = scale * (dS K), dK = dS^T (scale q); dP = dO V^T and dV = Pq^T dO as plain float32 products.

Inputs (`inputs`): qkv and dout of `attention_cases.trained_like`; probs = the float32 of the float64 reference's probabilities, with
magnitudes below 2^-126 set to 0 (what a float32 forward hands over); probs_q = the static expression of `export.activation_state`'s
docstring at 8 bits on each head's [0, max], in float32 on the CPU; dprobs = randn with per-head scales over two decades."""
import torch

import attention_cases as AC
from oracle import attention_oracle as A

U, F64 = A.U, A.F64
FLOOR = 2.0 ** -120


def static_quant32(x, lo, hi, bits):
    """x [..., C] float32, lo / hi [C]: round(clamp((x - lo) / r, 0, 1) * (2^bits - 1)) / (2^bits - 1) * r + lo, r = max(hi - lo, 1e-6),
    every operation in float32 (quantization/export.py::activation_state)"""
    f32 = torch.float32
    x, lo, hi = x.to(f32), lo.to(f32), hi.to(f32)
    r = torch.clamp(hi - lo, min=1e-6)
    L = torch.tensor(float(2 ** bits - 1), dtype=f32)
    return torch.round(torch.clamp((x - lo) / r, 0, 1) * L) / L * r + lo


def inputs(g, seed):
    """-> dict of float32 CPU tensors: qkv, bias, dout, probs, probs_q, dprobs"""
    qkv, bias, dout = AC.trained_like(g, seed)
    p = A.reference(g, qkv, bias)["probs"]                                        # float64 [windows, N, N, heads]
    probs = torch.where(p.abs() < 2.0 ** -126, torch.zeros_like(p), p).to(torch.float32)
    hi = probs.reshape(-1, g.heads).amax(0)
    probs_q = static_quant32(probs, torch.zeros(g.heads), hi, 8)
    gen = torch.Generator().manual_seed(seed + 1000)
    scales = 10.0 ** (2 * torch.rand(g.heads, generator=gen) - 1)
    dprobs = torch.randn(probs.shape, generator=gen) * scales
    return {"qkv": qkv, "bias": bias, "dout": dout, "probs": probs.contiguous(), "probs_q": probs_q.contiguous(),
            "dprobs": dprobs.contiguous()}


def _heads_first(t, dtype):
    """[windows, N, N, heads] -> [windows, heads, N, N]"""
    return t.detach().to(dtype).permute(0, 3, 1, 2)


def _floor(*operands):
    return FLOOR * max(float(t.detach().abs().max()) for t in operands)


def pv_bwd_reference(g, qkv, probs_q, dout):
    """-> dict: dprobs, u_dprobs [windows, N, N, heads]; dv, u_dv [B, H, W, C]; floor (all float64)"""
    with torch.no_grad():
        v = A.gather(g, qkv.detach().to(F64), 3)[2]
        (dO,) = A.gather(g, dout.detach().to(F64), 1)
        pq = _heads_first(probs_q, F64)
        dP = dO @ v.transpose(-1, -2)
        u_dP = U * (dO.abs() @ v.abs().transpose(-1, -2))
        dV = pq.transpose(-1, -2) @ dO
        u_dV = U * (pq.abs().transpose(-1, -2) @ dO.abs())
        return {"dprobs": dP.permute(0, 2, 3, 1).contiguous(), "u_dprobs": u_dP.permute(0, 2, 3, 1).contiguous(),
                "dv": A.scatter(g, [dV], F64), "u_dv": A.scatter(g, [u_dV], F64), "floor": _floor(qkv, probs_q, dout)}


def pv_bwd32(g, qkv, probs_q, dout):
    """float32 restatement -> dict: dprobs [windows, N, N, heads], dv [B, H, W, C]"""
    f32 = torch.float32
    with torch.no_grad():
        v = A.gather(g, qkv.detach().to(f32).cpu(), 3)[2]
        (dO,) = A.gather(g, dout.detach().to(f32).cpu(), 1)
        pq = _heads_first(probs_q.cpu(), f32)
        return {"dprobs": (dO @ v.transpose(-1, -2)).permute(0, 2, 3, 1).contiguous(), "dv": A.scatter(g, [pq.transpose(-1, -2) @ dO], f32)}


def probs_bwd_reference(g, qkv, probs, dprobs):
    """-> dict: dq, u_dq, dk, u_dk [B, H, W, C]; floor (all float64)"""
    with torch.no_grad():
        q, k, _ = A.gather(g, qkv.detach().to(F64), 3)
        p, gr = _heads_first(probs, F64), _heads_first(dprobs, F64)
        D = (p * gr).sum(-1, keepdim=True)
        dD = U * (p * gr).abs().sum(-1, keepdim=True)
        dS = p * (gr - D)
        ddS = p.abs() * dD + U * p.abs() * (gr.abs() + D.abs())
        dQ = g.scale * (dS @ k)
        dK = g.scale * (dS.transpose(-1, -2) @ q)
        u_dq = g.scale * (ddS @ k.abs() + U * (dS.abs() @ k.abs())) + U * dQ.abs()
        u_dk = g.scale * (ddS.transpose(-1, -2) @ q.abs() + 2 * U * (dS.abs().transpose(-1, -2) @ q.abs()))
        return {"dq": A.scatter(g, [dQ], F64), "u_dq": A.scatter(g, [u_dq], F64), "dk": A.scatter(g, [dK], F64),
                "u_dk": A.scatter(g, [u_dk], F64), "floor": _floor(qkv, probs, dprobs)}


def probs_bwd32(g, qkv, probs, dprobs):
    """float32 restatement in the kernel's order -> dict: dq, dk [B, H, W, C]"""
    f32 = torch.float32
    with torch.no_grad():
        q, k, _ = A.gather(g, qkv.detach().to(f32).cpu(), 3)
        p, gr = _heads_first(probs.cpu(), f32), _heads_first(dprobs.cpu(), f32)
        scale = torch.tensor(g.scale, dtype=f32)
        qs = q * scale
        D = (p * gr).sum(-1, keepdim=True)
        dS = p * (gr - D)
        return {"dq": A.scatter(g, [scale * (dS @ k)], f32), "dk": A.scatter(g, [dS.transpose(-1, -2) @ qs], f32)}


def restatement_ratios(g, inp):
    """-> (pv reference, probs reference, {result: worst err / (unit + floor) of the float32 restatement on `inp`})"""
    pv = pv_bwd_reference(g, inp["qkv"], inp["probs_q"], inp["dout"])
    pb = probs_bwd_reference(g, inp["qkv"], inp["probs"], inp["dprobs"])
    r_pv = pv_bwd32(g, inp["qkv"], inp["probs_q"], inp["dout"])
    r_pb = probs_bwd32(g, inp["qkv"], inp["probs"], inp["dprobs"])
    ratios = {"dprobs": A.worst_ratio(r_pv["dprobs"], pv["dprobs"], pv["u_dprobs"], pv["floor"]),
              "dv": A.worst_ratio(r_pv["dv"], pv["dv"], pv["u_dv"], pv["floor"]),
              "dq": A.worst_ratio(r_pb["dq"], pb["dq"], pb["u_dq"], pb["floor"]),
              "dk": A.worst_ratio(r_pb["dk"], pb["dk"], pb["u_dk"], pb["floor"])}
    return pv, pb, ratios
