"""float64 restatements of what the encoder's fine-tune backward adds (csrc/conv_bwd.hip, the stem part of
whisper_ipa_amd/training.py, and the non-causal attention backward at encoder shapes), their float32 evaluations, the float32
evaluation on the bf16 terms a split-product kernel keeps, and the case tables of tests/test_gpu_encoder_training.py.
Plain torch; nothing here touches the GPU at import.  The attention formulation, layouts, head scales and the error measure are
those of tests/backward_ref.py.

  stem_forward / stem_backward     conv1 (k3, p1) + GELU, conv2 (k3, s2, p1) + GELU and their backward, written out tap by tap in
                                   ``dtype``: what test_encoder_training_host.py holds against torch.autograd through F.conv1d / F.gelu.
  *_floor32                        the same formula in float32 on the CPU against float64 on the same inputs: the floor a GPU bound is
                                   margin x.  The kernels' own figures never enter a bound.
  attn_split_floor32               the float32 attention backward with every matmul operand replaced by the bf16 terms the split
                                   kernel keeps (three terms where a product forms a score or a probability gradient, two elsewhere).
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple

import numpy as np
import torch

import backward_ref as BR

STEM_MARGIN = 8.0  # as BR.ATTN_MARGIN

# Every *_FLOOR is the float32 CPU figure that tests/test_encoder_training_host.py measures (worst over the case table, rounded UP);
# every bound is the margin of its section times the floor.  What the kernels measured stands in the GPU tests' docstrings.
# conv stem (whole chain: stem forward kept in f32, then its backward)
STEM_FLOOR = {"dW1": 3.0e-6, "db1": 1.3e-6, "dW2": 3.8e-6, "db2": 6.4e-7, "dz1": 3.0e-6}
STEM_BOUND = {k: STEM_MARGIN * v for k, v in STEM_FLOOR.items()}
# wipa_conv2_dx alone (overlap-add and gelu' on given taps and z1)
CONV2_DX_FLOOR = 8.0e-7
CONV2_DX_BOUND = STEM_MARGIN * CONV2_DX_FLOOR
# attention backward, non-causal, Tq = Tk in ENC_ATTN_TS: the method of tests/test_gpu_backward_kernels.py (ATTN_BOUND) on these shapes
ENC_ATTN_FLOOR = {"dq": 6.6e-5, "dk": 6.8e-5, "dv": 3.7e-5, "dvec": 5.7e-7}
ENC_ATTN_BOUND = {k: BR.ATTN_MARGIN * v for k, v in ENC_ATTN_FLOOR.items()}
# ... with every matmul operand cut to the bf16 terms the split-product kernels keep (attn_backward_split32)
ENC_ATTN_SPLIT_FLOOR = {"dq": 9.4e-5, "dk": 9.7e-5, "dv": 6.2e-5, "dvec": 5.7e-7}
ENC_ATTN_SPLIT_BOUND = {k: BR.ATTN_MARGIN * v for k, v in ENC_ATTN_SPLIT_FLOOR.items()}
STEM_NS = (1, 2, 33, 75)
STEM_OUTPUTS = ("dW1", "db1", "dW2", "db2", "dz1")


class StemCase(NamedTuple):
    N: int
    B: int
    d: int
    n_mels: int


STEM_CASES = [StemCase(N, B, d, n_mels) for N in STEM_NS for B in (1, 3) for d in (64, 128) for n_mels in (80, 128)]


def gelu(z: torch.Tensor) -> torch.Tensor:
    return 0.5 * z * (1.0 + torch.erf(z / np.sqrt(2.0)))


def gelu_grad(z: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(z / np.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


@functools.lru_cache(maxsize=None)
def stem_inputs(case: StemCase) -> Dict[str, torch.Tensor]:
    """float32 mel [B, 2N, n_mels] in the front end's range, conv weights [out, 3, in] (mlx layout) scaled like a trained stem,
    biases, and dx [B, N, d]: the gradient of the stem's output gelu(z2) + positional table"""
    N, B, d, n_mels = case
    g = torch.Generator().manual_seed(N * 1000 + B * 100 + d + n_mels)
    return {"mel": torch.rand(B, 2 * N, n_mels, generator=g) * 2.0 - 1.0,
            "W1": torch.randn(d, 3, n_mels, generator=g) / np.sqrt(3 * n_mels), "b1": torch.randn(d, generator=g) * 0.1,
            "W2": torch.randn(d, 3, d, generator=g) / np.sqrt(3 * d), "b2": torch.randn(d, generator=g) * 0.1,
            "dx": torch.randn(B, N, d, generator=g)}


def stem_forward(x: Dict[str, torch.Tensor], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """-> z1 [B, 2N, d], c1 = gelu(z1), z2 [B, N, d] (pre-activations), u2 = gelu(z2)"""
    mel, W1, b1, W2, b2 = (x[k].to(dtype) for k in ("mel", "W1", "b1", "W2", "b2"))
    B, F, _ = mel.shape
    N = F // 2
    mp = torch.nn.functional.pad(mel, (0, 0, 1, 1))  # a zero frame either side
    z1 = b1 + sum(mp[:, k:k + F] @ W1[:, k, :].T for k in range(3))
    c1 = gelu(z1)
    cp = torch.nn.functional.pad(c1, (0, 0, 1, 1))
    z2 = b2 + sum(cp[:, k:k + F:2][:, :N] @ W2[:, k, :].T for k in range(3))
    return {"z1": z1, "c1": c1, "z2": z2, "u2": gelu(z2)}


def conv2_dx(taps: torch.Tensor, z1: torch.Tensor) -> torch.Tensor:
    """taps [B, N, 3, d], z1 [B, 2N, d] -> dz1 [B, 2N, d] in the documented order: frame s even takes tap 1 of s/2; s odd takes
    tap 2 of (s-1)/2, then + tap 0 of (s+1)/2 when that position exists"""
    B, N = taps.shape[:2]
    dc1 = torch.zeros_like(z1)
    dc1[:, 0::2] = taps[:, :, 1]
    odd = taps[:, :, 2].clone()
    odd[:, : N - 1] = odd[:, : N - 1] + taps[:, 1:, 0]
    dc1[:, 1::2] = odd
    return dc1 * gelu_grad(z1)


def stem_backward(x: Dict[str, torch.Tensor], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The whole stem in ``dtype``: forward, then dz2 = dx gelu'(z2); db2 = sum dz2; dW2[:, k, :] = sum dz2^T c1[2t + k - 1];
    taps = dz2 W2[:, k, :]; dz1 by conv2_dx; db1 = sum dz1; dW1[:, k, :] = sum dz1^T mel[s + k - 1] (frames outside the clip are
    zero).  conv1 has no input gradient."""
    f = stem_forward(x, dtype)
    mel, W2, dx = x["mel"].to(dtype), x["W2"].to(dtype), x["dx"].to(dtype)
    B, F, _ = mel.shape
    N = F // 2
    dz2 = dx * gelu_grad(f["z2"])
    cp = torch.nn.functional.pad(f["c1"], (0, 0, 1, 1))
    dW2 = torch.stack([torch.einsum("bto,bti->oi", dz2, cp[:, k:k + F:2][:, :N]) for k in range(3)], 1)
    taps = torch.stack([dz2 @ W2[:, k, :] for k in range(3)], 2)
    dz1 = conv2_dx(taps, f["z1"])
    mp = torch.nn.functional.pad(mel, (0, 0, 1, 1))
    dW1 = torch.stack([torch.einsum("bso,bsi->oi", dz1, mp[:, k:k + F]) for k in range(3)], 1)
    return {"dW1": dW1, "db1": dz1.sum((0, 1)), "dW2": dW2, "db2": dz2.sum((0, 1)), "dz1": dz1, "taps": taps, **f}


def stem_autograd(x: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """torch.autograd in float64 through F.conv1d / F.gelu as oracle.whisper_ref.encoder_forward spells the stem"""
    from oracle import whisper_ref as R

    F = torch.nn.functional
    W1, b1, W2, b2 = (x[k].double().requires_grad_(True) for k in ("W1", "b1", "W2", "b2"))
    h = x["mel"].double().transpose(1, 2)
    z1 = F.conv1d(h, W1.permute(0, 2, 1), b1, padding=1)
    z1.retain_grad()
    h = R._gelu(z1)
    h = R._gelu(F.conv1d(h, W2.permute(0, 2, 1), b2, stride=2, padding=1)).transpose(1, 2)
    (h * x["dx"].double()).sum().backward()
    return {"dW1": W1.grad, "db1": b1.grad, "dW2": W2.grad, "db2": b2.grad, "dz1": z1.grad.transpose(1, 2)}


@functools.lru_cache(maxsize=None)
def stem_reference(case: StemCase) -> Dict[str, torch.Tensor]:
    """float64 restatement on the inputs of ``case``, computed once and shared; do not modify"""
    return stem_backward(stem_inputs(case))


def stem_errors(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    return {k: BR.err_rms(got[k], ref[k]) for k in STEM_OUTPUTS if k in got}


def stem_floor32(case: StemCase) -> Dict[str, float]:
    """the restatement evaluated in float32 on the CPU (one thread: a floor must not depend on how torch cuts its sums)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = stem_backward(stem_inputs(case), torch.float32)
    finally:
        torch.set_num_threads(threads)
    return stem_errors(got, stem_reference(case))


def conv2_dx_floor32(case: StemCase) -> float:
    """the overlap-add alone: float32 conv2_dx on the float32-rounded float64 taps and z1, against float64 on the same values"""
    ref = stem_reference(case)
    taps, z1 = ref["taps"].float(), ref["z1"].float()
    return BR.err_rms(conv2_dx(taps, z1), conv2_dx(taps.double(), z1.double()))


def encoder_forward64(W: Dict[str, torch.Tensor], dims, mel: torch.Tensor) -> torch.Tensor:
    """AudioEncoder.__call__ in float64 on mel [B, 2N, n_mels] -> [B, N, d]: the oracle's encoder_forward restated without its
    float32 softmax cast (which is what keeps the oracle itself from running in float64).  test_encoder_training_host.py holds
    its float32-rounded result against the oracle's; the distance of the two is the float32 floor of the features."""
    from oracle import whisper_ref as R

    f = torch.float64
    P = {k: v.to(f) for k, v in W.items() if k.startswith("encoder.")}
    ln = torch.nn.functional.layer_norm
    x = stem_forward({"mel": mel, "W1": P["encoder.conv1.weight"], "b1": P["encoder.conv1.bias"], "W2": P["encoder.conv2.weight"],
                      "b2": P["encoder.conv2.bias"]}, f)["u2"]
    B, N, d = x.shape
    H = dims.n_audio_head
    x = x + R.sinusoids(dims.n_audio_ctx, d).to(f)[:N]
    for i in range(dims.n_audio_layer):
        p = f"encoder.blocks.{i}"
        h = ln(x, (d,), P[f"{p}.attn_ln.weight"], P[f"{p}.attn_ln.bias"], 1e-5)
        q = (h @ P[f"{p}.attn.query.weight"].T + P[f"{p}.attn.query.bias"]).view(B, N, H, d // H)
        k = (h @ P[f"{p}.attn.key.weight"].T).view(B, N, H, d // H)
        v = (h @ P[f"{p}.attn.value.weight"].T + P[f"{p}.attn.value.bias"]).view(B, N, H, d // H)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) * (d // H) ** -0.5
        a = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(B, N, d)
        x = x + a @ P[f"{p}.attn.out.weight"].T + P[f"{p}.attn.out.bias"]
        h = ln(x, (d,), P[f"{p}.mlp_ln.weight"], P[f"{p}.mlp_ln.bias"], 1e-5)
        x = x + gelu(h @ P[f"{p}.mlp1.weight"].T + P[f"{p}.mlp1.bias"]) @ P[f"{p}.mlp2.weight"].T + P[f"{p}.mlp2.bias"]
    return ln(x, (d,), P["encoder.ln_post.weight"], P["encoder.ln_post.bias"], 1e-5)


# ====================================================================== attention backward at encoder shapes
ENC_ATTN_TS = (33, 64, 75, 129, 300)
# non-causal, Tq = Tk; layouts alternate and the scales cycle as in BR.ATTN_CASES
ENC_ATTN_CASES: List[BR.AttnCase] = [BR.AttnCase(False, T, T, "ab"[i % 2], BR.QK_SCALES[i % 3]) for i, T in enumerate(ENC_ATTN_TS)]


def bf16_terms(t: torch.Tensor, n: int) -> torch.Tensor:
    """the sum of the first ``n`` bf16 terms of a float32 tensor (hi, hi + mid, hi + mid + lo), as split_bf16x2 / x3 cut them"""
    t = t.float()
    acc = torch.zeros_like(t)
    r = t.clone()
    for _ in range(n):
        h = r.to(torch.bfloat16).float()
        acc = acc + h
        r = r - h
    return acc


def attn_backward_split32(q, k, v, out, lse, d_out, causal: bool, qk_scale: float):
    """BR.attn_backward in float32 with every matmul operand cut to the bf16 terms the split kernel keeps: three terms where the
    product forms a score (Q K^T) or the probability gradient (dO V^T) -- they feed an exponential or a cancelling difference --
    and two terms for the operands of the three output products (dS K, dS^T Q, P^T dO).  Exponentials, D and sums in float32."""
    f = torch.float32
    q, k, v, out, lse, d_out = (t.to(f) for t in (q, k, v, out, lse, d_out))
    vis = BR._visible(q.shape[1], k.shape[1], causal)
    s = torch.einsum("bqhd,bkhd->bhqk", bf16_terms(q, 3), bf16_terms(k, 3))
    p = torch.exp(s - lse[..., None]).masked_fill(~vis, 0.0)
    dvec = (d_out * out).sum(-1).permute(0, 2, 1)
    ds = p * (torch.einsum("bqhd,bkhd->bhqk", bf16_terms(d_out, 3), bf16_terms(v, 3)) - dvec[..., None])
    ds2, p2 = bf16_terms(ds, 2), bf16_terms(p, 2)
    sc = torch.tensor(qk_scale, dtype=f)
    return (torch.einsum("bhqk,bkhd->bqhd", ds2, bf16_terms(k, 2)) * sc, torch.einsum("bhqk,bqhd->bkhd", ds2, bf16_terms(q, 2)) * sc,
            torch.einsum("bhqk,bqhd->bkhd", p2, bf16_terms(d_out, 2)), dvec)


def attn_split_floor32(case: BR.AttnCase) -> Dict[str, float]:
    x, out32, lse32, ref = BR.attn_reference(case)
    dq, dk, dv, dvec = attn_backward_split32(x["q"], x["k"], x["v"], out32, lse32, x["d_out"], case.causal, case.qk_scale)
    return BR.attn_slice_errors({"dq": dq, "dk": dk, "dv": dv, "dvec": dvec}, ref)


def run_attention_bwd_ex(case: BR.AttnCase, f32_split: int):
    """One call of wipa_attention_bwd_ex on the strided, poisoned buffers BR.run_attention_bwd builds for ``case`` (GPU): out / lse are
    the rounded float64 forward.  -> (got {dq, dk, dv, dvec} on the CPU, raw output buffers, expected untouched images)"""
    import ctypes as C

    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    x, out32, lse32, _ = BR.attn_reference(case)
    lay = BR.attn_layout(case)
    ins, outs = BR.attn_buffers(case, lay, x, out32, x["d_out"])
    n_vec = BR.ATTN_B * BR.ATTN_H * case.Tq
    dvec0 = torch.cat([torch.full((n_vec,), float("nan")), torch.full((8,), BR.SENTINEL)])
    shared = case.layout == "a"
    with on_stream() as s:
        dev = {k: v.cuda() for k, v in ins.items()}
        dout = {k: v.cuda() for k, v in outs.items()}
        if shared:
            dev["v"], dout["dv"] = dev["k"], dout["dk"]
        dvec = dvec0.cuda()
        lse_d = lse32.contiguous().cuda()
        a = BR.attn_desc(case, lay, dev, None, dev["o"])
        _lib.check(L.wipa_attention_bwd_ex(C.byref(a), ptr(dev["o"]), ptr(dev["g"]), ptr(lse_d), ptr(dout["dq"]) + 4 * lay["q"].off,
                                           ptr(dout["dk"]) + 4 * lay["k"].off, ptr(dout["dv"]) + 4 * lay["v"].off, ptr(dvec),
                                           case.qk_scale, int(f32_split), sptr(s)), "wipa_attention_bwd_ex")
    torch.cuda.synchronize()
    raw = {k: v.cpu() for k, v in dout.items()}
    raw["dvec"] = dvec.cpu()
    got = {"dq": lay["q"].get(raw["dq"]), "dk": lay["k"].get(raw["dk"]), "dv": lay["v"].get(raw["dv"]),
           "dvec": raw["dvec"][:n_vec].view(BR.ATTN_B, BR.ATTN_H, case.Tq)}
    return got, raw, dict(outs, dvec=dvec0)


def check_attention_bwd_ex(case: BR.AttnCase, bounds: Dict[str, float], f32_split: int) -> Dict[str, float]:
    """BR.check_attention_bwd for wipa_attention_bwd_ex: two runs into fresh buffers bit-equal, the gaps between strided rows
    untouched, no NaN left, per-slice errors against float64 under ``bounds``.  Prints and returns the errors."""
    got, raw, untouched = run_attention_bwd_ex(case, f32_split)
    _, raw2, _ = run_attention_bwd_ex(case, f32_split)
    for name in raw:
        assert BR.bits_equal(raw[name], raw2[name]), (case, name, "two runs differ")
    for name in untouched:
        assert BR.gaps_untouched(raw[name], untouched[name]), (case, name, "written outside its layout")
    errs = BR.attn_slice_errors(got, BR.attn_reference(case)[3])
    print(f"\nattention bwd_ex f32_split={f32_split} {tuple(case)}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < bounds[name], (case, name, e, bounds[name])
    return errs
