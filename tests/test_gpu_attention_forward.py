"""Kernel-level parity of the forward attention kernels (csrc/attention.hip) against float64, per query row, through the C ABI:
wipa_flash_attn_enc_bf16 / _f32, wipa_attention, wipa_attention_ragged, wipa_decode_attn (cache layout and through
wipa_decode_cross_attn) and wipa_decode_attn_ragged at their tile edges, strides and kernel switches.  ``pytest -m gpu``.

Common rules (tests/attention_ref.py holds references, inputs, criterion and case tables).  Every case runs in three input regimes
(witness, flat, ramp).  The error of a query row is max_d |got - ref| / A, A = max_d sum_k p_k |v_kd|, and the worst live row of a
case is held to bound = floor constant x margin: the floor is the CPU restatement of the kernel's documented arithmetic on these
very inputs (tests/test_attention_ref_host.py measures it and asserts floor <= constant; the kernels' own figures never enter a
bound), the margin is 3 for bf16 (MFMA accumulation order, v_exp / __expf) and backward_ref.ATTN_MARGIN = 8 for f32 and lse.
Input rows a kernel must not read (beyond the last key, below a ragged start, after the last clip) are NaN.  Every output buffer is
larger than what may be written -- rows after the last, ldo / o_rs gaps -- and filled with SENTINEL, which must come back
bit-identical; what is written starts as NaN.  Dead query rows of ragged cases are not judged but must not be NaN.  Every call runs
twice into fresh buffers and must give the same bits.
"""
import ctypes as C

import pytest
import torch

import attention_ref as AR
import backward_ref as BR
from backward_ref import SENTINEL, bits_equal, gaps_untouched

pytestmark = pytest.mark.gpu

NAN = float("nan")
HD = AR.HD

# ---------------------------------------------------------------------------------------------------------------- bounds
# FLOOR[(family, arithmetic)] = (witness, flat, ramp): the worst live query row of the CPU restatement (attention_ref.restate) against
# float64 over the family's cases, as tests/test_attention_ref_host.py prints it, rounded UP by about a tenth (the figure moves
# in its third digit with the BLAS of the machine that runs the host test, which asserts floor <= constant wherever it runs).
# bound = floor x margin; margin 3 where the arithmetic is bf16, 8 (BR.ATTN_MARGIN) where it is f32.
# "measured" = the worst row of the kernels on the MI355X, same order.
BF16_MARGIN = 3.0
FLOOR = {
    # f32 scores, P rounded to bf16, l from the unrounded p, output rounded to bf16.  floors 3.57e-3, 2.06e-3, 3.51e-3; measured 3.58e-3, 2.06e-3, 3.51e-3
    ("flash_bf16", "bf16"): (3.9e-3, 2.3e-3, 3.9e-3),
    # the float32 softmax statement.  floors 1.22e-6, 2.75e-7, 7.43e-7; measured 1.45e-6, 2.17e-7, 8.25e-7
    ("flash_f32", "f32"): (1.35e-6, 3.0e-7, 8.2e-7),
    # f32 scores, P V on a two-term bf16 split without the low x low product.  floors 6.84e-6, 5.07e-6, 7.35e-6; measured 7.32e-6, 5.07e-6, 7.39e-6
    ("flash_f32", "f32_split"): (7.5e-6, 5.6e-6, 8.1e-6),
    # f32 arithmetic, output rounded to bf16 (every bf16 VALU family below).  floors 3.46e-3, 3.74e-3, 3.42e-3; measured the same
    # three figures: the rounding of the output is all of the error
    ("attn", "bf16"): (3.8e-3, 4.1e-3, 3.8e-3),
    # floors 1.32e-6, 2.60e-7, 5.71e-7; measured 1.14e-6, 1.96e-7, 8.87e-7
    ("attn", "f32"): (1.45e-6, 2.9e-7, 6.3e-7),
    # floors 3.60e-3, 3.68e-3, 3.36e-3; measured the same
    ("attn_ragged", "bf16"): (4.0e-3, 4.0e-3, 3.7e-3),
    # floors 1.01e-6, 3.28e-7, 5.90e-7; measured 6.05e-7, 1.69e-7, 5.48e-7
    ("attn_ragged", "f32"): (1.1e-6, 3.6e-7, 6.5e-7),
    # floors 3.49e-3, 1.71e-3, 3.40e-3; measured the same
    ("decode_cache", "bf16"): (3.8e-3, 1.9e-3, 3.7e-3),
    # floors 6.61e-7, 1.62e-7, 2.40e-7; measured 4.31e-7, 8.37e-8, 2.15e-7
    ("decode_cache", "f32"): (7.3e-7, 1.8e-7, 2.65e-7),
    # floors 2.69e-3, 5.57e-4, 9.55e-4; measured the same
    ("decode_cross", "bf16"): (3.0e-3, 6.1e-4, 1.05e-3),
    # floors 1.24e-6, 1.12e-7, 3.56e-7; measured 1.02e-6, 2.43e-8, 8.10e-8
    ("decode_cross", "f32"): (1.4e-6, 1.25e-7, 3.9e-7),
    # floors 3.22e-3, 9.01e-4, 1.80e-3; measured the same
    ("decode_ragged", "bf16"): (3.5e-3, 1.0e-3, 2.0e-3),
    # floors 4.64e-7, 1.82e-7, 2.14e-7; measured 3.16e-7, 3.45e-8, 1.17e-7
    ("decode_ragged", "f32"): (5.1e-7, 2.0e-7, 2.35e-7),
}
# lse of wipa_attention in f32, |got - ref|: the float32 logsumexp on the CPU over the f32 wipa_attention cases.
# floors 2.80e-6, 5.39e-7, 6.37e-7; measured 2.32e-6, 8.07e-7, 9.76e-7
LSE_FLOOR = (3.1e-6, 5.9e-7, 7.0e-7)


def bound(case: AR.Case, regime: str, f32_split: bool = False) -> float:
    key = AR.floor_key(case, f32_split)
    margin = BF16_MARGIN if key[1] == "bf16" else BR.ATTN_MARGIN
    return FLOOR[key][AR.REGIMES.index(regime)] * margin


def lse_bound(regime: str) -> float:
    return LSE_FLOOR[AR.REGIMES.index(regime)] * BR.ATTN_MARGIN


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _api():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import dt_code, on_stream, ptr, sptr

    return _lib, _lib.lib(), dt_code, on_stream, ptr, sptr


def _full(shape, fill, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (int(shape),), fill, dtype=dtype)


def _out_buffer(idx: torch.Tensor, n: int, dtype):
    """flat output image of n elements: NaN where the kernel writes (idx), SENTINEL everywhere else"""
    assert int(idx.max()) < n
    img = _full(n, SENTINEL, dtype)
    img[idx.reshape(-1)] = NAN
    return img, img.clone()


class Run:
    """what one launch left: got [B, Tq, H, 64] (float32 image), lse [B, H, Tq] or None, raw {name: whole buffer},
    keep {name: image whose SENTINELs must be in raw still}"""

    def __init__(self, got, lse, raw, keep):
        self.got, self.lse, self.raw, self.keep = got, lse, raw, keep


def _launch_flash_bf16(case, x):
    _lib, L, _, on_stream, ptr, sptr = _api()
    B, H, T = case.B, case.H, case.Tq
    D, pad = H * HD, case.variant == "pad"
    Tp = (T + 63) // 64 * 64
    ldqk, ldvt, ldo = 2 * D + (64 if pad else 0), Tp + (64 if pad else 0), D + (8 if pad else 0)
    bf = torch.bfloat16
    qk = _full((B * T + 2, ldqk), NAN, bf)  # gap columns and the rows after the last clip's are NaN
    qk[:B * T, :D] = x["q"].reshape(B * T, D).to(bf)
    qk[:B * T, D:2 * D] = x["k"].reshape(B * T, D).to(bf)
    vt = _full((B, D, ldvt), 1e4 if pad else 0.0, bf)  # the ABI asks for finite columns >= T
    vt[:, :, :T] = x["v"].reshape(B, T, D).transpose(1, 2).to(bf)
    rows = torch.arange(B * T)[:, None] * ldo + torch.arange(D)[None, :]
    img, keep = _out_buffer(rows, (B * T + 2) * ldo + 16, bf)
    with on_stream() as s:
        qk_d, vt_d, out_d = qk.cuda(), vt.cuda(), img.cuda()
        _lib.check(L.wipa_flash_attn_enc_bf16(ptr(qk_d), ldqk, ptr(vt_d), ldvt, ptr(out_d), ldo, B, H, T, sptr(s)),
                   "wipa_flash_attn_enc_bf16")
    torch.cuda.synchronize()
    raw = out_d.cpu()
    return Run(raw[rows.reshape(-1)].view(B, T, H, HD).float(), None, {"out": raw}, {"out": keep})


def _launch_flash_f32(case, x, f32_split):
    _lib, L, _, on_stream, ptr, sptr = _api()
    B, H, T = case.B, case.H, case.Tq
    D = H * HD
    ldo = D + 8
    qk = _full((B * T + 2, 2 * D), NAN, torch.float32)  # q | k in one buffer, as the runtime passes them
    qk[:B * T, :D] = x["q"].reshape(B * T, D)
    qk[:B * T, D:] = x["k"].reshape(B * T, D)
    v = _full((B * T + 2, D), NAN, torch.float32)
    v[:B * T] = x["v"].reshape(B * T, D)
    rows = torch.arange(B * T)[:, None] * ldo + torch.arange(D)[None, :]
    img, keep = _out_buffer(rows, (B * T + 2) * ldo + 16, torch.float32)
    with on_stream() as s:
        qk_d, v_d, out_d = qk.cuda(), v.cuda(), img.cuda()
        _lib.check(L.wipa_flash_attn_enc_f32(ptr(qk_d), 2 * D, ptr(qk_d) + 4 * D, 2 * D, ptr(v_d), D, ptr(out_d), ldo, B, H, T,
                                             int(f32_split), sptr(s)), "wipa_flash_attn_enc_f32")
    torch.cuda.synchronize()
    raw = out_d.cpu()
    return Run(raw[rows.reshape(-1)].view(B, T, H, HD), None, {"out": raw}, {"out": keep})


def _launch_attention(case, x):
    """wipa_attention / wipa_attention_ragged on strided q / k / v views of ONE [B, T, 3, H, 64] buffer"""
    _lib, L, dt_code, on_stream, ptr, sptr = _api()
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    dt = AR.TORCH_DTYPE[case.dtype]
    es = 2 if case.dtype == "bf16" else 4
    T = max(Tq, Tk) + 3
    buf = _full((B, T, 3, H, HD), NAN, dt)  # query rows >= Tq and key rows >= Tk stay NaN
    buf[:, :Tq, 0] = x["q"].to(dt)
    buf[:, :Tk, 1] = x["k"].to(dt)
    buf[:, :Tk, 2] = x["v"].to(dt)
    for b, st in enumerate(case.starts):
        buf[b, :st, 1:] = NAN  # rows below a ragged start
    W = H * HD
    o_rs = W + 8
    o_bs = Tq * o_rs + 16
    b_, t_, h_, d_ = torch.meshgrid(torch.arange(B), torch.arange(Tq), torch.arange(H), torch.arange(HD), indexing="ij")
    idx = b_ * o_bs + t_ * o_rs + h_ * HD + d_
    img, keep = _out_buffer(idx, B * o_bs + 16, dt)
    want_lse = case.dtype == "f32" and not case.starts
    n_vec = B * H * Tq
    lse_img = torch.cat([_full(n_vec, NAN, torch.float32), _full(8, SENTINEL, torch.float32)])
    with on_stream() as s:
        buf_d, out_d, lse_d = buf.cuda(), img.cuda(), lse_img.cuda()
        d = _lib.AttnDesc()
        d.q, d.k, d.v, d.out = ptr(buf_d), ptr(buf_d) + W * es, ptr(buf_d) + 2 * W * es, ptr(out_d)
        d.lse = ptr(lse_d) if want_lse else None
        d.q_bs = d.k_bs = d.v_bs = T * 3 * W
        d.q_rs = d.k_rs = d.v_rs = 3 * W
        d.q_hs = d.k_hs = d.v_hs = HD
        d.o_bs, d.o_rs, d.o_hs = o_bs, o_rs, HD
        d.B, d.H, d.Tq, d.Tk, d.causal, d.dtype = B, H, Tq, Tk, int(case.causal), dt_code(dt)
        if case.variant == "tkdev":  # 40 keys from the descriptor, the rest from the device: only the VALU kernel reads tk_dev
            d.Tk = 40
            tk_d = torch.tensor([Tk - 40], dtype=torch.int32).cuda()
            d.tk_dev = ptr(tk_d)
        if case.starts:
            st_d = torch.tensor(case.starts, dtype=torch.int32).cuda()
            _lib.check(L.wipa_attention_ragged(C.byref(d), ptr(st_d), sptr(s)), "wipa_attention_ragged")
        else:
            _lib.check(L.wipa_attention(C.byref(d), sptr(s)), "wipa_attention")
    torch.cuda.synchronize()
    raw, raw_lse = out_d.cpu(), lse_d.cpu()
    lse = raw_lse[:n_vec].view(B, H, Tq) if want_lse else None
    if not want_lse:
        assert bool(torch.isnan(raw_lse[:n_vec]).all()), "lse written without being asked for"
    return Run(raw[idx.reshape(-1)].view(B, Tq, H, HD).float(), lse, {"out": raw, "lse": raw_lse}, {"out": keep, "lse": lse_img})


def _launch_decode_cache(case, x):
    """wipa_decode_attn / wipa_decode_attn_ragged through the cache layout: q, k, v [B, 448, H * 64], the position on the device"""
    _lib, L, dt_code, on_stream, ptr, sptr = _api()
    B, H, Tk = case.B, case.H, case.Tk
    dt = AR.TORCH_DTYPE[case.dtype]
    pos = Tk - 1
    W = H * HD
    qb, kb, vb = (_full((B, AR.N_CTX, H, HD), NAN, dt) for _ in range(3))  # rows beyond the position stay NaN
    qb[:, pos] = x["q"][:, 0].to(dt)
    kb[:, :Tk] = x["k"].to(dt)
    vb[:, :Tk] = x["v"].to(dt)
    lo = x["lo"][:, 0]
    for b in range(B if case.starts else 0):
        kb[b, :int(lo[b])] = NAN  # rows below the start the kernel uses (a start above the query row is clamped to it)
        vb[b, :int(lo[b])] = NAN
    o_bs = W + 8
    b_, h_, d_ = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(HD), indexing="ij")
    idx = b_ * o_bs + h_ * HD + d_
    img, keep = _out_buffer(idx, (B + 1) * o_bs + 16, dt)
    with on_stream() as s:
        q_d, k_d, v_d, out_d = qb.cuda(), kb.cuda(), vb.cuda(), img.cuda()
        pos_d = torch.tensor([pos], dtype=torch.int32).cuda()
        d = _lib.AttnDesc()
        d.q, d.k, d.v, d.out = ptr(q_d), ptr(k_d), ptr(v_d), ptr(out_d)
        d.tk_dev = d.q_row_dev = ptr(pos_d)
        d.q_bs = d.k_bs = d.v_bs = AR.N_CTX * W
        d.q_rs = d.k_rs = d.v_rs = W
        d.q_hs = d.k_hs = d.v_hs = HD
        d.o_bs, d.o_rs, d.o_hs = o_bs, o_bs, HD
        d.B, d.H, d.Tq, d.Tk, d.causal, d.dtype = B, H, 1, 1, 0, dt_code(dt)
        if case.starts:
            st_d = torch.tensor(case.starts, dtype=torch.int32).cuda()
            _lib.check(L.wipa_decode_attn_ragged(C.byref(d), ptr(st_d), sptr(s)), "wipa_decode_attn_ragged")
        else:
            _lib.check(L.wipa_decode_attn(C.byref(d), sptr(s)), "wipa_decode_attn")
    torch.cuda.synchronize()
    raw = out_d.cpu()
    return Run(raw[idx.reshape(-1)].view(B, 1, H, HD).float(), None, {"out": raw}, {"out": keep})


def _launch_decode_cross(case, x):
    """wipa_decode_cross_attn: q [B, H * 64], kv [B][2H][Tk][64], out [B, H * 64] (the wrapper fixes the strides: rows after the
    last are the only room for a SENTINEL)"""
    _lib, L, dt_code, on_stream, ptr, sptr = _api()
    B, H, Tk = case.B, case.H, case.Tk
    dt = AR.TORCH_DTYPE[case.dtype]
    W = H * HD
    kv = _full(B * 2 * H * Tk * HD + 64, NAN, dt)
    kv[:B * 2 * H * Tk * HD] = torch.cat([x["k"].permute(0, 2, 1, 3), x["v"].permute(0, 2, 1, 3)], 1).reshape(-1).to(dt)
    q = _full(B * W + 64, NAN, dt)
    q[:B * W] = x["q"].reshape(-1).to(dt)
    idx = torch.arange(B * W)
    img, keep = _out_buffer(idx, (B + 2) * W, dt)
    with on_stream() as s:
        q_d, kv_d, out_d = q.cuda(), kv.cuda(), img.cuda()
        _lib.check(L.wipa_decode_cross_attn(ptr(q_d), ptr(kv_d), ptr(out_d), B, H, Tk, dt_code(dt), sptr(s)), "wipa_decode_cross_attn")
    torch.cuda.synchronize()
    raw = out_d.cpu()
    return Run(raw[:B * W].view(B, 1, H, HD).float(), None, {"out": raw}, {"out": keep})


def _launch(case, x, f32_split=False) -> Run:
    if case.family == "flash_bf16":
        return _launch_flash_bf16(case, x)
    if case.family == "flash_f32":
        return _launch_flash_f32(case, x, f32_split)
    if case.family in ("attn", "attn_ragged"):
        return _launch_attention(case, x)
    if case.family == "decode_cross":
        return _launch_decode_cross(case, x)
    return _launch_decode_cache(case, x)


def check_case(case: AR.Case, f32_split: bool = False) -> None:
    """the whole check of one case, in every regime"""
    for regime in AR.REGIMES:
        x, ref = AR.inputs(case, regime), AR.reference(case, regime)
        one, two = _launch(case, x, f32_split), _launch(case, x, f32_split)
        for name in one.raw:
            assert bits_equal(one.raw[name], two.raw[name]), (case.id, regime, name, "two runs differ")
            assert gaps_untouched(one.raw[name], one.keep[name]), (case.id, regime, name, "written outside its layout")
        live = x["live"]
        assert not bool(torch.isnan(one.got[~live]).any()), (case.id, regime, "NaN in a dead query row")
        e, b = AR.worst_row(one.got, ref, live), bound(case, regime, f32_split)
        line = f"\n{case.id}{' split' if f32_split else ''} {regime}: worst row {e:.2e} (bound {b:.2e})"
        if one.lse is not None:
            el = AR.worst_lse(one.lse, ref, live)
            line += f"  lse {el:.2e} (bound {lse_bound(regime):.2e})"
        print(line)
        assert e <= b, (case.id, regime, e, b)
        if one.lse is not None:
            assert el <= lse_bound(regime), (case.id, regime, "lse", el, lse_bound(regime))


def _ids(c):
    return c.id


@pytest.mark.parametrize("case", AR.FLASH_BF16_CASES, ids=_ids)
def test_flash_encoder_bf16_per_row_at_tile_edges_and_strides(case):
    """four waves up to T = 256, eight above; ``pad``: ldqk = 2D + 64, ldvt = ceil64(T) + 64, ldo = D + 8, V^T columns >= T hold 1e4"""
    check_case(case)


@pytest.mark.parametrize("case", AR.FLASH_F32_CASES, ids=_ids)
def test_flash_encoder_f32_per_row_at_tile_edges(case, f32_mode):
    check_case(case, f32_split=(f32_mode == "split"))


@pytest.mark.parametrize("case", AR.ATTN_CASES, ids=_ids)
def test_attention_per_row_on_strided_views_of_one_buffer(case):
    """bf16 and f32 with Tq < 16: the VALU kernel; f32 with Tq >= 16: the f32 MFMA kernel, unless tk_dev is set (``tkdev``: the
    descriptor holds 40 of the 100 keys, so the MFMA kernel, which does not read tk_dev, would miss the bound by far).  f32 checks lse."""
    check_case(case)


@pytest.mark.parametrize("case", AR.ATTN_RAGGED_CASES, ids=_ids)
def test_attention_ragged_per_row_with_nan_below_the_starts(case):
    check_case(case)


@pytest.mark.parametrize("case", AR.DECODE_CACHE_CASES, ids=_ids)
def test_decode_attention_cache_layout_at_its_key_strides(case):
    check_case(case)


@pytest.mark.parametrize("case", AR.DECODE_CROSS_CASES, ids=_ids)
def test_decode_cross_attention_on_both_sides_of_the_long_cache_switch(case):
    check_case(case)


@pytest.mark.parametrize("case", AR.DECODE_RAGGED_CASES, ids=_ids)
def test_decode_attention_ragged_starts_at_the_key_strides_and_above_the_query_row(case):
    check_case(case)
