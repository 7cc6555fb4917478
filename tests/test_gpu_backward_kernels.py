"""Kernel-level parity of the backward kernels (csrc/attention_bwd.hip, csrc/train.hip) against float64, through the C ABI:
tile edges, strided and poisoned buffers, both forms of every two-form kernel, the scales.  ``pytest -m gpu``.

Common rules.  The reference is float64 from the same float32 inputs (tests/backward_ref.py).  The error of an output is
max|t - ref| / rms(ref).  Every output buffer is larger than what the kernel may write: gaps, padding columns and tails hold
SENTINEL and must come back bit-identical; what the ABI documents as overwritten starts as NaN.  Every call runs twice into fresh
buffers and must give the same bits.  Every bound is a named constant = a float32 CPU floor (measured by
tests/test_backward_ref_host.py on these very inputs, never by the kernel) x the margin of its section.
"""
import os
import subprocess
import sys

import pytest
import torch

import backward_ref as BR
from backward_ref import SENTINEL, bits_equal, err_rms

pytestmark = pytest.mark.gpu

NAN = float("nan")

# ---------------------------------------------------------------------------------------------------------------- bounds
# Every *_FLOOR below is the float32 CPU figure of tests/test_backward_ref_host.py, worst over the section's case table, rounded UP
# by about a tenth: the figure moves in its third digit with the vector width and BLAS of the machine that runs the host test,
# and the host test asserts floor <= constant on whatever machine it runs.  "measured" = the kernels on the MI355X.

# Attention backward, per (batch, head) slice.  Floor: the documented formulation in float32 on the CPU (rounded out / lse in),
# worst over the 11 cases: dq 4.95e-5, dk 9.93e-5, dv 7.95e-5, dvec 4.88e-7.  Margin 8 (__expf, the MFMA's accumulation order,
# D from the rounded out).  Measured, MFMA pair | VALU pair: dq 4.5e-5 | 4.9e-5, dk 6.7e-5 | 3.0e-5, dv 8.1e-5 | 3.6e-5, dvec 5.8e-7 | 9.9e-7.
ATTN_FLOOR = {"dq": 5.5e-5, "dk": 1.1e-4, "dv": 8.8e-5, "dvec": 5.4e-7}
ATTN_BOUND = {k: BR.ATTN_MARGIN * v for k, v in ATTN_FLOOR.items()}
# The forward of the chained test (out per slice, lse per slice).  Floor: the float32 softmax statement on the CPU over the three
# chained cases: out 1.31e-5, lse 5.2e-7.  Margin 8 (__expf, __logf).  Measured: out 8.0e-6, lse 2.6e-7.
ATTN_FWD_FLOOR = {"out": 1.45e-5, "lse": 5.8e-7}
ATTN_CHAIN_BOUND = dict(ATTN_BOUND, **{k: BR.ATTN_MARGIN * v for k, v in ATTN_FWD_FLOOR.items()})

# LayerNorm backward, per tensor.  Floor: torch's float32 layer_norm backward on the CPU, one thread (mean / rstd: torch float32),
# worst over the 9 shapes.  Margin 4.  dx_acc is dx added to a random base (accumulate_dx = 1).
# x = randn and 2 randn + 0.5:  floors dx 1.90e-6, dx_acc 1.36e-6, dw 4.57e-6, db 4.38e-6, mean 4.42e-7, rstd 1.08e-7;
# measured dx 1.9e-6, dx_acc 1.1e-6, dw 2.1e-6, db 1.5e-6, mean 4.1e-7, rstd 1.3e-7.
LN_FLOOR = {"dx": 2.1e-6, "dx_acc": 1.5e-6, "dw": 5.0e-6, "db": 4.8e-6, "mean": 4.9e-7, "rstd": 1.2e-7}
LN_BOUND = {k: BR.LN_MARGIN * v for k, v in LN_FLOOR.items()}
# x = 0.05 randn + 30 (offset-dominated: one ulp of x is 4e-5 of its spread):  floors dx 8.24e-5, dx_acc 8.23e-5, dw 1.25e-4,
# db 4.19e-6, mean 1.63e-7, rstd 1.16e-7; measured dx 2.4e-5, dx_acc 2.4e-5, dw 1.2e-4, db 1.6e-6, mean 1.4e-7, rstd 1.4e-7.
LN_OFFSET_FLOOR = {"dx": 9.0e-5, "dx_acc": 9.0e-5, "dw": 1.4e-4, "db": 4.6e-6, "mean": 1.8e-7, "rstd": 1.3e-7}
LN_OFFSET_BOUND = {k: BR.LN_MARGIN * v for k, v in LN_OFFSET_FLOOR.items()}

# Masked CE backward: max|got - ref| * max(count, 1), i.e. in units of probability.  Floor: float32 torch softmax on the CPU,
# worst over V = 1, 37, 512, 513, 5000: 4.37e-8.  Margin 8 (__expf).  Measured: 9.6e-8.
CE_FLOOR = 4.8e-8
CE_BOUND = BR.CE_MARGIN * CE_FLOOR
# The chained test's sum of the masked CE, relative.  float32 torch cross_entropy on the CPU is 3.9e-9 off, less than the one
# rounding the float32 sum itself may cost, so the floor is that rounding, 2^-24 = 6.0e-8.  Margin 8 (__expf, __logf).
# Measured: 3.9e-9 (and 3.5e-8 on the gradient, under CE_BOUND).
CE_SUM_FLOOR = 6.0e-8
CE_SUM_BOUND = BR.CE_MARGIN * CE_SUM_FLOOR

# GELU: the issue's figures.  A float32 evaluation of the kernels' Abramowitz-Stegun 7.1.26 series stays within
# 1.8e-7 max(|z|, 1) on gelu and 2.6e-7 on gelu' (the host test measures 1.43e-7 and 2.15e-7); the bounds are about 4 x those, for
# the GPU's approximate rcp and exp2.  Measured: gelu 1.55e-7 max(|z|, 1), gelu' 1.85e-7 |du|.
GELU_BOUND = 7e-7      # x max(|z|, 1)
GELU_GRAD_BOUND = 1e-6  # x |du|


def _api():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    return _lib, _lib.lib(), on_stream, ptr, sptr


def _buf(n, fill=SENTINEL):
    return torch.full((int(n),), fill, dtype=torch.float32)


# ================================================================================================ 1. attention backward
@pytest.mark.parametrize("case", BR.ATTN_CASES, ids=lambda c: f"{'causal' if c.causal else 'full'}-{c.Tq}x{c.Tk}-{c.layout}")
def test_attention_bwd_float64_parity_at_tile_edges_strides_and_scales(case):
    """wipa_attention_bwd (the f32 MFMA pair) on out / lse of the float64 forward rounded to float32."""
    BR.check_attention_bwd(case, ATTN_BOUND)


@pytest.mark.parametrize("case", BR.ATTN_CHAIN_CASES, ids=lambda c: f"{'causal' if c.causal else 'full'}-{c.Tq}x{c.Tk}-{c.layout}")
def test_attention_forward_then_backward_chain(case):
    """wipa_attention -> wipa_attention_bwd as the trainer chains them; the forward's out and lse are checked too (13 queries:
    the VALU forward with lse)."""
    BR.check_attention_bwd(case, ATTN_CHAIN_BOUND, chain=True)


def test_attention_bwd_valu_pair_in_a_subprocess():
    """WIPA_ATTN_BWD=valu (read once per process): the A/B baseline walks the same table under the same bounds."""
    code = ("import sys, os\nsys.path.insert(0, os.path.join(os.getcwd(), 'tests'))\nimport backward_ref as BR\n"
            f"w = BR.check_attention_table({ATTN_BOUND!r})\nprint('OK', w)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WIPA_ATTN_BWD="valu", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=root)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:] + r.stdout[-1500:]


def test_attention_bwd_refuses_a_misaligned_batch_stride():
    _lib, L, *_ = _api()
    case = BR.ATTN_CASES[1]
    rc, _, raw, untouched, _ = BR.run_attention_bwd(case, q_bs_delta=2)
    assert rc != 0 and b"wipa_attention_bwd" in L.wipa_last_error()
    for name, image in untouched.items():
        assert bits_equal(raw[name], image), name


# ================================================================================================ 2. LayerNorm backward
def _ln_call(x, dy, w, dx0, acc, stats_floats, rows, D, alloc_floats=None):
    """-> rc, dx, dw, db, stats (CPU).  dw / db [D + 8], stats [alloc + 8]: NaN where written, SENTINEL tails."""
    _lib, L, on_stream, ptr, sptr = _api()
    alloc = stats_floats if alloc_floats is None else alloc_floats
    with on_stream() as s:
        xd, dyd, wd = x.cuda(), dy.cuda(), w.cuda()
        dx = torch.cat([dx0.reshape(-1), _buf(8)]).cuda()
        dw, db = torch.cat([_buf(D, NAN), _buf(8)]).cuda(), torch.cat([_buf(D, NAN), _buf(8)]).cuda()
        stats = torch.cat([_buf(alloc, NAN), _buf(8)]).cuda()
        rc = L.wipa_layernorm_bwd(ptr(xd), ptr(dyd), ptr(wd), ptr(dx), acc, ptr(dw), ptr(db), ptr(stats), stats_floats, rows, D,
                                  BR.LN_EPS, sptr(s))
    torch.cuda.synchronize()
    return rc, dx.cpu(), dw.cpu(), db.cpu(), stats.cpu()


@pytest.mark.parametrize("rows,D", BR.LN_CASES)
def test_layernorm_bwd_float64_parity(rows, D):
    """three input families x scratch for one chunk / for the chunked column sums x accumulate_dx 0 / 1"""
    worst = [dict.fromkeys(BR.LN_OUTPUTS, 0.0), dict.fromkeys(BR.LN_OUTPUTS, 0.0)]
    for fam in range(len(BR.LN_FAMILIES)):
        x, ref = BR.ln_inputs(rows, D, fam), BR.ln_reference(rows, D, fam)
        off = int(fam == 2)
        bound = LN_OFFSET_BOUND if off else LN_BOUND
        for stats_floats in (2 * rows, 2 * rows + 64 * D):
            for acc in (0, 1):
                dx0 = x["base"] if acc else torch.full((rows, D), NAN)
                runs = [_ln_call(x["x"], x["dy"], x["w"], dx0, acc, stats_floats, rows, D) for _ in range(2)]
                (rc, dx, dw, db, stats), second = runs
                assert rc == 0 and second[0] == 0
                for a, b in zip(runs[0][1:], second[1:]):
                    assert bits_equal(a, b), "two runs differ"
                for t, n in ((dx, rows * D), (dw, D), (db, D), (stats, stats_floats)):
                    assert bool((t[n:] == SENTINEL).all()), "tail overwritten"
                st = stats[:2 * rows].view(rows, 2)
                got = {("dx_acc" if acc else "dx"): dx[:rows * D].view(rows, D), "dw": dw[:D], "db": db[:D], "mean": st[:, 0],
                       "rstd": st[:, 1]}
                for k, t in got.items():
                    e = err_rms(t, ref[k])
                    worst[off][k] = max(worst[off][k], e)
                    assert e < bound[k], (rows, D, fam, stats_floats, acc, k, e, bound[k])
    print(f"\nlayernorm bwd {rows}x{D}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst[0].items()) + "  | offset family: " +
          "  ".join(f"{k} {v:.2e}" for k, v in worst[1].items()))


def test_layernorm_bwd_db_is_exact_on_integer_dy():
    """dy integer in -3 .. 3: every partial sum is exact in float32, so db == the integer column sums in both forms"""
    rows, D = 2100, 256
    x = BR.ln_inputs(rows, D, 1, True)
    want = x["dy"].double().sum(0).float()
    for stats_floats in (2 * rows, 2 * rows + 64 * D):
        rc, _, _, db, _ = _ln_call(x["x"], x["dy"], x["w"], torch.full((rows, D), NAN), 0, stats_floats, rows, D)
        assert rc == 0 and torch.equal(db[:D], want), stats_floats


@pytest.mark.parametrize("rows,D,short", [(5, 2052, 0), (5, 130, 0), (5, 128, 1)])
def test_layernorm_bwd_refusals_write_nothing(rows, D, short):
    g = torch.Generator().manual_seed(D)
    x, dy, w = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g), torch.randn(D, generator=g)
    alloc = 2 * rows + 64 * D
    rc, dx, dw, db, stats = _ln_call(x, dy, w, torch.full((rows, D), SENTINEL), 0, 2 * rows - 1 if short else alloc, rows, D, alloc)
    assert rc != 0
    assert bool((dx == SENTINEL).all()) and bool(torch.isnan(dw[:D]).all()) and bool(torch.isnan(db[:D]).all())
    assert bool(torch.isnan(stats[:alloc]).all()) and bool((stats[alloc:] == SENTINEL).all())


# ================================================================================================ 3. masked CE backward
def _ce_bwd_call(logits_pad, ldl, tok, ld_tok, V, mask, count):
    _lib, L, on_stream, ptr, sptr = _api()
    with on_stream() as s:
        lg, tk, mk = logits_pad.clone().cuda(), tok.cuda(), mask.cuda()
        cnt = torch.tensor([count, NAN], dtype=torch.float32).cuda()
        _lib.check(L.wipa_masked_ce_bwd(ptr(lg), ldl, ptr(tk), ld_tok, BR.CE_B, BR.CE_T, V, ptr(mk), ptr(cnt), sptr(s)))
    torch.cuda.synchronize()
    return lg.cpu()


def _ce_tokens(tgt, ld_tok):
    """[B, ld_tok] int32: row b = (an input token, the T targets, then values no column equals)"""
    tok = torch.full((BR.CE_B, ld_tok), 1 << 30, dtype=torch.int32)
    tok[:, 0] = 1 << 29
    tok[:, 1:BR.CE_T + 1] = tgt.view(BR.CE_B, BR.CE_T).to(torch.int32)
    return tok


@pytest.mark.parametrize("V", BR.CE_VS)
def test_masked_ce_bwd_float64_parity(V):
    logits, tgt = BR.ce_inputs(V)
    rows, ldl, ld_tok = BR.CE_B * BR.CE_T, (V + 31) // 32 * 32 + 32, BR.CE_T + 4
    pad = torch.full((rows, ldl), SENTINEL)
    pad[:, :V] = logits
    mask = torch.tensor(BR.CE_MASK, dtype=torch.float32)
    assert mask[0] == 0 and mask[-1] == 0 and all(mask[r] == 1 for r in (BR.CE_ROW_TARGET_SPIKE, BR.CE_ROW_OTHER_SPIKE, BR.CE_ROW_CONSTANT))
    worst = 0.0
    for count in BR.CE_COUNTS:
        got = _ce_bwd_call(pad, ldl, _ce_tokens(tgt, ld_tok), ld_tok, V, mask, count)
        assert bits_equal(got, _ce_bwd_call(pad, ldl, _ce_tokens(tgt, ld_tok), ld_tok, V, mask, count)), "two runs differ"
        assert bool((got[:, V:] == SENTINEL).all()), "padding columns overwritten"
        assert bits_equal(got[mask == 0][:, :V], torch.zeros(int((mask == 0).sum()), V)), "masked rows must be exactly +0"
        ref = BR.ce_backward(logits, tgt, mask, count)
        e = float((got[:, :V].double() - ref).abs().max()) * max(count, 1.0)
        assert e == e and e < CE_BOUND, (V, count, e, CE_BOUND)
        worst = max(worst, e)
    print(f"\nmasked CE bwd V={V}: worst error {worst:.2e} (probability units)")


def test_masked_ce_then_backward_chain():
    """wipa_masked_ce -> wipa_masked_ce_bwd at V = 513 against float64 autograd of the masked mean CE with the oracle's mask"""
    _lib, L, on_stream, ptr, sptr = _api()
    logits, tokens = BR.ce_chain_inputs()
    sum_ref, n_ref, grad_ref, mask_ref = BR.ce_chain_reference()
    V, B, T = BR.CE_CHAIN_V, BR.CE_B, BR.CE_T
    rows, ldl, ld_tok = B * T, (V + 31) // 32 * 32 + 32, T + 1 + 3
    pad = torch.full((rows, ldl), SENTINEL)
    pad[:, :V] = logits
    tok = torch.full((B, ld_tok), 1 << 30, dtype=torch.int32)
    tok[:, :T + 1] = tokens.to(torch.int32)
    res = []
    for _ in range(2):
        with on_stream() as s:
            lg, tk = pad.clone().cuda(), tok.cuda()
            row_buf = torch.cat([_buf(2 * rows, NAN), _buf(8)]).cuda()
            out2 = torch.cat([_buf(2, NAN), _buf(6)]).cuda()
            _lib.check(L.wipa_masked_ce(ptr(lg), ldl, ptr(tk), ld_tok, B, T, V, BR.CE_CHAIN_EOT, ptr(row_buf), ptr(out2), sptr(s)))
            _lib.check(L.wipa_masked_ce_bwd(ptr(lg), ldl, ptr(tk), ld_tok, B, T, V, ptr(row_buf) + 4 * rows, ptr(out2) + 4, sptr(s)))
        torch.cuda.synchronize()
        res.append((lg.cpu(), row_buf.cpu(), out2.cpu()))
    (lg, row_buf, out2), second = res
    assert all(bits_equal(a, b) for a, b in zip(res[0], second)), "two runs differ"
    assert bool((lg[:, V:] == SENTINEL).all()) and bool((row_buf[2 * rows:] == SENTINEL).all()) and bool((out2[2:] == SENTINEL).all())
    assert torch.equal(row_buf[rows:2 * rows], mask_ref.float()) and float(out2[1]) == n_ref
    e_sum = abs(float(out2[0]) - float(sum_ref)) / float(sum_ref)
    e = float((lg[:, :V].double() - grad_ref).abs().max()) * max(n_ref, 1.0)
    print(f"\nmasked CE chain: sum {float(out2[0]):.6f} vs {float(sum_ref):.6f} (rel {e_sum:.2e}), gradient error {e:.2e}")
    assert e_sum < CE_SUM_BOUND and e == e and e < CE_BOUND, (e_sum, e)


# ================================================================================================ 4. embedding backward
@pytest.mark.parametrize("B,T,D", BR.EMB_CASES)
def test_embed_bwd_is_bit_equal_to_the_sequential_float32_loop(B, T, D):
    _lib, L, on_stream, ptr, sptr = _api()
    tok, dx, d_tok0 = BR.embed_inputs(B, T, D)
    flat = tok.reshape(-1)
    assert (tok[0, 1:4] == tok[0, 1]).all() and (tok[:, T - 1] == tok[0, T - 1]).all() and 0 in flat and BR.EMB_VOCAB - 1 in flat
    want_tok, want_pos = BR.embed_backward_sequential(tok, dx, d_tok0)
    res = []
    for _ in range(2):
        with on_stream() as s:
            tk, dxd = flat.contiguous().cuda(), dx.cuda()
            d_tok = torch.cat([d_tok0.reshape(-1), _buf(8)]).cuda()
            d_pos = _buf((T + 3) * D, NAN).cuda()
            _lib.check(L.wipa_embed_bwd(ptr(tk), ptr(dxd), B, T, D, ptr(d_tok), ptr(d_pos), sptr(s)))
        torch.cuda.synchronize()
        res.append((d_tok.cpu(), d_pos.cpu()))
    (d_tok, d_pos), second = res
    assert bits_equal(d_tok, second[0]) and bits_equal(d_pos, second[1]), "two runs differ"
    assert bool((d_tok[BR.EMB_VOCAB * D:] == SENTINEL).all()) and bool(torch.isnan(d_pos[T * D:]).all())
    got_tok = d_tok[:BR.EMB_VOCAB * D].view(BR.EMB_VOCAB, D)
    assert bits_equal(got_tok, torch.from_numpy(want_tok)), "token rows: not the documented order"
    assert bits_equal(d_pos[:T * D].view(T, D), torch.from_numpy(want_pos)), "position rows: not the documented order"
    absent = [v for v in range(BR.EMB_VOCAB) if v not in set(flat.tolist())]
    assert absent and bits_equal(got_tok[absent], d_tok0[absent])


# ================================================================================================ 5. column sums, transpose, GELU
def _colsum_call(xd, ld, rows, cols, out0, acc, ws_floats):
    """ws_floats < 0: no workspace.  -> out [cols + 8], workspace [max(ws, 0) + 8] on the CPU"""
    _lib, L, on_stream, ptr, sptr = _api()
    with on_stream() as s:
        out = torch.cat([out0, _buf(8)]).cuda()
        ws = _buf(max(ws_floats, 0) + 8).cuda()
        _lib.check(L.wipa_colsum(ptr(xd), ld, rows, cols, ptr(out), acc, ptr(ws) if ws_floats >= 0 else None, max(ws_floats, 0), sptr(s)))
    torch.cuda.synchronize()
    return out.cpu(), ws.cpu()


@pytest.mark.parametrize("cols", BR.COLSUM_COLS)
def test_colsum_exact_on_integers_and_within_the_path_bound_on_randn(cols):
    """rows around the 4 x 8 unroll, the 512-row threshold of the chunked form and the 64-chunk cap; both forms x accumulate;
    workspace absent / exactly R cols / one float less (R drops by one) / room for fewer than two chunks.
    integers in -8 .. 8: bit-equal to the exact sums (one dropped or doubled row fails).  randn: per column
    |err| <= k 2^-24 sum|x| with k = backward_ref.colsum_path_adds (derivation in its docstring)."""
    ld = cols + 7
    worst = 0.0
    for integer in (True, False):
        x, base, run, run_abs = BR.colsum_inputs(cols, integer)
        xd = x.cuda()
        for rows in BR.COLSUM_ROWS:
            full = min(64, (rows + 255) // 256) * cols
            for ws_floats in (-1, full, full - 1, 2 * cols - 1):
                R = BR.colsum_chunks(rows, cols, ws_floats)
                for acc in (0, 1):
                    out0 = base if acc else _buf(cols, NAN)
                    out, ws = _colsum_call(xd, ld, rows, cols, out0, acc, ws_floats)
                    out_b, ws_b = _colsum_call(xd, ld, rows, cols, out0, acc, ws_floats)
                    assert bits_equal(out, out_b) and bits_equal(ws, ws_b), "two runs differ"
                    used = R * cols if R > 1 else 0
                    assert bool((ws[used:] == SENTINEL).all()) and bool((out[cols:] == SENTINEL).all()), (rows, ws_floats, R)
                    ref = run[rows - 1] + (base.double() if acc else 0.0)
                    if integer:
                        assert torch.equal(out[:cols].double(), ref), (rows, ws_floats, acc, R)
                    else:
                        k = BR.colsum_path_adds(rows, R, acc)
                        lim = k * 2.0 ** -24 * (run_abs[rows - 1] + (base.double().abs() if acc else 0.0))
                        d = (out[:cols].double() - ref).abs()
                        assert bool((d <= lim).all()), (rows, ws_floats, acc, R, float((d / lim).max()))
                        worst = max(worst, float((d / lim).max()))
    print(f"\ncolsum cols={cols}: worst randn error / (k 2^-24 sum|x|) = {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,rows_pad", BR.TRANSPOSE_CASES)
def test_transpose_bits_zero_padding_and_untouched_columns(rows, cols, rows_pad, dtype):
    _lib, L, on_stream, ptr, sptr = _api()
    g = torch.Generator().manual_seed(rows + cols)
    ld_in, ld_out = cols + 3, rows_pad + 5
    a = torch.full((rows, ld_in), NAN)
    a[:, :cols] = torch.randn(rows, cols, generator=g)
    a = a.to(dtype)
    res = []
    for _ in range(2):
        with on_stream() as s:
            ad = a.cuda()
            out = torch.full((cols * ld_out + 8,), SENTINEL).to(dtype).cuda()
            _lib.check(L.wipa_transpose(ptr(ad), ld_in, ptr(out), ld_out, rows, cols, rows_pad, 0 if dtype == torch.float32 else 1, sptr(s)))
        torch.cuda.synchronize()
        res.append(out.cpu())
    out = res[0]
    assert bits_equal(out, res[1]), "two runs differ"
    body = out[:cols * ld_out].view(cols, ld_out)
    sent = torch.tensor(SENTINEL).to(dtype)
    assert bits_equal(body[:, :rows], a[:, :cols].T.contiguous())
    assert bits_equal(body[:, rows:rows_pad], torch.zeros(cols, rows_pad - rows, dtype=dtype)), "padding must be +0"
    assert bool((body[:, rows_pad:] == sent).all()) and bool((out[cols * ld_out:] == sent).all())


def test_gelu_and_gelu_bwd_against_the_exact_erf():
    """4096 points on [-12, 12], +-0, +-1e-30, a subnormal; n = 4100 and n = 4; n = 4102 refused"""
    _lib, L, on_stream, ptr, sptr = _api()
    z = BR.gelu_points()
    g = torch.Generator().manual_seed(9)
    du = torch.randn(z.numel(), generator=g)
    du[:8] = torch.tensor([1.0, -1.0, 3.0, -0.5, 1.0, 1.0, 1e-20, -1e20])
    u_ref, d_ref = BR.gelu64(z)
    res = []
    for _ in range(2):
        with on_stream() as s:
            zd, dud = z.cuda(), du.cuda()
            u, dz = _buf(z.numel() + 8).cuda(), _buf(z.numel() + 8).cuda()
            u4, dz4 = _buf(12).cuda(), _buf(12).cuda()
            _lib.check(L.wipa_gelu(ptr(zd), ptr(u), 4100, sptr(s)))
            _lib.check(L.wipa_gelu_bwd(ptr(zd), ptr(dud), ptr(dz), 4100, sptr(s)))
            _lib.check(L.wipa_gelu(ptr(zd) + 4 * 4100, ptr(u4), 4, sptr(s)))
            _lib.check(L.wipa_gelu_bwd(ptr(zd) + 4 * 4100, ptr(dud) + 4 * 4100, ptr(dz4), 4, sptr(s)))
            ur, dzr = _buf(4104 + 8).cuda(), _buf(4104 + 8).cuda()
            assert L.wipa_gelu(ptr(zd), ptr(ur), 4102, sptr(s)) != 0 and b"wipa_gelu" in L.wipa_last_error()
            assert L.wipa_gelu_bwd(ptr(zd), ptr(dud), ptr(dzr), 4102, sptr(s)) != 0 and b"wipa_gelu_bwd" in L.wipa_last_error()
        torch.cuda.synchronize()
        res.append([t.cpu() for t in (u, dz, u4, dz4, ur, dzr)])
    u, dz, u4, dz4, ur, dzr = res[0]
    assert all(bits_equal(a, b) for a, b in zip(res[0], res[1])), "two runs differ"
    assert bool((u[4100:] == SENTINEL).all()) and bool((dz[4100:] == SENTINEL).all()) and bool((u4[4:] == SENTINEL).all())
    assert bool((dz4[4:] == SENTINEL).all()) and bool((ur == SENTINEL).all()) and bool((dzr == SENTINEL).all())
    got_u, got_dz = torch.cat([u[:4100], u4[:4]]), torch.cat([dz[:4100], dz4[:4]])
    assert bool(torch.isfinite(got_u).all()) and bool(torch.isfinite(got_dz).all())
    zz = z.double().abs().clamp(min=1.0)
    e_u = (got_u.double() - u_ref).abs() / zz
    e_d = (got_dz.double() - du.double() * d_ref).abs() / du.double().abs()
    print(f"\ngelu: worst |err| / max(|z|, 1) = {float(e_u.max()):.2e} at z = {float(z[e_u.argmax()]):.3f};  "
          f"gelu': worst |err| / |du| = {float(e_d.max()):.2e} at z = {float(z[e_d.argmax()]):.3f}")
    assert float(e_u.max()) <= GELU_BOUND and float(e_d.max()) <= GELU_GRAD_BOUND
