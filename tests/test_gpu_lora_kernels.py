"""Kernel-level parity of the low-rank adapter kernels (csrc/lora.hip) against float64, through the C ABI.  ``pytest -m gpu``.

The common rules of tests/test_gpu_backward_kernels.py.  The reference is float64 from the same float32 inputs (tests/lora_ref.py).
The error of an output is max|t - ref| / rms(ref).  Every output buffer is larger than what the kernel may write: row gaps and tails
hold SENTINEL and must come back bit-identical; what the ABI documents as overwritten starts as NaN; the gaps of INPUT rows hold NaN,
so a read past a row's K or N columns poisons the result.  Every call runs twice into fresh buffers and must give the same bits.
Every bound is a named constant = a float32 CPU floor (measured by tests/test_lora_host.py on these very inputs, never by the kernel)
x lora_ref.MARGIN."""
import numpy as np
import pytest
import torch

import lora_ref as LR
from lora_ref import SENTINEL

pytestmark = pytest.mark.gpu

NAN = float("nan")

# Every figure of FLOOR is the float32 numpy figure of tests/test_lora_host.py, worst over lora_ref.CASES, rounded UP by about a tenth
# (the figure moves in its third digit with the BLAS of the machine that runs the host test, which asserts floor <= constant wherever it
# runs).  Worst floors: u 1.75e-6, y 4.03e-7, dA 1.52e-6, dB 1.78e-6, dx 1.58e-6.  Margin 4: products are exact on both sides, the
# kernels differ from the CPU in summation order alone.
# Measured on the MI355X (worst over the table): u 7.3e-7, y 2.8e-7, dA 1.2e-6, dB 1.0e-6, dx 1.4e-6.
FLOOR = {"u": 1.95e-6, "y": 4.5e-7, "dA": 1.7e-6, "dB": 2.0e-6, "dx": 1.75e-6}
BOUND = {k: LR.MARGIN * v for k, v in FLOOR.items()}


def _api():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    return _lib, _lib.lib(), on_stream, ptr, sptr


def _rows(a: np.ndarray, ld: int, gap: float, tail: int = 8, tail_fill: float = SENTINEL) -> torch.Tensor:
    """a [M, C] as the first C columns of rows of ld floats (the gap columns hold ``gap``), then ``tail`` floats of ``tail_fill``"""
    M, C = a.shape
    buf = torch.full((M * ld + tail,), gap, dtype=torch.float32)
    buf[: M * ld].view(M, ld)[:, :C] = torch.from_numpy(np.array(a, dtype=np.float32))
    buf[M * ld:] = tail_fill
    return buf


def _filled(n: int, fill: float, tail: int = 8) -> torch.Tensor:
    return torch.cat([torch.full((int(n),), fill, dtype=torch.float32), torch.full((tail,), SENTINEL, dtype=torch.float32)])


def _bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _run(case: LR.Case):
    """forward and backward of a case -> dict of CPU buffers as the kernels left them (plus the images of what they must not touch)"""
    _lib, L, on_stream, ptr, sptr = _api()
    x, ref = LR.inputs(case), LR.reference(case)
    M, K, N, r = case.M, case.K, case.N, case.r
    ldx, ldy = case.ldx or K, case.ldy or N
    lddx = K + 8 if case.ldx else K
    ws_bytes = L.wipa_lora_workspace_bytes(M, K, N, r)
    assert ws_bytes % 4 == 0 and ws_bytes >= 4 * M * r
    y_img = _rows(x["y0"], ldy, SENTINEL)
    dx_img = _rows(x["dx0"] if case.accumulate_dx else np.full((M, K), np.nan, np.float32), lddx, SENTINEL)
    with on_stream() as s:
        xd, Ad, Bd = _rows(x["x"], ldx, NAN).cuda(), torch.tensor(x["A"]).cuda(), torch.tensor(x["Bm"]).cuda()
        y, u = y_img.cuda(), _filled(M * r, NAN).cuda()
        rc_f = L.wipa_lora_fwd(ptr(xd), ldx, ptr(Ad), ptr(Bd), ptr(y), ldy, ptr(u), M, K, N, r, case.gain, sptr(s))
        dyd, u32 = _rows(x["dy"], ldy, NAN).cuda(), torch.tensor(ref["u32"]).cuda()
        dA, dB, dx = _filled(r * K, NAN).cuda(), _filled(N * r, NAN).cuda(), dx_img.cuda()
        ws = _filled(ws_bytes // 4, NAN).cuda()
        rc_b = L.wipa_lora_bwd(ptr(dyd), ldy, ptr(xd), ldx, ptr(u32), ptr(Ad), ptr(Bd), ptr(dA), ptr(dB), None if case.dx_null else ptr(dx),
                               lddx, case.accumulate_dx, M, K, N, r, case.gain, ptr(ws), ws_bytes, sptr(s))
    torch.cuda.synchronize()
    assert rc_f == 0 and rc_b == 0, L.wipa_last_error()
    return dict(y=y.cpu(), u=u.cpu(), dA=dA.cpu(), dB=dB.cpu(), dx=dx.cpu(), ws=ws.cpu(), y_img=y_img, dx_img=dx_img, ldy=ldy, lddx=lddx)


@pytest.mark.parametrize("case", LR.CASES, ids=lambda c: c.id)
def test_lora_forward_and_backward_float64_parity(case):
    M, K, N, r = case.M, case.K, case.N, case.r
    ref = LR.reference(case)
    a, b = _run(case), _run(case)
    for k in ("y", "u", "dA", "dB", "dx"):
        assert _bits(a[k], b[k]), f"{k}: two runs differ"
    ldy, lddx = a["ldy"], a["lddx"]
    got = dict(u=a["u"][: M * r].view(M, r), y=a["y"][: M * ldy].view(M, ldy)[:, :N], dA=a["dA"][: r * K].view(r, K),
               dB=a["dB"][: N * r].view(N, r))
    if not case.dx_null:
        got["dx"] = a["dx"][: M * lddx].view(M, lddx)[:, :K]
    errs = {k: LR.err_rms(v.numpy(), ref[k]) for k, v in got.items()}
    print(f"\n{case.id}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    # gaps and tails: bit-identical
    assert _bits(a["y"][: M * ldy].view(M, ldy)[:, N:], a["y_img"][: M * ldy].view(M, ldy)[:, N:]), "columns >= N of a y row were touched"
    for k, n in (("y", M * ldy), ("u", M * r), ("dA", r * K), ("dB", N * r), ("dx", M * lddx), ("ws", a["ws"].numel() - 8)):
        assert bool((a[k][n:] == SENTINEL).all()), f"{k}: written past its end"
    if case.dx_null:
        assert _bits(a["dx"], a["dx_img"]), "dx == NULL: the buffer was not passed and cannot have changed"
    else:
        assert _bits(a["dx"][: M * lddx].view(M, lddx)[:, K:], a["dx_img"][: M * lddx].view(M, lddx)[:, K:]), "the gap of a dx row was touched"
    for k, e in errs.items():
        assert e <= BOUND[k], (case.id, k, e, BOUND[k])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,K,r,s", LR.MERGE_CASES)
def test_lora_merge_within_the_chain_bound(N, K, r, s, dtype):
    """f32: |W - float64| <= (r + 2) 2^-24 (|base| + |s| |Bm| |A|) elementwise; bf16: the same plus one bf16 rounding of the
    result (8 significant bits: unit roundoff 2^-8).  W rows are wider than K: the gap holds SENTINEL and stays."""
    _lib, L, on_stream, ptr, sptr = _api()
    x = LR.merge_inputs(N, K, r)
    base = torch.tensor(x["base"]).to(dtype)
    ref = LR.merge(base.float().numpy(), x["A"], x["Bm"], s)
    bound = LR.merge_bound(base.float().numpy(), x["A"], x["Bm"], s, r)
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)
    ldw = K + 8
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    image = torch.full((N * ldw + 8,), SENTINEL, dtype=dtype)  # SENTINEL as the dtype rounds it
    image[: N * ldw].view(N, ldw)[:, :K] = NAN
    outs = []
    for _ in range(2):
        with on_stream() as st:
            W = image.cuda()
            bd, Ad, Bd = base.cuda(), torch.tensor(x["A"]).cuda(), torch.tensor(x["Bm"]).cuda()
            rc = L.wipa_lora_merge(ptr(W), ldw, _lib.WIPA_BF16 if dtype == torch.bfloat16 else _lib.WIPA_F32, ptr(bd), K, ptr(Ad), ptr(Bd),
                                   N, K, r, s, sptr(st))
        torch.cuda.synchronize()
        assert rc == 0, L.wipa_last_error()
        outs.append(W.cpu())
    W = outs[0]
    assert torch.equal(W.view(it), outs[1].view(it)), "two runs differ"
    got = W[: N * ldw].view(N, ldw)
    assert torch.equal(got[:, K:].contiguous().view(it), image[: N * ldw].view(N, ldw)[:, K:].contiguous().view(it)), "the gap of a W row was touched"
    assert torch.equal(W[N * ldw:].view(it), image[N * ldw:].view(it)), "written past the end of W"
    excess = np.abs(got[:, :K].float().numpy().astype(np.float64) - ref) / bound
    print(f"\nmerge {N}x{K} r{r} {dtype}: worst |W - ref| / bound = {np.nanmax(excess):.3f}")
    assert not np.isnan(excess).any() and float(excess.max()) <= 1.0
    if dtype == torch.float32:  # the adapter moved the weight: a merge that returned the base would sit far outside the bound
        assert float(np.abs(ref - x["base"]).max()) > 100 * float(bound.max())
