"""Kernel-level parity of wipa_lora_bank_apply (csrc/lora_bank.hip) against float64, through the C ABI.  ``pytest -m gpu``.

The reference is float64 from the same inputs (tests/lora_bank_ref.py), y and out addressed through the descriptor into a flat buffer
whose every other element holds SENTINEL and must come back bit-identical: columns beyond N, the rows of id -1 (act none), segments
without an adapter, the gaps of the cache layouts.  The gap columns of x rows hold NaN.  Every call runs twice and must give the same
bits.  Bounds: FLOOR is the float32 numpy floor of the same contraction (tests/test_lora_bank_host.py measures it on these very inputs
and asserts floor <= constant wherever it runs), x lora_bank_ref.MARGIN; a bf16 output adds 2^-8 |ref| for its one final rounding; the
GELU case adds the bound the project holds its device GELU series to (lora_bank_ref.bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lora_bank_ref as BR
from lora_bank_ref import SENTINEL

pytestmark = pytest.mark.gpu

# worst float32 numpy floor over lora_bank_ref.CASES (f32 and bf16 inputs), max|err| / rms(ref), rounded up by about a tenth:
# measured 4.79e-7 (8x512x128-r64, bf16 inputs).  Measured on the MI355X, max|err| / rms worst over the table: 6.1e-7 on f32 outputs.
FLOOR = 5.2e-7
MODES = ("f32", "bf16", "bf16_f32y")  # x / y dtypes: f32 / f32, bf16 / bf16, bf16 / f32 (a residual site's slab 0)


def _api():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    return _lib, _lib.lib(), on_stream, ptr, sptr


def _tdt(bf16: bool):
    return torch.bfloat16 if bf16 else torch.float32


def _images(case: BR.Case, mode: str):
    """-> (x image [M * ldx + 8] with NaN gaps, y image [buffer_len] with SENTINEL outside the addressed elements), CPU tensors"""
    xin = BR.inputs(case, mode != "f32")
    ldx = case.ldx or case.K
    x = torch.full((case.M * ldx + 8,), float("nan"), dtype=torch.float32)
    x[: case.M * ldx].view(case.M, ldx)[:, : case.K] = torch.from_numpy(np.array(xin["x"]))
    y = torch.full((BR.buffer_len(case),), SENTINEL, dtype=torch.float32)
    y[torch.from_numpy(BR.offsets(case).reshape(-1))] = torch.from_numpy(np.array(xin["y0"]).reshape(-1))
    return x.to(_tdt(mode != "f32")), y.to(_tdt(mode == "bf16"))


def _call(case: BR.Case, mode: str, ids=None, in_place: bool = True, ids_host=None, **over):
    """one wipa_lora_bank_apply -> (rc, out buffer on the CPU)"""
    _lib, L, on_stream, ptr, sptr = _api()
    xin = BR.inputs(case, mode != "f32")
    ids = case.ids if ids is None else ids
    x_img, y_img = _images(case, mode)
    with on_stream() as s:
        x, y = x_img.cuda(), y_img.cuda()
        out = y if in_place else torch.full_like(y, SENTINEL)
        A, B = torch.tensor(xin["A"]).cuda(), torch.tensor(xin["B"]).cuda()
        gain, idt = torch.tensor(xin["gain"]).cuda(), torch.tensor(ids, dtype=torch.int32).cuda()
        cod = torch.tensor([case.c_offset_dev], dtype=torch.int64).cuda() if case.c_offset_dev is not None else None
        d = _lib.LoraBankDesc(x=ptr(x), y=ptr(y), out=ptr(out), gain=ptr(gain), ids=ptr(idt), c_offset_dev=ptr(cod), ldx=case.ldx or case.K,
                              ld=case.ld or case.N, rg_stride=case.rg_stride, cg_stride=case.cg_stride, c_offset=case.c_offset, M=case.M,
                              K=case.K, N=case.N, r=case.r, n=case.n, rows_per_id=case.rows_per_id, n_seg=case.n_seg,
                              x_dtype=_lib.WIPA_F32 if mode == "f32" else _lib.WIPA_BF16,
                              y_dtype=_lib.WIPA_BF16 if mode == "bf16" else _lib.WIPA_F32, rg_in=case.rg_in, cg_in=case.cg_in, act=case.act)
        for sg in range(case.n_seg):
            d.col_scale[sg] = case.col_scale[sg]
            if case.seg_adapted[sg]:
                d.A[sg], d.B[sg] = ptr(A[sg]), ptr(B[sg])
        if ids_host is not None:
            d.ids_host = (C.c_int32 * len(ids_host))(*ids_host)
        for k, v in over.items():
            setattr(d, k, v)
        rc = L.wipa_lora_bank_apply(C.byref(d), sptr(s))
    torch.cuda.synchronize()
    return rc, out.cpu()


def _bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", BR.CASES + BR.EXTRA_CASES, ids=lambda c: c.id)
def test_bank_apply_float64_parity(case, mode):
    """Measured on the MI355X, worst |err| / bound over the table: f32 0.28, bf16 1.00 (0.996: a bf16 rounding of a value just above a
    power of two is 2^-8 of it), bf16 x with f32 y 0.29."""
    _lib, L, *_ = _api()
    bf16_in, bf16_out = mode != "f32", mode == "bf16"
    ref = BR.reference(case, bf16_in)
    rc, a = _call(case, mode, ids_host=case.ids)
    assert rc == 0, L.wipa_last_error()
    rc, b = _call(case, mode)
    assert rc == 0, L.wipa_last_error()
    assert _bits(a, b), "two calls differ"
    _, y_img = _images(case, mode)
    off = torch.from_numpy(BR.offsets(case))
    wr = BR.written(case)
    # what the call may not write: everything outside the addressed elements, and the addressed elements of rows on -1 and of segments
    # without an adapter when act is none
    keep = torch.ones(a.numel(), dtype=torch.bool)
    keep[off[torch.from_numpy(wr)]] = False
    assert _bits(a[keep], y_img[keep]), "bytes outside the adapted elements were touched"
    got = a[off.reshape(-1)].view(case.M, case.N).float().numpy().astype(np.float64)
    err, bound = np.abs(got - ref["out"]), BR.bound(case, FLOOR, bf16_out, bf16_in)
    print(f"\n{case.id} {mode}: worst |err| / bound = {float((err / bound).max()):.3f}  max|err| / rms = {float(err.max()) / BR.rms(ref['out']):.2e}")
    assert not np.isnan(err).any() and bool((err <= bound).all()), (case.id, mode, float((err / bound).max()))
    # the adapters moved the output: a call that returned y would sit far outside the bound
    if not case.act:
        moved = np.abs(ref["out"] - BR.inputs(case, bf16_in)["y0"])[wr]
        assert moved.size and float(moved.max()) > 50 * BR.MARGIN * FLOOR * BR.rms(ref["pre"])
    # out != y: the same bits land in a second buffer, and y keeps its own
    rc, o = _call(case, mode, in_place=False)
    assert rc == 0, L.wipa_last_error()
    assert _bits(o[~keep], a[~keep]) and _bits(o[keep], torch.full_like(o[keep], SENTINEL))


@pytest.mark.parametrize("mode", ("f32", "bf16"))
@pytest.mark.parametrize("case", [c for c in BR.CASES + BR.EXTRA_CASES if c.M > 1], ids=lambda c: c.id)
def test_a_rows_bits_do_not_depend_on_the_other_rows_ids(case, mode):
    """every row group keeps its id while all others move to other adapters, then to -1: its output bits stay"""
    _lib, L, *_ = _api()
    groups = len(case.ids)
    rc, full = _call(case, mode)
    assert rc == 0, L.wipa_last_error()
    off = torch.from_numpy(BR.offsets(case))
    for variant in range(2):
        for keep_grp in sorted({0, groups // 2, groups - 1}):
            ids = [((i + 1 + g) % case.n if variant == 0 else -1) for g, i in enumerate(case.ids)]
            ids[keep_grp] = case.ids[keep_grp]
            rc, other = _call(case, mode, ids=tuple(ids))
            assert rc == 0, L.wipa_last_error()
            rows = slice(keep_grp * case.rows_per_id, min(case.M, (keep_grp + 1) * case.rows_per_id))
            sel = off[rows].reshape(-1)
            assert _bits(full[sel], other[sel]), (case.id, variant, keep_grp)


def test_refusals_name_the_argument():
    _lib, L, *_ = _api()
    case = BR.CASES[1]
    for over, word in ((dict(r=6), "r = 6"), (dict(r=68), "r = 68"), (dict(n=65), "n = 65"), (dict(n=0), "n = 0"), (dict(K=126), "K = 126"),
                       (dict(ldx=126), "ldx = 126"), (dict(ld=198), "ld = 198"), (dict(cg_in=6), "cg_in = 6"), (dict(n_seg=4), "n_seg = 4"),
                       (dict(N=190), "N = 190"), (dict(rows_per_id=0), "rows_per_id = 0"), (dict(act=2), "act = 2"), (dict(x_dtype=2), "x_dtype = 2"),
                       (dict(c_offset=2), "c_offset = 2")):
        rc, out = _call(case, "f32", **over)
        msg = L.wipa_last_error().decode()
        assert rc == -1 and msg.startswith("wipa_lora_bank_apply: ") and word in msg, (over, msg)
    rc, out = _call(case, "f32", ids_host=(0, 2, -1, 3, 0))
    assert rc == -1 and "ids_host[3] = 3" in L.wipa_last_error().decode()
    rc, out = _call(case, "f32", y_dtype=_lib.WIPA_BF16)
    assert rc == -1 and "y_dtype = 1" in L.wipa_last_error().decode()
    rc, out = _call(case, "f32", x=0x1004)
    assert rc == -1 and "x: a 16-byte aligned" in L.wipa_last_error().decode()
