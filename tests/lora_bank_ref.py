"""float64 numpy statement of wipa_lora_bank_apply (csrc/lora_bank.hip), descriptor addressing included, and the case table its GPU
test walks.

    out[m, n] = act(y[m, n] + c[s] * gain[id] * sum_j (sum_k x[m, k] A[s][id][j, k]) B[s][id][n', j]),   id = ids[m // rows_per_id]

with s = n // (N / n_seg) the column segment, n' = n % (N / n_seg); id = -1 (or a segment without an adapter) leaves the sum out.
Element (m, n) of y and out lives at
    c_offset + c_offset_dev + (m // rg_in) * rg_stride + (m % rg_in) * ld + (n // cg_in) * cg_stride + n % cg_in
in a flat buffer.  The reference of an output is float64 from the same inputs (x and y as the call's dtype holds them); ``floor32`` is
the same statement in float32 numpy.  No GPU, no torch."""
import functools
import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

SENTINEL = -7.71484375e3  # lora_ref.SENTINEL (a bf16 buffer holds its bf16 rounding); no output comes near it
QK_SCALE = 64 ** -0.25
MARGIN = 4.0  # lora_ref.MARGIN: the kernel differs from the float32 CPU statement in summation order alone
# the bound tests/test_gpu_backward_kernels.py holds the device's Abramowitz-Stegun 7.1.26 GELU to, in units of max(|z|, 1): the series
# error (1.5e-7 on erf) plus the GPU's approximate rcp and exp2.  The adapter epilogue calls the same device function.
GELU_BOUND = 7e-7
BF16_EPS = 2.0 ** -8  # the single final rounding of a bf16 output, as a multiple of |ref|


class Case(NamedTuple):
    M: int
    K: int
    N: int
    r: int
    n: int
    rows_per_id: int
    ids: Tuple[int, ...]
    n_seg: int = 1
    seg_adapted: Tuple[bool, ...] = (True,)
    col_scale: Tuple[float, ...] = (1.0,)
    act: int = 0
    ld: Optional[int] = None  # None: N
    rg_in: int = 0
    rg_stride: int = 0
    cg_in: int = 0
    cg_stride: int = 0
    c_offset: int = 0
    c_offset_dev: Optional[int] = None
    ldx: Optional[int] = None

    @property
    def id(self) -> str:
        return f"{self.M}x{self.K}x{self.N}-r{self.r}-n{self.n}-p{self.rows_per_id}"


def _ids(seed: int, rows: int, n: int) -> Tuple[int, ...]:
    g = np.random.default_rng(seed)
    return tuple(int(v) for v in g.integers(-1, n, rows))


# the issue's table.  2: q|k|v of 64 columns each, the key segment without an adapter, one row on -1, rows wider than N.
# 3: the self K / V cache [3][64 rows][8 positions][128] at position 3: one row group per row, one column group per segment, the
# position's offset on the device.  4: the four-row prompt pass of two clips.  5: key | value of three clips of 37 frames written as
# [clip][2][H = 1][37][64]; the middle clip has no adapter.  6: mlp1 with the GELU; row ids include -1.
CASES = (
    Case(1, 64, 64, 4, 1, 1, (0,)),
    Case(5, 128, 192, 8, 3, 1, (0, 2, -1, 1, 0), n_seg=3, seg_adapted=(True, False, True), col_scale=(QK_SCALE, QK_SCALE, 1.0), ld=200, ldx=136),
    Case(64, 128, 384, 16, 7, 1, _ids(3, 64, 7), n_seg=3, seg_adapted=(True, True, True), col_scale=(QK_SCALE, QK_SCALE, 1.0), ld=128,
         rg_in=1, rg_stride=8 * 128, cg_in=128, cg_stride=64 * 8 * 128, c_offset_dev=3 * 128),
    Case(8, 512, 128, 64, 2, 4, (1, 0)),
    Case(3 * 37, 128, 128, 16, 3, 37, (2, -1, 0), n_seg=2, seg_adapted=(True, True), col_scale=(QK_SCALE, 1.0), ld=64, rg_in=37,
         rg_stride=2 * 37 * 64, cg_in=64, cg_stride=37 * 64, c_offset=8),
    Case(17, 128, 512, 8, 3, 1, _ids(6, 17, 3)[:-1] + (-1,), act=1),
)
# beyond the issue's table: more than 1024 rows with fewer than 16 rows per id, which the tile kernel serves with partly filled tiles
# (one row per id, and the four-row prompt pass of 260 clips)
EXTRA_CASES = (
    Case(1040, 64, 64, 4, 2, 1, _ids(9, 1040, 2)),
    Case(1040, 64, 128, 8, 3, 4, _ids(10, 260, 3), n_seg=2, seg_adapted=(True, True), col_scale=(QK_SCALE, 1.0)),
)
GAINS = (2.0, 0.5, 1.25, 4.0, 1.0, 0.75, 3.0)  # alpha / r of the bank's adapters, a different one each


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def offsets(case: Case) -> np.ndarray:
    """int64 [M, N]: where element (m, n) lives in the flat y / out buffer"""
    rg_in, cg_in, ld = case.rg_in or case.M, case.cg_in or case.N, case.ld or case.N
    m, n = np.arange(case.M, dtype=np.int64)[:, None], np.arange(case.N, dtype=np.int64)[None, :]
    return case.c_offset + (case.c_offset_dev or 0) + (m // rg_in) * case.rg_stride + (m % rg_in) * ld + (n // cg_in) * case.cg_stride + n % cg_in


def buffer_len(case: Case) -> int:
    return int(offsets(case).max()) + 1 + 24


def gelu64(v: np.ndarray) -> np.ndarray:
    return np.asarray(v, dtype=np.float64) * 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(v, dtype=np.float64) / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def inputs(case: Case, bf16: bool = False) -> Dict[str, np.ndarray]:
    """x, y0 ~ N(0, 1) (rounded to bf16 when the call holds them so); per segment A uniform in +-1/sqrt(K) as init_adapter draws it and
    B ~ 0.1 N(0, 1), never zero; gain"""
    g = np.random.default_rng(7000 * case.M + 10 * case.r + case.n)
    M, K, N, r, n = case.M, case.K, case.N, case.r, case.n
    sn = N // case.n_seg
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    x, y0 = f(M, K), f(M, N)
    if bf16:
        x, y0 = bf16_round(x), bf16_round(y0)
    out = dict(x=x, y0=y0, A=g.uniform(-K ** -0.5, K ** -0.5, (case.n_seg, n, r, K)).astype(np.float32),
               B=(0.1 * g.standard_normal((case.n_seg, n, sn, r))).astype(np.float32), gain=np.asarray(GAINS[:n], dtype=np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


def apply(case: Case, x, y0, A, B, gain, ids=None, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """-> (the pre-activation y0 + term, the output), dense [M, N] in ``dtype`` (the GELU itself is always taken in float64)"""
    ids = case.ids if ids is None else ids
    x, y0, A, B, gain = (np.asarray(t, dtype=dtype) for t in (x, y0, A, B, gain))
    sn = case.N // case.n_seg
    pre = np.array(y0, dtype=dtype)
    for m in range(case.M):
        i = ids[m // case.rows_per_id]
        if i < 0:
            continue
        for s in range(case.n_seg):
            if case.seg_adapted[s]:
                u = A[s, i] @ x[m]
                pre[m, s * sn:(s + 1) * sn] += dtype(case.col_scale[s]) * gain[i] * (B[s, i] @ u)
    return pre, (gelu64(pre).astype(dtype) if case.act else pre)


def written(case: Case, ids=None) -> np.ndarray:
    """bool [M, N]: the elements the call may write -- with act every one, else those of adapted segments in rows with an adapter"""
    ids = case.ids if ids is None else ids
    if case.act:
        return np.ones((case.M, case.N), dtype=bool)
    sn = case.N // case.n_seg
    rows = np.asarray([ids[m // case.rows_per_id] >= 0 for m in range(case.M)])[:, None]
    cols = np.repeat(np.asarray(case.seg_adapted), sn)[None, :]
    return rows & cols


@functools.lru_cache(maxsize=None)
def reference(case: Case, bf16: bool = False) -> Dict[str, np.ndarray]:
    x = inputs(case, bf16)
    pre, out = apply(case, x["x"], x["y0"], x["A"], x["B"], x["gain"])
    return dict(pre=pre, out=out)


def floor32(case: Case, bf16: bool = False) -> float:
    """max|float32 numpy - float64| / rms(float64) of the pre-activation: the contraction's own float32 error"""
    x, ref = inputs(case, bf16), reference(case, bf16)
    pre32, _ = apply(case, x["x"], x["y0"], x["A"], x["B"], x["gain"], dtype=np.float32)
    return float(np.abs(pre32.astype(np.float64) - ref["pre"]).max()) / rms(ref["pre"])


def bound(case: Case, floor: float, bf16_out: bool, bf16: bool = False) -> np.ndarray:
    """elementwise bound on |out - reference| [M, N]: MARGIN x floor x rms of the pre-activation (the GELU's slope is below 1.13, so with
    act the same figure x 1.13, plus GELU_BOUND max(|z|, 1) for the series), plus BF16_EPS |ref| for a bf16 output's one rounding"""
    ref = reference(case, bf16)
    b = np.full((case.M, case.N), MARGIN * floor * rms(ref["pre"]))
    if case.act:
        b = 1.13 * b + GELU_BOUND * np.maximum(np.abs(ref["pre"]), 1.0)
    if bf16_out:
        b = b + BF16_EPS * np.abs(ref["out"])
    return b
