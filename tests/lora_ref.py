"""float64 numpy statements of the low-rank adapter kernels (csrc/lora.hip) and the case table their GPU test walks.

    forward    u = x A^T ;  y = y0 + gain * u Bm^T
    backward   du = gain * dy Bm ;  dB = gain * dy^T u ;  dA = du^T x ;  dx (+)= du A
    merge      W = base + s * Bm A

The reference of an output is float64 from the same float32 inputs; the backward takes the float64 u ROUNDED to float32, as the
kernel takes the forward's.  ``floor32`` is the same statement in float32 numpy: the error a float32 evaluation has anyway, which
the bounds of tests/test_gpu_lora_kernels.py are multiples of.  No GPU, no torch."""
import functools
from typing import Dict, NamedTuple, Optional

import numpy as np

SENTINEL = -7.71484375e3  # exactly representable; no kernel output comes near it
QK_SCALE = 64 ** -0.25
MARGIN = 4.0  # kernels that differ from the float32 CPU statement only in summation order (LN_MARGIN of backward_ref.py)
OUTPUTS = ("u", "y", "dA", "dB", "dx")


class Case(NamedTuple):
    M: int
    K: int
    N: int
    r: int
    gain: float
    accumulate_dx: int
    ldx: Optional[int] = None   # None: K
    ldy: Optional[int] = None   # None: N.  Larger: y and dy are the first N columns of wider rows (a two-half buffer)
    dx_null: bool = False

    @property
    def id(self) -> str:
        return f"{self.M}x{self.K}x{self.N}-r{self.r}"


# the issue's table: a single row, ldx > K, one full tile, one row past a tile, the widest rank, and the cross-attention shape of three
# clips (many row chunks, ldy = 2N, no dx); both accumulate_dx values; gain 1, QK_SCALE and a negative one
CASES = (
    Case(1, 64, 64, 4, 1.0, 0),
    Case(17, 128, 192, 8, QK_SCALE, 1, ldx=136),
    Case(64, 128, 128, 16, -0.7, 0),
    Case(65, 512, 128, 16, 1.0, 1),
    Case(130, 128, 512, 64, QK_SCALE, 0),
    Case(4500, 128, 128, 8, -1.3, 0, ldy=256, dx_null=True),
)


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def err_rms(got, ref) -> float:
    """max|got - ref| / rms(ref); inf when got holds a NaN"""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max()
    return float("inf") if np.isnan(d) else float(d) / max(rms(ref), 1e-300)


def forward(x, A, Bm, y0, gain, dtype=np.float64):
    x, A, Bm, y0 = (np.asarray(t, dtype=dtype) for t in (x, A, Bm, y0))
    u = x @ A.T
    return u, y0 + dtype(gain) * (u @ Bm.T)


def backward(dy, x, u, A, Bm, gain, dx0=None, accumulate_dx=0, with_dx=True, dtype=np.float64):
    dy, x, u, A, Bm = (np.asarray(t, dtype=dtype) for t in (dy, x, u, A, Bm))
    du = dtype(gain) * (dy @ Bm)
    out = dict(du=du, dB=dtype(gain) * (dy.T @ u), dA=du.T @ x)
    if with_dx:
        out["dx"] = du @ A + (np.asarray(dx0, dtype=dtype) if accumulate_dx else 0)
    return out


def merge(base, A, Bm, s, dtype=np.float64):
    base, A, Bm = (np.asarray(t, dtype=dtype) for t in (base, A, Bm))
    return base + dtype(s) * (Bm @ A)


def merge_bound(base, A, Bm, s, r: int):
    """the forward error bound of the chain as specified (r fmaf steps from zero, one fmaf with the base, each rounding once):
    (r + 2) 2^-24 (|base| + |s| |Bm| |A|), elementwise"""
    base, A, Bm = (np.abs(np.asarray(t, dtype=np.float64)) for t in (base, A, Bm))
    return (r + 2) * 2.0 ** -24 * (base + abs(s) * (Bm @ A))


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Dict[str, np.ndarray]:
    """float32 inputs of a case: x, dy, y0 (the base output), dx0 (what dx holds before an accumulating call) ~ N(0, 1); A uniform in
    +-1/sqrt(K) as init_adapter draws it; Bm ~ 0.1 N(0, 1), never zero (a zero Bm makes du and dA vanish and shows nothing)"""
    g = np.random.default_rng(1000 * case.M + case.r)
    M, K, N, r = case.M, case.K, case.N, case.r
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    out = dict(x=f(M, K), dy=f(M, N), y0=f(M, N), dx0=f(M, K), A=g.uniform(-K ** -0.5, K ** -0.5, (r, K)).astype(np.float32),
               Bm=(0.1 * g.standard_normal((N, r))).astype(np.float32))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Dict[str, np.ndarray]:
    """float64 outputs of a case and ``u32``, the float32 rounding of u that the backward (kernel and reference alike) reads"""
    x = inputs(case)
    u, y = forward(x["x"], x["A"], x["Bm"], x["y0"], case.gain)
    u32 = u.astype(np.float32)
    b = backward(x["dy"], x["x"], u32, x["A"], x["Bm"], case.gain, x["dx0"], case.accumulate_dx, not case.dx_null)
    out = dict(u=u, y=y, u32=u32, **b)
    for v in out.values():
        v.setflags(write=False)
    return out


def floor32(case: Case) -> Dict[str, float]:
    """err_rms of the float32 numpy evaluation of every output of a case"""
    x, ref = inputs(case), reference(case)
    u, y = forward(x["x"], x["A"], x["Bm"], x["y0"], case.gain, np.float32)
    b = backward(x["dy"], x["x"], ref["u32"], x["A"], x["Bm"], case.gain, x["dx0"], case.accumulate_dx, not case.dx_null, np.float32)
    got = dict(u=u, y=y, **b)
    return {k: err_rms(got[k], ref[k]) for k in OUTPUTS if k in got}


MERGE_CASES = ((64, 64, 4, 2.0), (132, 68, 8, 0.5), (128, 512, 64, -0.25))  # (N, K, r, s)


@functools.lru_cache(maxsize=None)
def merge_inputs(N: int, K: int, r: int) -> Dict[str, np.ndarray]:
    g = np.random.default_rng(N + K + r)
    return dict(base=g.standard_normal((N, K)).astype(np.float32), A=g.uniform(-K ** -0.5, K ** -0.5, (r, K)).astype(np.float32),
                Bm=g.standard_normal((N, r)).astype(np.float32))
