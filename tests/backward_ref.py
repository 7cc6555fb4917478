"""float64 references of the backward kernels (csrc/attention_bwd.hip, csrc/train.hip), their float32 restatements, the case
tables of tests/test_gpu_backward_kernels.py and the GPU checker of the attention backward (shared with the child process that
runs the VALU pair).  Plain torch / numpy; nothing here touches the GPU at import.

  *_ref64            the operation in float64 from the float32 input values.  What the kernels are held to.
  *_floor32          the same formula evaluated in float32 on the CPU (torch's own float32 kernels where the issue names them).
                     Its error against float64, on the very inputs of a test, is the FLOOR a bound is derived from:
                     bound = worst floor over the case table x the margin of the section.  tests/test_backward_ref_host.py
                     measures every floor and asserts it under bound / margin; the kernels' own figures never enter a bound.
  err_rms            max|t - ref| / rms(ref), the error measure of every float comparison here.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

SENTINEL = -7.71484375e3  # exactly representable; no kernel output comes near it


def rms(t: torch.Tensor) -> float:
    return float(t.double().pow(2).mean().sqrt())


def err_rms(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got - ref| / rms(ref); inf when got holds a NaN"""
    d = (got.double() - ref.double()).abs().max()
    return float("inf") if torch.isnan(d) else float(d) / max(rms(ref), 1e-300)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit-for-bit equality (NaN payloads and signed zeros included)"""
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ====================================================================== 1. attention backward
HD = 64
ATTN_B, ATTN_H = 2, 3
HEAD_SCALES = (0.3, 0.6, 1.0)  # q, k of head h: softmax rows from nearly flat to nearly one-hot
ATTN_MARGIN = 8.0
QK_SCALES = (1.0, 64 ** -0.25, 0.37)


class AttnCase(NamedTuple):
    causal: bool
    Tq: int
    Tk: int
    layout: str
    qk_scale: float


def _attn_table() -> List[AttnCase]:
    shapes = [(True, 21, 21), (True, 64, 64), (True, 65, 65), (True, 130, 130), (True, 100, 164), (True, 33, 70),
              (False, 13, 150), (False, 64, 128), (False, 70, 200), (False, 16, 220), (False, 129, 65)]
    # layouts alternate through the table: (a) meets causal and non-causal cases, and so does (b); the scales cycle with period 3
    return [AttnCase(c, tq, tk, "ab"[i % 2], QK_SCALES[i % 3]) for i, (c, tq, tk) in enumerate(shapes)]


ATTN_CASES = _attn_table()
ATTN_CHAIN_CASES = [c for c in ATTN_CASES if (c.Tq, c.Tk) in ((100, 164), (13, 150), (70, 200))]


def attn_inputs(case: AttnCase) -> Dict[str, torch.Tensor]:
    """float32 q, k [B, T, H, 64] (head h scaled by HEAD_SCALES[h]), v, d_out"""
    g = torch.Generator().manual_seed(1000 * case.Tq + case.Tk + int(case.causal))
    B, H = ATTN_B, ATTN_H
    sc = torch.tensor(HEAD_SCALES).view(1, 1, H, 1)
    return {"q": torch.randn(B, case.Tq, H, HD, generator=g) * sc, "k": torch.randn(B, case.Tk, H, HD, generator=g) * sc,
            "v": torch.randn(B, case.Tk, H, HD, generator=g), "d_out": torch.randn(B, case.Tq, H, HD, generator=g)}


def _visible(Tq: int, Tk: int, causal: bool) -> torch.Tensor:
    """[Tq, Tk] bool: query i sees key j <= i + (Tk - Tq)"""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    return torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + (Tk - Tq)


def attn_forward(q, k, v, causal: bool, dtype=torch.float64):
    """-> out [B, Tq, H, 64], lse [B, H, Tq] in ``dtype``; q and k are the pre-scaled values, S = q . k"""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    s = s.masked_fill(~_visible(q.shape[1], k.shape[1], causal), float("-inf"))
    lse = torch.logsumexp(s, -1)
    return torch.einsum("bhqk,bkhd->bqhd", torch.exp(s - lse[..., None]), v), lse


def attn_backward(q, k, v, out, lse, d_out, causal: bool, qk_scale: float, dtype=torch.float64):
    """The documented formulation (csrc/attention_bwd.hip header) in ``dtype``:
    P = exp(S - lse), D = dO . O, dS = P (dP - D), dq = scale dS K, dk = scale dS^T Q, dv = P^T dO.
    -> dq, dk, dv [B, T, H, 64], D [B, H, Tq]"""
    q, k, v, out, lse, d_out = (t.to(dtype) for t in (q, k, v, out, lse, d_out))
    s = torch.einsum("bqhd,bkhd->bhqk", q, k)
    p = torch.exp(s - lse[..., None]).masked_fill(~_visible(q.shape[1], k.shape[1], causal), 0.0)
    dvec = (d_out * out).sum(-1).permute(0, 2, 1)
    ds = p * (torch.einsum("bqhd,bkhd->bhqk", d_out, v) - dvec[..., None])
    sc = torch.tensor(qk_scale, dtype=dtype)
    return (torch.einsum("bhqk,bkhd->bqhd", ds, k) * sc, torch.einsum("bhqk,bqhd->bkhd", ds, q) * sc,
            torch.einsum("bhqk,bqhd->bkhd", p, d_out), dvec)


@functools.lru_cache(maxsize=None)
def attn_reference(case: AttnCase):
    """-> (inputs, out32, lse32, ref) : the float64 forward rounded to float32 (what the kernel is given) and the float64
    gradients {dq, dk, dv, dvec} from the UNROUNDED forward.  Computed once per case and shared; do not modify."""
    x = attn_inputs(case)
    out, lse = attn_forward(x["q"], x["k"], x["v"], case.causal)
    dq, dk, dv, dvec = attn_backward(x["q"], x["k"], x["v"], out, lse, x["d_out"], case.causal, case.qk_scale)
    return x, out.float(), lse.float(), {"dq": dq, "dk": dk, "dv": dv, "dvec": dvec, "out": out, "lse": lse}


def attn_slice_errors(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """worst err_rms over the (batch, head) slices of each of dq / dk / dv [B, T, H, 64] and dvec / lse [B, H, Tq]"""
    res = {}
    for name, t in got.items():
        worst = 0.0
        for b in range(ATTN_B):
            for h in range(ATTN_H):
                sl = (b, h) if name in ("dvec", "lse") else (b, slice(None), h)
                worst = max(worst, err_rms(t[sl], ref[name][sl]))
        res[name] = worst
    return res


def attn_floor32(case: AttnCase) -> Dict[str, float]:
    """error of the float32 restatement (rounded out / lse in, everything in float32 on the CPU) against float64"""
    x, out32, lse32, ref = attn_reference(case)
    dq, dk, dv, dvec = attn_backward(x["q"], x["k"], x["v"], out32, lse32, x["d_out"], case.causal, case.qk_scale, torch.float32)
    return attn_slice_errors({"dq": dq, "dk": dk, "dv": dv, "dvec": dvec}, ref)


def attn_forward_floor32(case: AttnCase) -> Dict[str, float]:
    x, _, _, ref = attn_reference(case)
    out, lse = attn_forward(x["q"], x["k"], x["v"], case.causal, torch.float32)
    return attn_slice_errors({"out": out, "lse": lse}, ref)


class Strided:
    """a [B, T, H, 64] tensor inside a flat float32 buffer: element (b, t, h, d) at off + b*bs + t*rs + h*64 + d"""

    def __init__(self, n_floats: int, off: int, bs: int, rs: int, T: int):
        self.n, self.off, self.bs, self.rs, self.T = n_floats, off, bs, rs, T
        b, t, h, d = torch.meshgrid(torch.arange(ATTN_B), torch.arange(T), torch.arange(ATTN_H), torch.arange(HD), indexing="ij")
        self.idx = off + b * bs + t * rs + h * HD + d
        assert int(self.idx.max()) < n_floats

    def put(self, flat: torch.Tensor, vals: torch.Tensor) -> None:
        flat[self.idx.reshape(-1)] = vals.reshape(-1).to(flat.dtype)

    def get(self, flat: torch.Tensor) -> torch.Tensor:
        return flat[self.idx.reshape(-1)].view(self.idx.shape)


def attn_layout(case: AttnCase) -> Dict[str, Strided]:
    """(a) q rows of stride 3*H*64 + 8; k | v the two halves of ONE buffer of row stride 2*H*64 (the trainer's cross layout);
    out / d_out rows of H*64 + 16; every batch stride T * row stride + 32.  (b) four buffers, q_rs = H*64, k_rs = H*64 + 4,
    v_rs = H*64 + 12, o_rs = H*64 + 8, batch stride T * row stride: all four batch strides differ as well.
    Every buffer has a 16-float tail.  The entries "k" and "v" of (a) name the same buffer size and differ in ``off``."""
    W, B, Tq, Tk = ATTN_H * HD, ATTN_B, case.Tq, case.Tk
    if case.layout == "a":
        q_rs, kv_rs, o_rs = 3 * W + 8, 2 * W, W + 16
        q_bs, kv_bs, o_bs = Tq * q_rs + 32, Tk * kv_rs + 32, Tq * o_rs + 32
        return {"q": Strided(B * q_bs + 16, 0, q_bs, q_rs, Tq), "k": Strided(B * kv_bs + 16, 0, kv_bs, kv_rs, Tk),
                "v": Strided(B * kv_bs + 16, W, kv_bs, kv_rs, Tk), "o": Strided(B * o_bs + 16, 0, o_bs, o_rs, Tq)}
    q_rs, k_rs, v_rs, o_rs = W, W + 4, W + 12, W + 8
    return {"q": Strided(B * Tq * q_rs + 16, 0, Tq * q_rs, q_rs, Tq), "k": Strided(B * Tk * k_rs + 16, 0, Tk * k_rs, k_rs, Tk),
            "v": Strided(B * Tk * v_rs + 16, 0, Tk * v_rs, v_rs, Tk), "o": Strided(B * Tq * o_rs + 16, 0, Tq * o_rs, o_rs, Tq)}


def _flat(n: int, fill: float) -> torch.Tensor:
    return torch.full((n,), fill, dtype=torch.float32)


def attn_buffers(case: AttnCase, lay: Dict[str, Strided], x, out32, d_out):
    """CPU images of the input buffers (gaps NaN: a read outside the layout poisons the result) and of the gradient buffers
    (NaN where the ABI says "overwritten", SENTINEL in every row gap, padding column and tail)"""
    nan = float("nan")
    shared_kv = case.layout == "a"
    ins = {"q": _flat(lay["q"].n, nan), "k": _flat(lay["k"].n, nan), "o": _flat(lay["o"].n, nan), "g": _flat(lay["o"].n, nan)}
    ins["v"] = ins["k"] if shared_kv else _flat(lay["v"].n, nan)
    lay["q"].put(ins["q"], x["q"]); lay["k"].put(ins["k"], x["k"]); lay["v"].put(ins["v"], x["v"])
    lay["o"].put(ins["o"], out32); lay["o"].put(ins["g"], d_out)
    outs = {"dq": _flat(lay["q"].n, SENTINEL), "dk": _flat(lay["k"].n, SENTINEL)}
    outs["dv"] = outs["dk"] if shared_kv else _flat(lay["v"].n, SENTINEL)
    for name, key in (("dq", "q"), ("dk", "k"), ("dv", "v")):
        lay[key].put(outs[name], torch.full(lay[key].idx.shape, nan))
    return ins, outs


def attn_desc(case: AttnCase, lay: Dict[str, Strided], dev: Dict[str, torch.Tensor], lse_dev=None, out_dev=None):
    from whisper_ipa_amd import _lib

    a = _lib.AttnDesc()
    a.q = dev["q"].data_ptr() + 4 * lay["q"].off
    a.k = dev["k"].data_ptr() + 4 * lay["k"].off
    a.v = dev["v"].data_ptr() + 4 * lay["v"].off
    a.out = out_dev.data_ptr() if out_dev is not None else dev["o"].data_ptr()
    a.lse = lse_dev.data_ptr() if lse_dev is not None else None
    a.q_bs, a.q_rs, a.q_hs = lay["q"].bs, lay["q"].rs, HD
    a.k_bs, a.k_rs, a.k_hs = lay["k"].bs, lay["k"].rs, HD
    a.v_bs, a.v_rs, a.v_hs = lay["v"].bs, lay["v"].rs, HD
    a.o_bs, a.o_rs, a.o_hs = lay["o"].bs, lay["o"].rs, HD
    a.B, a.H, a.Tq, a.Tk, a.causal, a.dtype = ATTN_B, ATTN_H, case.Tq, case.Tk, int(case.causal), 0
    return a


def run_attention_bwd(case: AttnCase, chain: bool = False, q_bs_delta: int = 0):
    """One call of wipa_attention_bwd on the strided, poisoned buffers of ``case`` (GPU).  chain: out / lse come from
    wipa_attention instead of the rounded float64 forward.  q_bs_delta: added to the descriptor's q_bs (refusal test).
    -> (rc, got {dq, dk, dv, dvec [, out, lse]} on the CPU, raw output buffers, expected untouched images, layout)"""
    import ctypes as C

    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    x, out32, lse32, _ = attn_reference(case)
    lay = attn_layout(case)
    ins, outs = attn_buffers(case, lay, x, out32, x["d_out"])
    n_vec = ATTN_B * ATTN_H * case.Tq
    dvec0 = torch.cat([_flat(n_vec, float("nan")), _flat(8, SENTINEL)])
    with on_stream() as s:
        dev = {k: v.cuda() for k, v in ins.items()}
        if case.layout == "a":
            dev["v"] = dev["k"]
        dout = {k: v.cuda() for k, v in outs.items()}
        if case.layout == "a":
            dout["dv"] = dout["dk"]
        dvec = dvec0.cuda()
        lse_d = lse32.contiguous().cuda()
        out_d = dev["o"]
        if chain:
            lse_d = torch.cat([_flat(n_vec, float("nan")), _flat(8, SENTINEL)]).cuda()
            fw = _flat(lay["o"].n, SENTINEL)
            lay["o"].put(fw, torch.full(lay["o"].idx.shape, float("nan")))
            out_d = fw.cuda()
            a = attn_desc(case, lay, dev, lse_d, out_d)
            _lib.check(L.wipa_attention(C.byref(a), sptr(s)), "wipa_attention")
        a = attn_desc(case, lay, dev, None, out_d)
        a.q_bs += q_bs_delta
        rc = L.wipa_attention_bwd(C.byref(a), ptr(out_d), ptr(dev["g"]), ptr(lse_d), ptr(dout["dq"]) + 4 * lay["q"].off,
                                  ptr(dout["dk"]) + 4 * lay["k"].off, ptr(dout["dv"]) + 4 * lay["v"].off, ptr(dvec),
                                  case.qk_scale, sptr(s))
    torch.cuda.synchronize()
    raw = {k: v.cpu() for k, v in dout.items()}
    raw["dvec"] = dvec.cpu()
    got = {"dq": lay["q"].get(raw["dq"]), "dk": lay["k"].get(raw["dk"]), "dv": lay["v"].get(raw["dv"]),
           "dvec": raw["dvec"][:n_vec].view(ATTN_B, ATTN_H, case.Tq)}
    if chain:
        raw["out"], raw["lse"] = out_d.cpu(), lse_d.cpu()
        got["out"] = lay["o"].get(raw["out"])
        got["lse"] = raw["lse"][:n_vec].view(ATTN_B, ATTN_H, case.Tq)
    untouched = dict(outs, dvec=dvec0)
    return rc, got, raw, untouched, lay


def gaps_untouched(raw: torch.Tensor, image: torch.Tensor) -> bool:
    """every SENTINEL of the pre-filled image is still there, bit for bit"""
    keep = image == SENTINEL
    return bits_equal(raw[keep], image[keep])


def check_attention_bwd(case: AttnCase, bounds: Dict[str, float], chain: bool = False) -> Dict[str, float]:
    """the whole check of one case: two runs into fresh buffers bit-equal, gaps untouched, no NaN left, per-slice errors under
    ``bounds`` (keys dq, dk, dv, dvec [, out, lse]).  Prints and returns the errors."""
    rc, got, raw, untouched, lay = run_attention_bwd(case, chain)
    assert rc == 0, rc
    rc2, _, raw2, _, _ = run_attention_bwd(case, chain)
    assert rc2 == 0
    for name in raw:
        assert bits_equal(raw[name], raw2[name]), (case, name, "two runs differ")
    for name in untouched:
        assert gaps_untouched(raw[name], untouched[name]), (case, name, "written outside its layout")
    if chain:
        fw = lay["o"]
        keep = torch.ones(fw.n, dtype=torch.bool)
        keep[fw.idx.reshape(-1)] = False
        assert bool((raw["out"][keep] == SENTINEL).all()) and bool((raw["lse"][-8:] == SENTINEL).all()), (case, "forward gaps")
    x, _, _, ref = attn_reference(case)
    if chain:  # D = dO . O of the out the backward was GIVEN, here the forward kernel's
        ref = dict(ref, dvec=(x["d_out"].double() * got["out"].double()).sum(-1).permute(0, 2, 1))
    errs = attn_slice_errors(got, ref)
    print(f"\nattention bwd {'chain ' if chain else ''}{tuple(case)}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < bounds[name], (case, name, e, bounds[name])
    return errs


def check_attention_table(bounds: Dict[str, float]) -> Dict[str, float]:
    """every case of ATTN_CASES under the same bounds (what the child process of the VALU pair runs)"""
    worst: Dict[str, float] = {}
    for case in ATTN_CASES:
        for k, v in check_attention_bwd(case, bounds).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ====================================================================== 2. LayerNorm backward
LN_CASES = [(1, 64), (3, 128), (5, 384), (63, 768), (64, 768), (65, 1028), (130, 1280), (2100, 256), (7, 2048)]
LN_FAMILIES = [(1.0, 0.0), (2.0, 0.5), (0.05, 30.0)]  # x = randn * s + m; the last is offset-dominated (bound of its own)
LN_MARGIN = 4.0
LN_EPS = 1e-5
LN_OUTPUTS = ("dx", "dx_acc", "dw", "db", "mean", "rstd")


@functools.lru_cache(maxsize=None)
def ln_inputs(rows: int, D: int, fam: int, integer_dy: bool = False) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(rows * 4099 + D * 3 + fam)
    s, m = LN_FAMILIES[fam]
    x = torch.randn(rows, D, generator=g) * s + m
    dy = torch.randint(-3, 4, (rows, D), generator=g).float() if integer_dy else torch.randn(rows, D, generator=g)
    return {"x": x, "w": torch.randn(D, generator=g), "dy": dy, "base": torch.randn(rows, D, generator=g)}


def ln_backward(x, w, dy, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum_r dy xhat; db = sum_r dy; stats = (mean, rstd)"""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return {"dx": dx, "dw": (dy * xh).sum(0), "db": dy.sum(0), "mean": mean[:, 0], "rstd": rstd[:, 0]}


@functools.lru_cache(maxsize=None)
def ln_reference(rows: int, D: int, fam: int, integer_dy: bool = False) -> Dict[str, torch.Tensor]:
    """float64 reference of one (case, family), shared; dx_acc = base + dx.  Do not modify."""
    x = ln_inputs(rows, D, fam, integer_dy)
    r = ln_backward(x["x"], x["w"], x["dy"])
    r["dx_acc"] = x["base"].double() + r["dx"]
    return r


def ln_floor32(rows: int, D: int, fam: int) -> Dict[str, float]:
    """torch's float32 layer_norm backward on the CPU (and float32 mean / rstd) against float64, per tensor.  On ONE thread:
    torch cuts the row sums of dw / db by its thread count (2100 rows: 4.6e-6 on one thread, 7e-7 on sixteen), and a floor must
    not depend on the machine; one thread is the plain sequential sum."""
    x = ln_inputs(rows, D, fam)
    ref = ln_reference(rows, D, fam)
    xl, wl = x["x"].clone().requires_grad_(True), x["w"].clone().requires_grad_(True)
    bl = torch.zeros(D, requires_grad=True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.nn.functional.layer_norm(xl, (D,), wl, bl, LN_EPS).backward(x["dy"])
    finally:
        torch.set_num_threads(threads)
    mean = x["x"].mean(-1)
    rstd = torch.rsqrt(x["x"].var(-1, unbiased=False) + LN_EPS)
    got = {"dx": xl.grad, "dx_acc": x["base"] + xl.grad, "dw": wl.grad, "db": bl.grad, "mean": mean, "rstd": rstd}
    return {k: err_rms(got[k], ref[k]) for k in LN_OUTPUTS}


# ====================================================================== 3. masked CE backward
CE_B, CE_T = 3, 5
CE_VS = (1, 37, 512, 513, 5000)
CE_COUNTS = (0.0, 1.0, 7.0, 40.0)
CE_MARGIN = 8.0
CE_MASK = (0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0)  # arbitrary, first and last row masked out
CE_ROW_TARGET_SPIKE, CE_ROW_OTHER_SPIKE, CE_ROW_CONSTANT = 2, 5, 8  # all three are unmasked rows


@functools.lru_cache(maxsize=None)
def ce_inputs(V: int):
    """-> logits [15, V] f32, targets [15] (columns 0 and V-1 among them)"""
    g = torch.Generator().manual_seed(77 + V)
    rows = CE_B * CE_T
    logits = torch.randn(rows, V, generator=g) * 2
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[1], tgt[4] = 0, V - 1
    logits[CE_ROW_TARGET_SPIKE] = torch.randn(V, generator=g)
    logits[CE_ROW_TARGET_SPIKE, tgt[CE_ROW_TARGET_SPIKE]] += 60.0  # the softmax saturates, p - 1 cancels
    logits[CE_ROW_OTHER_SPIKE] = torch.randn(V, generator=g)
    logits[CE_ROW_OTHER_SPIKE, (tgt[CE_ROW_OTHER_SPIKE] + 1) % V] += 60.0  # (V = 1: the only column is the target)
    logits[CE_ROW_CONSTANT] = 1.75
    return logits, tgt


def ce_backward(logits, tgt, mask, count: float, dtype=torch.float64) -> torch.Tensor:
    """mask_r (softmax_r - onehot(tgt_r)) / max(count, 1)"""
    p = torch.softmax(logits.to(dtype), -1)
    p = p - torch.nn.functional.one_hot(tgt, logits.shape[1]).to(dtype)
    return p * mask.to(dtype)[:, None] / max(count, 1.0)


def ce_floor32(V: int) -> float:
    """float32 torch softmax on the CPU, in units of probability (the 1 / max(count, 1) factor taken out)"""
    logits, tgt = ce_inputs(V)
    mask = torch.tensor(CE_MASK, dtype=torch.float32)
    d = ce_backward(logits, tgt, mask, 1.0, torch.float32).double() - ce_backward(logits, tgt, mask, 1.0)
    return float(d.abs().max())


CE_CHAIN_V, CE_CHAIN_EOT = 513, 7


def ce_chain_inputs():
    """tokens [3, 6]: a row with no EOT, a row whose FIRST target is EOT, a row with EOT from the middle on; logits [15, 513]"""
    e = CE_CHAIN_EOT
    tokens = torch.tensor([[3, 100, 512, 0, 9, 250], [3, e, e, e, e, e], [3, 41, 300, e, e, e]], dtype=torch.int64)
    g = torch.Generator().manual_seed(5)
    return torch.randn(CE_B * CE_T, CE_CHAIN_V, generator=g) * 2, tokens


def ce_chain_reference(dtype=torch.float64):
    """autograd of the masked mean CE with the oracle's mask -> (sum_ce, n_valid, d loss / d logits, mask)"""
    from oracle import whisper_ref as R

    logits, tokens = ce_chain_inputs()
    lg = logits.to(dtype).requires_grad_(True)
    tgt = tokens[:, 1:]
    mask = R.loss_mask(tgt, CE_CHAIN_EOT).reshape(-1)
    ce = torch.nn.functional.cross_entropy(lg, tgt.reshape(-1), reduction="none")
    sum_ce = (ce * mask.to(dtype)).sum()
    n = mask.sum().to(dtype)
    (sum_ce / torch.clamp(n, min=1.0)).backward()
    return sum_ce.detach(), float(n), lg.grad, mask


# ====================================================================== 4. embedding backward
EMB_CASES = [(3, 7, 64), (4, 9, 100), (2, 5, 384)]
EMB_VOCAB = 50


@functools.lru_cache(maxsize=None)
def embed_inputs(B: int, T: int, D: int):
    g = torch.Generator().manual_seed(B * 100 + T * 10 + D)
    tok = torch.randint(1, EMB_VOCAB - 1, (B, T), generator=g)
    tok[0, 1:4] = 17           # a run of one token inside a row
    tok[:, T - 1] = 23         # the same token in every batch row
    tok[1, 0], tok[B - 1, 2] = 0, EMB_VOCAB - 1
    return tok.to(torch.int32), torch.randn(B * T, D, generator=g), torch.randn(EMB_VOCAB, D, generator=g)


def embed_backward_sequential(tok, dx, d_tok0) -> Tuple[np.ndarray, np.ndarray]:
    """The documented order in np.float32 adds: d_tok[tokens[r]] += dx[r] for r ascending; d_pos[t] = 0 + dx[0*T + t] +
    dx[1*T + t] + ... for b ascending.  No products occur, so a kernel that keeps the order is bit-equal."""
    B, T = tok.shape
    dxn = dx.numpy().astype(np.float32)
    d_tok = d_tok0.numpy().astype(np.float32).copy()
    flat = tok.reshape(-1).numpy()
    for r in range(B * T):
        d_tok[flat[r]] = d_tok[flat[r]] + dxn[r]
    d_pos = np.zeros((T, dxn.shape[1]), np.float32)
    for b in range(B):
        d_pos = d_pos + dxn[b * T:(b + 1) * T]
    return d_tok, d_pos


# ====================================================================== 5. column sums, transpose, GELU
COLSUM_COLS = (1, 63, 64, 65, 133)
COLSUM_ROWS = (1, 3, 31, 32, 33, 511, 512, 513, 16385)
COLSUM_MAX_ROWS = 16385
TRANSPOSE_CASES = [(1, 1, 1), (63, 65, 64), (64, 64, 128), (70, 133, 96), (130, 63, 160)]


def colsum_chunks(rows: int, cols: int, workspace_floats: int) -> int:
    """R of wipa_colsum: one launch unless there is a workspace and rows >= 512; then ceil(rows / 256) chunks, at most 64, at
    most what the workspace holds, and never a single chunk through the workspace"""
    if workspace_floats <= 0 or rows < 512:
        return 1
    R = min(64, (rows + 255) // 256)
    if R * cols > workspace_floats:
        R = workspace_floats // cols
    return R if R >= 2 else 1


def colsum_path_adds(rows: int, R: int, accumulate: int) -> int:
    """k = the number of float32 additions on the longest path from an input to out[c], read off colsum_kernel:
    a chunk has per = ceil(rows / R) rows; a thread takes every 4th of them into 8 accumulators, 32 rows per trip, so an
    accumulator gets at most ceil(per / 32) adds; the tail (fewer than 8 rows of the thread) goes into accumulator 0: + 7;
    the 8 accumulators are added as a tree: + 3; the 4 row lanes as a tree: + 2; with R > 1 the finish kernel adds the R
    partials in sequence: + R; accumulate adds the old value: + 1."""
    per = (rows + R - 1) // R
    return (per + 31) // 32 + 7 + 3 + 2 + (R if R > 1 else 0) + (1 if accumulate else 0)


@functools.lru_cache(maxsize=None)
def colsum_inputs(cols: int, integer: bool):
    """x [16385, cols + 7] f32 (the 7 padding columns NaN), a base for accumulate, and the float64 running sums of x and |x|
    over the rows (row r-1 = the sums of the first r rows), computed once"""
    g = torch.Generator().manual_seed(cols + (1000 if integer else 0))
    shape = (COLSUM_MAX_ROWS, cols)
    v = torch.randint(-8, 9, shape, generator=g).float() if integer else torch.randn(shape, generator=g)
    base = torch.randint(-8, 9, (cols,), generator=g).float() if integer else torch.randn(cols, generator=g)
    x = torch.full((COLSUM_MAX_ROWS, cols + 7), float("nan"))
    x[:, :cols] = v
    return x, base, v.double().cumsum(0), v.double().abs().cumsum(0)


GELU_GRID = 4096


def gelu_points() -> torch.Tensor:
    """4104 f32 values: [0, 4100) = +-0, +-1e-30 and the grid of 4096 points on [-12, 12], what the n = 4100 call covers;
    [4100, 4104) = a subnormal, its negative and +-1, what the n = 4 call covers"""
    grid = torch.linspace(-12.0, 12.0, GELU_GRID, dtype=torch.float64).float()
    z = torch.cat([torch.tensor([0.0, -0.0, 1e-30, -1e-30]), grid, torch.tensor([1e-40, -1e-40, 1.0, -1.0])])
    assert z.numel() == 4104 and 0 < float(z[4100]) < 1.1754944e-38
    return z


def gelu64(z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """exact-erf GELU and its derivative in float64"""
    z = z.double()
    cdf = 0.5 * (1.0 + torch.erf(z / np.sqrt(2.0)))
    return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def gelu_series32(z: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """float32 evaluation of the Abramowitz-Stegun 7.1.26 series the kernels use (|eps| <= 1.5e-7 on erf), with exact
    float32 reciprocal and exp: what the formula itself costs before the GPU's approximate rcp / exp2"""
    f = np.float32
    zz = z.numpy().astype(f)
    x = zz * f(0.70710678118654752440)
    ax = np.abs(x)
    t = f(1.0) / (f(0.3275911) * ax + f(1.0))
    p = f(1.061405429) * t + f(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + f(c)
    erf = np.copysign(f(1.0) - p * t * np.exp(-(ax * ax)).astype(f), x).astype(f)
    cdf = f(0.5) * (f(1.0) + erf)
    pdf = f(0.3989422804014327) * np.exp(f(-0.5) * zz * zz).astype(f)
    return (f(0.5) * zz * (f(1.0) + erf)).astype(f), (cdf + zz * pdf).astype(f)
