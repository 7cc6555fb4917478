"""float64 references of the forward attention kernels (csrc/attention.hip), their case tables, the three input regimes, the
per-query-row criterion, CPU restatements of the documented arithmetic (floors) and mutations of the reference (what the
criterion has to see).  Shared by tests/test_attention_ref_host.py and tests/test_gpu_attention_forward.py.  Plain torch on
the CPU; nothing here touches the GPU.

  reference          softmax(Q K^T) V in float64 from the very values the kernel receives (bf16 inputs are rounded first and then
                     widened), with lse and the absolute-value output A[b, q, h] = max_d sum_k p_k |v_kd|.
  row_err            err[b, q, h] = max_d |got - ref| / A[b, q, h]: every query row is judged in its own units, so a small row
                     cannot hide behind a large one; a NaN in ``got`` is an infinite error.  lse: |got - ref|.
  regimes            witness / flat / ramp, see ``inputs``.
  restate            the documented arithmetic of a kernel family on the CPU.  Its row_err against float64 on a test's own inputs
                     is the FLOOR a bound is derived from: bound = floor constant x margin.  The kernels' own figures never
                     enter a bound.
  mutations          deliberately wrong float64 results.  The host test asserts that each exceeds 3 x the bound in some regime.

A visible key set is always a range: query i of batch row b sees keys lo[b, i] .. hi[b, i] (causal: hi = i + Tk - Tq; ragged:
lo = the row's start; the one-row decode kernels clamp a start above the query row to it).  A query with hi < lo is a padding
query of a ragged prompt: dead, not judged, and the kernel leaves the value of the row's first own key there.

Left out: the forms behind WIPA_SELF_ATTN_WAVES, WIPA_ATTN_FWD and WIPA_FLASH_Q128.  They are A/B leftovers that the library
reads once per process, so one pytest process cannot run both sides.

Two things the shapes force.  (1) A one-row decode case has B * H = 6 live queries (3 per batch row where every row has a start
of its own) and up to 10 edge keys, so its witnesses cover the edge keys in ``edge_keys``'s order of priority (0, the last, then
around the last and the first multiple of each stride, larger stride first) as far as the queries go -- the firsts of the smaller
strides are what the shorter caches of the table cover; every other case covers all of them.  (2) Under a causal mask
K and V are shared by rows that see a key and rows that do not, so "the first key beyond the mask" cannot carry a poison of its
own there; the leak of that key is what the ramp regime shows (it is the top-scoring key of every even query) and beyond-the-end
rows of every buffer are NaN in the GPU test.
"""
from __future__ import annotations

import functools
import math
import zlib
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

HD = 64
ATTN_B, ATTN_H = 2, 3
N_CTX = 448  # rows of a self-attention cache
REGIMES = ("witness", "flat", "ramp")
WITNESS_RANGE = (0.3, 0.95)
RAMP_SPAN = 12.0
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


class Case(NamedTuple):
    family: str  # flash_bf16 | flash_f32 | attn | attn_ragged | decode_cache | decode_cross | decode_ragged
    dtype: str   # bf16 | f32
    Tq: int
    Tk: int
    causal: bool = False
    variant: str = ""  # flash_bf16: min | pad (strides, V^T padding);  attn: valu | mfma | tkdev (the kernel it must take)
    starts: Tuple[int, ...] = ()  # ragged: first key of every batch row

    @property
    def B(self) -> int:
        return len(self.starts) if self.starts else ATTN_B

    @property
    def H(self) -> int:
        return ATTN_H

    @property
    def id(self) -> str:
        tail = ("-causal" if self.causal and self.family == "attn" else "") + (f"-{self.variant}" if self.variant else "")
        return f"{self.family}-{self.dtype}-{self.Tq}x{self.Tk}{tail}"


FLASH_BF16_T = (1, 33, 64, 65, 200, 256, 257, 300, 320, 520)  # <= 256: four waves; above: eight (257: one live query in block 2)
FLASH_F32_T = (1, 37, 64, 65, 128, 129, 200)
ATTN_BF16 = ((1, 1, False), (5, 69, True), (15, 64, False), (16, 65, True), (17, 17, True), (33, 200, False))
ATTN_F32_VALU = ((3, 130, False), (15, 15, True))
ATTN_F32_MFMA = ((16, 16, True), (64, 65, False), (65, 129, True), (80, 200, False))
ATTN_F32_TKDEV = (32, 100, False)  # Tq >= 16 with tk_dev set: the f32 MFMA form declines, the VALU kernel runs
RAGGED = ((40, (0, 1, 15, 16, 17, 39)), (130, (0, 63, 64, 65, 100, 129)))
DECODE_CACHE_TK = {"bf16": (1, 8, 31, 32, 33, 127, 128, 129, 448), "f32": (1, 15, 16, 17, 63, 64, 65, 448)}
DECODE_CROSS_TK = (512, 513, 1500)  # 512 | 513: wipa_decode_attn switches to the long-cache instantiation (nt loads)
DECODE_RAGGED_TK = 200
DECODE_RAGGED_STARTS = (0, 1, 31, 32, 33, 127, 128, 199, 300)  # 300 lies above the query row 199: the kernel clamps it

FLASH_BF16_CASES = [Case("flash_bf16", "bf16", T, T, False, var) for T in FLASH_BF16_T for var in ("min", "pad")]
FLASH_F32_CASES = [Case("flash_f32", "f32", T, T) for T in FLASH_F32_T]
ATTN_CASES = ([Case("attn", "bf16", tq, tk, c, "valu") for tq, tk, c in ATTN_BF16] +
              [Case("attn", "f32", tq, tk, c, "valu") for tq, tk, c in ATTN_F32_VALU] +
              [Case("attn", "f32", tq, tk, c, "mfma") for tq, tk, c in ATTN_F32_MFMA] +
              [Case("attn", "f32", *ATTN_F32_TKDEV, "tkdev")])
ATTN_RAGGED_CASES = [Case("attn_ragged", dt, T, T, True, "", st) for dt in ("bf16", "f32") for T, st in RAGGED]
DECODE_CACHE_CASES = [Case("decode_cache", dt, 1, tk) for dt in ("bf16", "f32") for tk in DECODE_CACHE_TK[dt]]
DECODE_CROSS_CASES = [Case("decode_cross", dt, 1, tk) for dt in ("bf16", "f32") for tk in DECODE_CROSS_TK]
DECODE_RAGGED_CASES = [Case("decode_ragged", dt, 1, DECODE_RAGGED_TK, False, "", DECODE_RAGGED_STARTS) for dt in ("bf16", "f32")]
ALL_CASES = (FLASH_BF16_CASES + FLASH_F32_CASES + ATTN_CASES + ATTN_RAGGED_CASES + DECODE_CACHE_CASES + DECODE_CROSS_CASES +
             DECODE_RAGGED_CASES)


def strides(case: Case) -> Tuple[int, ...]:
    """the key strides of the kernel a case runs: flash tiles of 64 keys in two MFMA blocks of 32; the VALU and f32 MFMA kernels
    tiles of 64 keys over 16 key lanes; the decode kernel 32 | 128 keys (bf16) or 16 | 64 (f32) per wave | workgroup trip"""
    if case.family == "flash_bf16":
        return (32, 64)
    if case.family == "flash_f32":
        return (64,)
    if case.family in ("attn", "attn_ragged"):
        return (16, 64)
    return (32, 128) if case.dtype == "bf16" else (16, 64)


def key_range(case: Case) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> lo, hi [B, Tq] int64: query i of row b sees keys lo .. hi; hi < lo marks a dead (padding) query"""
    B, Tq, Tk = case.B, case.Tq, case.Tk
    first = torch.tensor(case.starts if case.starts else (0,) * B, dtype=torch.int64)
    if case.family == "decode_ragged":
        first = first.clamp(max=Tk - 1)
    i = torch.arange(Tq)
    hi = (i + (Tk - Tq)) if case.causal else torch.full((Tq,), Tk - 1)
    return first[:, None].expand(B, Tq).contiguous(), hi[None, :].expand(B, Tq).contiguous()


def edge_keys(n: int, strd: Tuple[int, ...]) -> List[int]:
    """the edge keys of a row of n keys, relative to its first, in order of priority: 0, the last, then the two keys around the
    last multiple of each stride (the ragged tail), then around the first; larger stride first"""
    out = [0, n - 1]
    for which in ("last", "first"):
        for S in sorted(strd, reverse=True):
            m = ((n - 1) // S) * S if which == "last" else S
            if S <= m < n:
                out += [m - 1, m]
    seen, res = set(), []
    for e in out:
        if e not in seen:
            seen.add(e)
            res.append(e)
    return res


def required_edges(case: Case) -> List[Tuple[Tuple[int, ...], int]]:
    """-> [(batch rows, absolute key)]: an edge must be the witness of a live query of one of the rows.  Ragged rows have edges
    of their own (the kernels move the row's base to its start); otherwise any batch row will do."""
    lo, _ = key_range(case)
    if not case.starts:
        return [(tuple(range(case.B)), e) for e in edge_keys(case.Tk, strides(case))]
    req = []
    for b in range(case.B):
        first = int(lo[b, 0])
        req += [((b,), first + e) for e in edge_keys(case.Tk - first, strides(case))]
    return req


def _coprime_step(n: int) -> int:
    a = max(1, int(0.618 * n)) | 1
    while math.gcd(a, n) != 1:
        a += 1
    return a


@functools.lru_cache(maxsize=None)
def witness_map(case: Case) -> Tuple[torch.Tensor, Tuple[Tuple[Tuple[int, ...], int], ...]]:
    """-> wit [B, H, Tq] (the witness key of every query, -1 for a dead one), the required edges left uncovered.
    pi(i) = lo + (a i + s) mod n over the n keys the query sees, a coprime to Tk, s = 7 b + 3 h; under a causal mask the even
    rows take their diagonal key hi.  Then, in the edges' order of priority, every required edge that no query got is given to
    the first query that sees it, is not an even causal row and holds no earlier edge."""
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    lo, hi = key_range(case)
    n = (hi - lo + 1).clamp(min=1)
    a = _coprime_step(Tk)
    i = torch.arange(Tq)
    wit = torch.empty(B, H, Tq, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            wit[b, h] = lo[b] + (a * i + 7 * b + 3 * h) % n[b]
            if case.causal:
                wit[b, h, 0::2] = hi[b, 0::2]
    live = hi >= lo
    wit[~live[:, None, :].expand(B, H, Tq)] = -1
    req = required_edges(case)
    locked = torch.zeros(B, H, Tq, dtype=torch.bool)
    if case.causal:
        locked[:, :, 0::2] = True
    uncovered = []
    for bs, e in req:  # in order of priority: a query that holds an earlier edge is locked, one that holds a later edge may be taken
        done = False
        for b in bs:
            has = torch.nonzero(wit[b] == e)
            if len(has):
                locked[b, has[0, 0], has[0, 1]] = True
                done = True
                break
        for b in (() if done else bs):
            free = torch.nonzero((live[b] & (lo[b] <= e) & (e <= hi[b]))[None, :] & ~locked[b])
            if len(free):
                wit[b, free[0, 0], free[0, 1]] = e
                locked[b, free[0, 0], free[0, 1]] = True
                done = True
                break
        if not done:
            uncovered.append((bs, e))
    return wit, tuple(uncovered)


def _seed(case: Case, regime: str) -> int:
    return zlib.crc32(repr((tuple(case), regime)).encode())


def _round(t: torch.Tensor, dtype: str) -> torch.Tensor:
    """the float32 image of what the kernel receives"""
    return t.to(TORCH_DTYPE[dtype]).float()


@functools.lru_cache(maxsize=None)
def inputs(case: Case, regime: str) -> Dict[str, torch.Tensor]:
    """q [B, Tq, H, 64], k, v [B, Tk, H, 64] as float32 images of ``case.dtype`` values, lo, hi [B, Tq], live [B, Tq].  Shared; do
    not modify.  v = randn in every regime.
      witness  keys are random unit vectors, query (b, h, i) is c k[wit] with c = ln n + 1.5 over the n keys it sees: the
               witness key holds 0.3 .. 0.95 of the row, so a key that is dropped, doubled or read from elsewhere shows.
      flat     q = 0.05 randn, k = 0.6 randn: nearly uniform rows, where denominators matter.
      ramp     dims 62 | 63 of a key hold t - 1 | -t, t its position in the row's key range scaled to [0, 1]; an even query holds
               RAMP_SPAN in dim 62, an odd one in dim 63 (parity of b H + h + i): scores rise from -12 to 0 with the key index
               for even queries and fall for odd ones, so the running maximum moves in every tile for half the lanes of a wave
               and never for the other half, and no score lies above 0 (a zero-score padding key counts)."""
    g = torch.Generator().manual_seed(_seed(case, regime))
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    lo, hi = key_range(case)
    live = hi >= lo
    v = torch.randn(B, Tk, H, HD, generator=g)
    if regime == "witness":
        k = torch.nn.functional.normalize(torch.randn(B, Tk, H, HD, generator=g), dim=-1)
        wit, _ = witness_map(case)
        c = torch.log((hi - lo + 1).clamp(min=1).float()) + 1.5  # [B, Tq]: the witness key's score, the keys being unit vectors
        idx = wit.clamp(min=0).permute(0, 2, 1)  # [B, Tq, H]
        q = torch.gather(k, 1, idx[..., None].expand(B, Tq, H, HD)) * c[:, :, None, None]
    elif regime == "flat":
        q = 0.05 * torch.randn(B, Tq, H, HD, generator=g)
        k = 0.6 * torch.randn(B, Tk, H, HD, generator=g)
    elif regime == "ramp":
        q = 0.3 * torch.randn(B, Tq, H, HD, generator=g)
        k = 0.3 * torch.randn(B, Tk, H, HD, generator=g)
        first = lo[:, 0].float()
        t = ((torch.arange(Tk)[None, :] - first[:, None]) / (Tk - 1 - first[:, None]).clamp(min=1.0)).clamp(0.0, 1.0)  # [B, Tk]
        k[..., 62] = (t - 1.0)[:, :, None]
        k[..., 63] = (-t)[:, :, None]
        par = (torch.arange(B)[:, None, None] * H + torch.arange(H)[None, None, :] + torch.arange(Tq)[None, :, None]) % 2
        q[..., 62] = RAMP_SPAN * (par == 0)
        q[..., 63] = RAMP_SPAN * (par == 1)
    else:
        raise ValueError(regime)
    return {"q": _round(q, case.dtype), "k": _round(k, case.dtype), "v": _round(v, case.dtype), "lo": lo, "hi": hi, "live": live}


# ====================================================================== reference and criterion
def visible(lo: torch.Tensor, hi: torch.Tensor, Tk: int) -> torch.Tensor:
    """[B, Tq, Tk] bool.  A dead query sees the key at lo alone, as the kernels leave it."""
    j = torch.arange(Tk)[None, None, :]
    hi = torch.maximum(hi, lo)
    return (j >= lo[..., None]) & (j <= hi[..., None])


def scores(x, dtype=torch.float64) -> torch.Tensor:
    return torch.einsum("bqhd,bkhd->bhqk", x["q"].to(dtype), x["k"].to(dtype))


def attend(s: torch.Tensor, vis: torch.Tensor, v: torch.Tensor):
    """-> out [B, Tq, H, 64], lse [B, H, Tq], A [B, Tq, H], p [B, H, Tq, Tk] in the dtype of ``s``"""
    s = s.masked_fill(~vis[:, None], float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    v = v.to(s.dtype)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    A = torch.einsum("bhqk,bkhd->bqhd", p, v.abs()).amax(-1)
    return out, lse, A, p


@functools.lru_cache(maxsize=None)
def reference(case: Case, regime: str) -> Dict[str, torch.Tensor]:
    """float64 {out, lse, A} of one (case, regime), computed once and shared; do not modify"""
    x = inputs(case, regime)
    out, lse, A, _ = attend(scores(x), visible(x["lo"], x["hi"], case.Tk), x["v"])
    return {"out": out, "lse": lse, "A": A}


def row_err(got: torch.Tensor, ref: Dict[str, torch.Tensor]) -> torch.Tensor:
    """[B, Tq, H]: max_d |got - ref| / A, inf where got holds a NaN"""
    d = (got.double() - ref["out"]).abs().amax(-1) / ref["A"]
    return torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)


def worst_row(got: torch.Tensor, ref: Dict[str, torch.Tensor], live: torch.Tensor) -> float:
    """the worst live query row of a case"""
    return float(row_err(got, ref)[live].max())


def worst_lse(got: torch.Tensor, ref: Dict[str, torch.Tensor], live: torch.Tensor) -> float:
    d = (got.double() - ref["lse"]).abs().permute(0, 2, 1)  # [B, Tq, H]
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float(d[live].max())


# ====================================================================== restatements of the documented arithmetic (floors)
def floor_key(case: Case, f32_split: bool = False) -> Tuple[str, str]:
    """the (family, arithmetic) a floor constant is kept under"""
    if case.family == "flash_bf16":
        return case.family, "bf16"
    if case.family == "flash_f32":
        return case.family, "f32_split" if f32_split else "f32"
    return case.family, case.dtype


def restate(case: Case, regime: str, f32_split: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> out, lse of the kernel's documented arithmetic on the CPU.
      bf16 flash   f32 scores, P rounded to bf16 for the P V MFMA, l summed from the unrounded p, output rounded to bf16
                   (the rounding of P is relative, so the running maximum it is taken under does not matter).
      f32 split    f32 scores (three bf16 terms per operand: f32-exact), P V on a two-term bf16 split of both operands with the
                   product of the two low terms left out, as the header of flash_enc_f32s_kernel says.
      the rest     the float32 softmax statement; a bf16 kernel rounds its output to bf16."""
    kind = "flash_bf16" if case.family == "flash_bf16" else "f32_split" if f32_split else case.dtype
    return restate_inputs(inputs(case, regime), kind)


def restate_inputs(x, kind: str, pad: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``restate`` on given inputs; kind: flash_bf16 | f32_split | bf16 | f32.  pad [B, Tq] (flash_bf16 only): that many
    zero-score keys counted in l, the padded-denominator mutation inside the restatement."""
    Tk = x["k"].shape[1]
    vis = visible(x["lo"], x["hi"], Tk)
    if kind in ("flash_bf16", "f32_split"):
        s = scores(x).float().masked_fill(~vis[:, None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        if pad is not None:
            m = m.clamp(min=0.0)
        p = torch.exp(s - m)
        l = p.double().sum(-1)
        if pad is not None:
            l = l + pad.double()[:, None, :] * torch.exp(-m[..., 0].double())
        v = x["v"]
        if kind == "flash_bf16":
            num = torch.einsum("bhqk,bkhd->bqhd", p.bfloat16().double(), v.double())
        else:
            ph, vh = p.bfloat16().float(), v.bfloat16().float()
            pl, vl = (p - ph).bfloat16().float(), (v - vh).bfloat16().float()
            num = sum(torch.einsum("bhqk,bkhd->bqhd", a.double(), b.double()) for a, b in ((ph, vh), (ph, vl), (pl, vh)))
        out = (num / l.permute(0, 2, 1)[..., None]).float()
        lse = (m[..., 0].double() + torch.log(l)).float()
        return (out.bfloat16().float() if kind == "flash_bf16" else out), lse
    out, lse, _, _ = attend(scores(x, torch.float32), vis, x["v"])
    return _round(out, kind), lse


def floor(case: Case, regime: str, f32_split: bool = False) -> Tuple[float, float]:
    """-> worst live row of the restatement against float64, worst |lse - ref|"""
    x, ref = inputs(case, regime), reference(case, regime)
    out, lse = restate(case, regime, f32_split)
    return worst_row(out, ref, x["live"]), worst_lse(lse, ref, x["live"])


# ====================================================================== mutations of the reference
def _range_out(case: Case, x, lo, hi, k=None, v=None, q=None) -> torch.Tensor:
    y = dict(x, **{n: t for n, t in (("q", q), ("k", k), ("v", v)) if t is not None})
    return attend(scores(y), visible(lo, hi, case.Tk), y["v"])[0]


def _pad_keys(case: Case, x) -> torch.Tensor:
    """[B, Tq]: the keys between a row's last and the end of its last tile (the decode kernel: of the workgroup's last trip)"""
    n = (x["hi"] - x["lo"] + 1).clamp(min=1)
    S = max(strides(case))
    return (n + S - 1) // S * S - n


def mutations(case: Case, regime: str) -> Dict[str, torch.Tensor]:
    """{name: wrong float64 out} for every mutation that applies to the case.
      drop_key[b..:j]      key j missing from the rows that see it beside others, for every covered edge key
      pad_denominator      the zero-score keys that fill a row's last tile counted in its denominator
      causal+1 / causal-1  the causal mask off by one (the diagonal's neighbour leaks / the diagonal is lost)
      start+1 / start-1    a ragged row's start off by one
      v_head+1, q_row+1, clip+1     V of the next head, the next query row, K and V of the next clip
      no_rescale           the accumulator not rescaled when the running maximum moves between tiles"""
    x, ref = inputs(case, regime), reference(case, regime)
    lo, hi, Tk = x["lo"], x["hi"], case.Tk
    vis = visible(lo, hi, Tk)
    s = scores(x)
    res: Dict[str, torch.Tensor] = {}
    if Tk > 1:
        _, uncovered = witness_map(case)
        for bs, e in required_edges(case):
            if (bs, e) in uncovered:
                continue
            v2 = vis.clone()
            drop = torch.zeros_like(vis)
            drop[list(bs), :, e] = True
            v2 &= ~(drop & (vis.sum(-1, keepdim=True) > 1))
            if not torch.equal(v2, vis):
                res[f"drop_key[{bs[0]}{'..' if len(bs) > 1 else ''}:{e}]"] = attend(s, v2, x["v"])[0]
    pad = _pad_keys(case, x)
    if int(pad[x["live"]].max()) > 0:
        scale = 1.0 / (1.0 + pad.double()[:, None, :] * torch.exp(-ref["lse"]))  # [B, H, Tq]
        res["pad_denominator"] = ref["out"] * scale.permute(0, 2, 1)[..., None]
    if case.causal and case.Tq > 1:
        res["causal+1"] = _range_out(case, x, lo, (hi + 1).clamp(max=Tk - 1))
        res["causal-1"] = _range_out(case, x, lo, torch.maximum(hi - 1, torch.minimum(lo, hi)))
    if case.starts:
        res["start+1"] = _range_out(case, x, torch.minimum(lo + 1, torch.maximum(hi, lo)), hi)
        res["start-1"] = _range_out(case, x, (lo - 1).clamp(min=0), hi)
    res["v_head+1"] = _range_out(case, x, lo, hi, v=x["v"].roll(-1, 2))
    if case.Tq > 1:
        res["q_row+1"] = ref["out"].roll(-1, 1)
    res["clip+1"] = _range_out(case, x, lo, hi, k=x["k"].roll(-1, 0), v=x["v"].roll(-1, 0))
    S = max(strides(case))
    if int((hi - lo + 1).max()) > S:
        sm = s.masked_fill(~vis[:, None], float("-inf"))
        tile = ((torch.arange(Tk)[None, None, :] - lo[..., None]).clamp(min=0) // S)[:, None]  # [B, 1, Tq, Tk]
        n_t = int(tile.max()) + 1
        run = torch.full(sm.shape[:-1], float("-inf"), dtype=sm.dtype)
        m_at = torch.empty_like(sm)  # the running maximum after the tile a key lies in
        for t in range(n_t):
            in_t = (tile == t).expand_as(sm)
            run = torch.maximum(run, sm.masked_fill(~in_t, float("-inf")).amax(-1))
            m_at = torch.where(in_t, run[..., None].expand_as(sm), m_at)
        num = torch.einsum("bhqk,bkhd->bqhd", torch.exp(sm - m_at), x["v"].double())
        den = torch.exp(sm - run[..., None]).sum(-1)
        res["no_rescale"] = num / den.permute(0, 2, 1)[..., None]
    return res


def old_flash_inputs(T: int) -> Dict[str, torch.Tensor]:
    """the inputs of tests/test_gpu_kernels.py::test_flash_attention_encoder_bf16 (B = 2, H = 2, 0.6 randn, seed T)"""
    g = torch.Generator().manual_seed(T)
    B, H = 2, 2
    q = (torch.randn(B, T, H, 64, generator=g) * 0.6).bfloat16().float()
    k = (torch.randn(B, T, H, 64, generator=g) * 0.6).bfloat16().float()
    v = torch.randn(B, T, H, 64, generator=g).bfloat16().float()
    lo = torch.zeros(B, T, dtype=torch.int64)
    return {"q": q, "k": k, "v": v, "lo": lo, "hi": lo + (T - 1), "live": torch.ones(B, T, dtype=torch.bool)}
