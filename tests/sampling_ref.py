"""CPU restatement of the sampling tail (csrc/elementwise.hip: row_pick<.., SAMPLE>; include/wipa.h "Temperature sampling"):
Philox4x32-10 in numpy integers, u = ((word >> 9) + 0.5) * 2^-23, the Gumbel noise and the keys in float64, the filtered row from
tests/timestamp_ref.apply_rules.  What wipa_sample_noise / wipa_sample_step / the sampling decode are tested against."""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

import timestamp_ref as TR

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(counter, key):
    """``counter``: four arrays (or ints) of 32-bit words, broadcast against each other; ``key``: two.  Returns four uint64 arrays
    holding the 32-bit output words.  Salmon et al., SC'11; ten rounds, the key bumped by the Weyl constants between rounds."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def uniform_from_words(words) -> np.ndarray:
    """u in (0, 1): 23 random bits and a half -- every value is exact in float32 and in float64"""
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_noise(seed: int, streams, attempt: int, p: int, V: int) -> np.ndarray:
    """g [N, V] float64 for ``streams`` [N, 2] (lo, hi): key (seed_lo, seed_hi), counter (c >> 2, p | attempt << 16, lo, hi), word c & 3"""
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1, 2)
    nq = (V + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, :]
    words = philox4x32_10((q, (int(p) | (int(attempt) << 16)) & 0xFFFFFFFF, streams[:, :1], streams[:, 1:]),
                          (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w = np.stack(words, axis=-1).reshape(streams.shape[0], 4 * nq)[:, :V]
    return -np.log(-np.log(uniform_from_words(w)))


@dataclass
class SampleStep:
    row: np.ndarray      # the filtered row l, float64 (-inf: dead)
    next: int            # argmax of l / T + g over the alive columns, lowest column on ties
    logprob: float       # l[next] - logsumexp(l): the UNTEMPERED log-softmax at the drawn column
    key_margin: float    # top-1 minus top-2 key (inf with fewer than two alive columns)
    lse: float           # logsumexp(l)
    fired: dict


def sample_row(logits, temperature: float, noise: np.ndarray, mask: Optional[np.ndarray] = None, rules: Optional[dict] = None,
               seq: Sequence[int] = (), first: bool = False) -> SampleStep:
    """one row: ``noise`` [V] from gumbel_noise; ``rules``: dict(tb=, nt=, eot=, max_init=) or None (the plain masked row)"""
    if rules is None:
        l = np.asarray(logits, dtype=np.float64).copy()
        if mask is not None:
            l = l + np.asarray(mask, dtype=np.float64)
        fired = {}
    else:
        st = TR.apply_rules(logits, seq, rules["tb"], rules["nt"], rules["eot"], first, rules.get("max_init", 50), mask)
        l, fired = st.row, st.fired
    lse = TR._logsumexp(l)
    alive = np.isfinite(l)
    keys = np.where(alive, l / float(temperature) + noise, -np.inf)
    nxt = int(np.argmax(keys))
    top2 = np.sort(keys)[-2:]
    margin = float(top2[1] - top2[0]) if alive.sum() >= 2 else np.inf
    return SampleStep(l, nxt, float(l[nxt] - lse), margin, lse, fired)


def chi2_quantile(q: float, df: int) -> float:
    """the q quantile of chi-square(df), by bisection on the regularised incomplete gamma function"""
    import torch

    lo, hi = 0.0, 50.0 * df + 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        cdf = float(torch.special.gammainc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(mid / 2.0, dtype=torch.float64)))
        lo, hi = (mid, hi) if cdf < q else (lo, mid)
    return hi


def chi_square_vs_softmax(tokens, l, temperature: float):
    """(statistic, degrees of freedom, the 1 - 1e-6 quantile) of the draws ``tokens`` against softmax(l / T); bins whose
    expectation is below 5 are pooled into one"""
    l = np.asarray(l, dtype=np.float64)
    tokens = np.asarray(tokens)
    z = l / float(temperature)
    pr = np.exp(z - TR._logsumexp(z))
    assert (pr[tokens] > 0).all(), "a dead column was drawn"
    n = len(tokens)
    counts = np.bincount(tokens, minlength=len(l)).astype(np.float64)
    expect = n * pr
    big = expect >= 5
    obs, exp = list(counts[big]), list(expect[big])
    if (~big & (pr > 0)).any():
        obs.append(counts[~big].sum())
        exp.append(expect[~big].sum())
    obs, exp = np.array(obs), np.array(exp)
    stat = float(((obs - exp) ** 2 / exp).sum())
    df = len(obs) - 1
    return stat, df, chi2_quantile(1.0 - 1e-6, df)


# ---------------------------------------------------------------- shared inputs of the host and the GPU distribution test
DIST_V, DIST_ROWS, DIST_T, DIST_SEED = 67, 4096, 0.7, 20261018
DIST_DEAD = (5, 31, 66)  # the last one is a trailing column (V mod 4 = 3)


def distribution_case():
    """(logits [V] f32, mask [V] f32 with three -inf columns, streams [4096, 2])"""
    l = (np.random.default_rng(67).standard_normal(DIST_V) * 2.0).astype(np.float32)
    streams = np.stack([np.arange(DIST_ROWS) + 1000, np.arange(DIST_ROWS) % 3], axis=1)
    return l, TR.vocab_mask(DIST_V, DIST_DEAD), streams
