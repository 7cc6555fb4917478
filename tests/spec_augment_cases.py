"""The grid of SpecAugment settings that the host test (tests/test_spec_augment_host.py: plan against restatement) and the GPU test
(tests/test_gpu_spec_augment.py: kernel against the restatement's mask) walk, and how a grid point becomes an augmenter."""
import itertools

import numpy as np

import spec_augment_ref as SA

FRAMES, N_MELS, BATCHES, LENGTHS, MIN_MASKS = (66, 150, 3000), (80, 128), (1, 3), (1, 10, 27), (0, 2, 64)
KINDS = ("zero", "p05", "one", "low0", "lowffff")  # prob 0 | 0.05 | 1.0 (length 1 only) | x & 0xffff == 0 | x & 0xffff == 0xffff
SEED = 0x1234_5678_9ABC_DEF0


def n_frames_values(length: int, frames: int):
    return (0, 1, length - 1, length, length + 1, frames, None)


def rate_for(kind: str, length: int, L: int, L_max: int):
    """the Q16 rate of a grid point on an axis of length L (refusal taken at L_max), or None when no rate gives the wanted low
    bits of x = rate * L within the 64-span rule (0xffff needs an odd L)"""
    if kind == "zero":
        return 0
    if kind == "p05":
        return SA.rate_q16(0.05, length)
    if kind == "one":
        return SA.rate_q16(1.0, length) if length == 1 else None
    want = 0 if kind == "low0" else 0xFFFF
    r = np.arange(1, 65537, dtype=np.int64)
    ok = ((r * L) & 0xFFFF) == want
    ok &= ((r * L_max) >> 16) + 1 <= SA.MAX_SPANS
    hit = r[ok]
    return int(hit[len(hit) // 2]) if len(hit) and L > 0 else None


def refused(rates, frames: int, n_mels: int) -> bool:
    return any(((rates[a] * (frames, n_mels)[a]) >> 16) + 1 > SA.MAX_SPANS for a in range(2))


def grid(frames: int, n_mels: int):
    """(B, length, n_frames value, kind, min_masks, rates) of every grid point that has a probability"""
    for B, length, kind, mm in itertools.product(BATCHES, LENGTHS, KINDS, MIN_MASKS):
        for nf in n_frames_values(length, frames):
            L0 = SA.axis_length(0, nf, frames, n_mels)
            rates = (rate_for(kind, length, L0, frames), rate_for(kind, length, n_mels, n_mels))
            if rates[0] is None and rates[1] is None:
                continue
            rates = tuple(0 if r is None else r for r in rates)  # an axis without such a probability is drawn with none
            yield B, length, nf, kind, mm, rates


def augmenter(audio, rates, length: int, mm: int, fill: float = 0.0, seed: int = SEED):
    """through the probabilities, as a user sets it: rate * length / 65536 is exact in float64 and rounds back to the rate.  A
    rate of the two low-bits kinds that no probability <= 1 reaches at this length (x & 0xffff == 0xffff has ONE rate per odd L) is
    written into the cfg, which is what the C ABI takes."""
    probs = [r * length / 65536 for r in rates]
    aug = audio.SpecAugment(min(probs[0], 1.0), length, mm, min(probs[1], 1.0), length, mm, fill=fill, seed=seed)
    for a in range(2):
        if probs[a] > 1.0:
            aug.cfg.rate_q16[a] = rates[a]
    assert tuple(aug.cfg.rate_q16) == tuple(rates)
    return aug


def streams_for(B: int, salt: int) -> np.ndarray:
    return np.stack([np.arange(B) * 7919 + salt, np.full(B, salt % 5)], axis=1)
