"""CPU restatement of the SpecAugment draw (include/wipa.h "SpecAugment"; csrc/spec_augment.hip): integers only, on
sampling_ref.philox4x32_10.  What wipa_spec_augment_plan, the kernel's mask and the trainer's augmented step are tested against."""
from typing import Optional, Sequence

import numpy as np

import sampling_ref as SR

MAX_SPANS = 64


def rate_q16(prob: float, length: int) -> int:
    return min(65536, round(prob / length * 65536))


def _word(k, axis: int, stream, seed: int):
    """word 0 of philox4x32_10 at counter (k, axis, stream_lo, stream_hi), key (seed lo, seed hi); ``k`` may be an array"""
    return SR.philox4x32_10((k, axis, int(stream[0]), int(stream[1])), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))[0]


def axis_length(axis: int, n_frames: Optional[int], frames: int, n_mels: int) -> int:
    if axis == 1:
        return n_mels
    return frames if n_frames is None else min(max(int(n_frames), 0), frames)


def span_count(rate: int, min_masks: int, L: int, axis: int, stream, seed: int) -> int:
    if L == 0:
        return 0
    x = int(rate) * int(L)
    word = int(_word(0xFFFFFFFF, axis, stream, seed))
    return min(MAX_SPANS, max(int(min_masks), (x >> 16) + (1 if (word >> 16) < (x & 0xFFFF) else 0)))


def spans(rate: int, length: int, min_masks: int, L: int, axis: int, stream, seed: int):
    """(w, [start of every span]) of one clip and axis"""
    w = min(int(length), int(L))
    n = span_count(rate, min_masks, L, axis, stream, seed)
    if n == 0:
        return w, []
    words = np.asarray(_word(np.arange(n, dtype=np.uint64), axis, stream, seed), dtype=np.uint64)
    starts = (words * np.uint64(L - w + 1)) >> np.uint64(32)  # umulhi: 32 x 32 bits fit uint64
    return w, [int(s) for s in starts]


def plan(rates: Sequence[int], lengths: Sequence[int], min_masks: Sequence[int], streams, n_frames, frames: int, n_mels: int,
         seed: int) -> np.ndarray:
    """int32 [B, 2, 65]: the count, then the starts, -1 in the unused places -- the table wipa_spec_augment_plan writes"""
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1, 2)
    out = np.full((streams.shape[0], 2, MAX_SPANS + 1), -1, dtype=np.int32)
    for b, st in enumerate(streams):
        for a in range(2):
            L = axis_length(a, None if n_frames is None else n_frames[b], frames, n_mels)
            _, starts = spans(rates[a], lengths[a], min_masks[a], L, a, st, seed)
            out[b, a, 0] = len(starts)
            out[b, a, 1:1 + len(starts)] = starts
    return out


def mask(rates, lengths, min_masks, streams, n_frames, frames: int, n_mels: int, seed: int) -> np.ndarray:
    """bool [B, frames, n_mels]: True where the element becomes ``fill``"""
    streams = np.asarray(streams, dtype=np.uint64).reshape(-1, 2)
    out = np.zeros((streams.shape[0], frames, n_mels), dtype=bool)
    for b, st in enumerate(streams):
        for a in range(2):
            L = axis_length(a, None if n_frames is None else n_frames[b], frames, n_mels)
            w, starts = spans(rates[a], lengths[a], min_masks[a], L, a, st, seed)
            for s in starts:
                assert 0 <= s and s + w <= L
                if a == 0:
                    out[b, s:s + w, :] = True
                else:
                    out[b, :, s:s + w] = True
    return out


def apply(mel: np.ndarray, m: np.ndarray, fill: float = 0.0) -> np.ndarray:
    """a masked copy of ``mel`` [B, frames, n_mels] f32: ``fill``'s bits where ``m``, the input's bits elsewhere"""
    out = np.array(mel, dtype=np.float32, copy=True)
    out[m] = np.float32(fill)
    return out
