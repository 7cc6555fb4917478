"""CPU: the SpecAugment draw.  wipa_spec_augment_plan (the text the kernel compiles, csrc/spec_augment.hip) against the numpy
restatement tests/spec_augment_ref.py, exactly, over the grid of include/wipa.h's statement; the properties of the spans; the mean
span count; the refusals by name; the frame counts the ingest reports.  No GPU is touched."""
import ctypes as C
import itertools
import wave

import numpy as np
import pytest

import sampling_ref as SR
import spec_augment_ref as SA
from spec_augment_cases import FRAMES, KINDS, N_MELS, SEED, augmenter, grid, rate_for, refused, streams_for


@pytest.fixture(scope="module")
def audio():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import audio

    return audio


@pytest.mark.parametrize("frames,n_mels", list(itertools.product(FRAMES, N_MELS)))
def test_plan_equals_the_restatement_over_the_grid(audio, frames, n_mels):
    from whisper_ipa_amd._lib import WipaError

    seen = {k: 0 for k in KINDS}
    n_refused = 0
    for i, (B, length, nf, kind, mm, rates) in enumerate(grid(frames, n_mels)):
        aug = augmenter(audio, rates, length, mm)
        streams = streams_for(B, i)
        n_frames = None if nf is None else [nf] * B
        if refused(rates, frames, n_mels):
            with pytest.raises(WipaError, match="too many spans"):
                aug.plan(streams, n_frames, frames, n_mels)
            n_refused += 1
            continue
        got = aug.plan(streams, n_frames, frames, n_mels)
        want = SA.plan(rates, (length, length), (mm, mm), streams, n_frames, frames, n_mels, SEED)
        assert got.dtype == np.int32 and got.shape == (B, 2, 65)
        assert np.array_equal(got, want), (B, length, nf, kind, mm, rates)
        for b in range(B):  # every start plus w stays within L
            for a in range(2):
                L = SA.axis_length(a, nf, frames, n_mels)
                w = min(length, L)
                n = got[b, a, 0]
                assert 0 <= n <= 64 and (n >= min(mm, 64) or L == 0) and (L > 0 or n == 0)
                assert ((got[b, a, 1:1 + n] >= 0) & (got[b, a, 1:1 + n] + w <= L)).all()
        seen[kind] += 1
    assert all(seen[k] > 0 for k in ("zero", "p05", "low0")), seen
    # 0xffff needs an odd L, and an odd L has ONE such rate (-1 / L mod 65536): for the odd n_frames values of this grid (1, 9, 11,
    # 27) these are 65535, 29127, 29789 and 9709, and at 3000 frames the 64-span rule admits no rate above 1376
    assert seen["lowffff"] > 0 or frames == 3000, seen
    assert n_refused > 0  # prob 1.0 at length 1 on the long axis


def test_low_bits_of_x_are_what_the_grid_says():
    """the two edge probabilities do put x & 0xffff at 0 and at 0xffff, where the Bernoulli term is never / almost always taken"""
    r0, rf = rate_for("low0", 10, 80, 80), rate_for("lowffff", 10, 9, 66)
    assert r0 and (r0 * 80) & 0xFFFF == 0
    assert rf and (rf * 9) & 0xFFFF == 0xFFFF


def test_a_row_is_the_same_alone_and_in_a_batch_and_follows_its_stream(audio):
    aug = audio.SpecAugment(0.3, 10, 2, 0.2, 27, 1, seed=SEED)
    streams = np.array([[5, 0], [6, 0], [7, 3]])
    n_frames = [150, 66, 11]
    batch = aug.plan(streams, n_frames, 150, 80)
    assert np.array_equal(batch, SA.plan(tuple(aug.cfg.rate_q16), (10, 27), (2, 1), streams, n_frames, 150, 80, SEED))
    for b in range(3):
        assert np.array_equal(aug.plan(streams[b:b + 1], n_frames[b:b + 1], 150, 80)[0], batch[b])
    moved = aug.plan(np.array([[5, 1], [6, 1], [7, 4]]), n_frames, 150, 80)  # stream_hi changed (the step count of the trainer)
    for b in range(3):
        assert not np.array_equal(moved[b], batch[b])
    other_seed = audio.SpecAugment(0.3, 10, 2, 0.2, 27, 1, seed=SEED + (1 << 32)).plan(streams, n_frames, 150, 80)
    assert not np.array_equal(other_seed, batch)  # the high word of the seed is part of the key


def test_no_probability_and_no_minimum_is_an_empty_plan(audio):
    aug = audio.SpecAugment(0.0, 10, 0, 0.0, 10, 0)
    p = aug.plan(streams_for(3, 1), [0, 17, 3000], 3000, 128)
    assert (p[:, :, 0] == 0).all() and (p[:, :, 1:] == -1).all()


def test_mean_span_count(audio):
    """4096 streams at prob 0.05, length 10, L 3000: n = floor(x / 65536) + Bernoulli((x & 0xffff) / 65536), so the mean count is
    within 4 standard errors of x / 65536 -- on the restatement first, then on the plan"""
    rate, L, N = SA.rate_q16(0.05, 10), 3000, 4096
    x = rate * L
    p = (x & 0xFFFF) / 65536
    bound = 4 * np.sqrt(p * (1 - p) / N)
    streams = np.stack([np.arange(N) + 31, np.arange(N) % 7], axis=1)
    words = SR.philox4x32_10((0xFFFFFFFF, 0, streams[:, 0], streams[:, 1]), (SEED & 0xFFFFFFFF, SEED >> 32))[0]
    ref = (x >> 16) + ((np.asarray(words, dtype=np.uint64) >> np.uint64(16)) < np.uint64(x & 0xFFFF))
    assert abs(ref.mean() - x / 65536) <= bound, (ref.mean(), x / 65536, bound)
    assert [SA.span_count(rate, 0, L, 0, s, SEED) for s in streams[:64]] == ref[:64].tolist()
    aug = audio.SpecAugment(0.05, 10, 0, seed=SEED)
    got = aug.plan(streams, None, L, 80)[:, 0, 0]
    assert np.array_equal(got, ref)
    assert abs(got.mean() - x / 65536) <= bound


def test_refusals_are_by_name(audio):
    from whisper_ipa_amd import _lib

    one = np.array([[0, 0]])
    with pytest.raises(_lib.WipaError, match="too many spans.*mask_time"):
        audio.SpecAugment(1.0, 1, 0).plan(one, None, 66, 80)
    with pytest.raises(_lib.WipaError, match="too many spans.*mask_feature"):
        audio.SpecAugment(0.0, 10, 0, 1.0, 1, 0).plan(one, None, 66, 80)
    audio.SpecAugment(63 / 66, 1, 0).plan(one, None, 66, 80)  # just under 63 spans and the Bernoulli term: within the 64
    with pytest.raises(_lib.WipaError, match="mask_time_min_masks"):
        audio.SpecAugment(mask_time_min_masks=65)
    with pytest.raises(_lib.WipaError, match="mask_feature_min_masks"):
        audio.SpecAugment(mask_feature_min_masks=-1)
    with pytest.raises(_lib.WipaError, match="mask_time_length"):
        audio.SpecAugment(mask_time_length=0)
    with pytest.raises(_lib.WipaError, match="mask_feature_length"):
        audio.SpecAugment(mask_feature_length=0)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(_lib.WipaError, match="mask_time_prob"):
            audio.SpecAugment(mask_time_prob=bad)
        with pytest.raises(_lib.WipaError, match="mask_feature_prob"):
            audio.SpecAugment(mask_feature_prob=bad)
    # the C entry checks a hand-made cfg itself
    lib = _lib.lib()
    out = np.empty((1, 2, 65), dtype=np.int32)
    st = np.zeros((1, 2), dtype=np.uint32)
    for field, value, name in (("length", 0, b"mask_time_length"), ("min_masks", 65, b"mask_time_min_masks"), ("rate_q16", 65537, b"rate_q16")):
        cfg = _lib.SpecAugmentCfg()
        cfg.length[0] = cfg.length[1] = 10
        getattr(cfg, field)[0] = value
        assert lib.wipa_spec_augment_plan(C.byref(cfg), st.ctypes.data, None, 1, 66, 80, 0, out.ctypes.data) != 0
        assert name in lib.wipa_last_error()


def test_frame_counts_from_the_ingest_host_part(audio, tmp_path):
    """ceil(samples / 160), capped at 3000, from the sample counts PcmBatch holds (the host part of the ingest: no GPU)"""
    lengths = (1, 160, 161, 16000 * 3 + 7, 16000 * 31)
    paths = []
    for i, n in enumerate(lengths):
        p = tmp_path / f"c{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(np.zeros(n, dtype="<i2").tobytes())
        paths.append(str(p))
    counts = audio.PcmBatch(paths, pin=False).sample_counts()
    assert counts == [1, 160, 161, 48007, 480000]
    assert audio.frames_of_samples(counts) == [1, 1, 2, 301, 3000]
