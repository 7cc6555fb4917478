"""The log-mel references against each other, on the CPU: the two f32 references (the oracle's FFT path, the matrix emulation of
the fused kernel) pass the rule the kernels are held to (tests/test_gpu_logmel.py), and every planted fault of
``logmel_ref.emulate_f32`` breaks it on at least one clip -- so a kernel with such a fault cannot pass."""
import numpy as np
import pytest

import logmel_ref as L
from oracle import whisper_ref as R


def test_signals_are_seeded_f32_clips_in_batch_order():
    S = L.signals()
    assert tuple(S) == L.ORDER and len(S) == 9
    for name, a in S.items():
        assert a.dtype == np.float32 and a.shape == (L.N_SAMPLES,) and np.isfinite(a).all() and np.abs(a).max() <= 1.0, name
        assert np.array_equal(a, L.cached_signals()[name]), name  # seeded: two builds agree bit for bit
    assert not S["silence"].any()
    assert set(np.flatnonzero(S["impulses"])) == set(L.IMPULSES_AT)
    assert np.array_equal(S["speech_2s"][: L.SHORT_SAMPLES], S["speech"][: L.SHORT_SAMPLES]) and not S["speech_2s"][L.SHORT_SAMPLES:].any()
    assert np.abs(S["noise_clipped"]).max() == 1.0 and 0 < (np.abs(S["noise_clipped"]) == 1.0).mean() < 0.5
    assert abs(S["speech"].mean() - 0.02) < 5e-3
    loud, quiet = L.ORDER.index(L.LOUD), L.ORDER.index(L.QUIET)
    assert loud == 0 and 0 < quiet < len(L.ORDER) - 1  # a quiet clip sits between loud ones, and not in workspace slot 0


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("name", L.ORDER)
def test_f32_references_pass_the_rule_they_set(name, n_mels):
    r = L.reference(name, n_mels)
    print(f"{name} n_mels={n_mels}: max {r.max:.3f}  clamped {r.n_clamped}  oracle-f32 {r.e_oracle:.2e}  emulation {r.e_emulation:.2e}  "
          f"bound {r.bound:.2e}")
    assert r.y.shape == (L.N_FRAMES, n_mels) and r.y.dtype == np.float64
    assert r.e_oracle <= r.bound and r.e_emulation <= r.bound
    assert r.bound == max(4.0 * max(r.e_oracle, r.e_emulation), 2e-6)
    assert r.bound <= 1e-3  # no clip is held to less than the white-noise tests of test_gpu_model.py ask
    # the reference agrees with the oracle on WHICH elements sit on the floor, up to those within the bound of it
    o = R.log_mel_spectrogram(L.cached_signals()[name], n_mels)
    assert abs(float(o.min()) - r.y.min()) <= r.bound


def test_reference64_of_a_pure_tone_is_what_the_window_says():
    """a 0.5 sine at bin 25 exactly: |X[25]| = 0.5 * sum(w) / 2 = 50, power 2500 spread over the mel filters by their weights at
    bins 24..26 (Hann main lobe: 1/4, 1, 1/4 in power ... amplitudes 1/2, 1, 1/2)"""
    y, mx = L.reference64(L.cached_signals()["tone_1k"], 80)
    w = R.mel_filters(80).astype(np.float64)
    mel = w[:, 24] * 625.0 + w[:, 25] * 2500.0 + w[:, 26] * 625.0
    assert abs(mx - np.log10(mel.max())) < 1e-6
    assert abs(y[1500].max() - (np.log10(mel.max()) + 4) / 4) < 1e-6
    assert y.min() == (mx - 8 + 4) / 4


@pytest.mark.parametrize("fault", L.FAULTS)
def test_planted_fault_exceeds_the_bound_on_some_clip(fault):
    caught = []
    for name in L.ORDER:
        r = L.reference(name, 80)
        err = float(np.abs(L.emulate_f32(L.cached_signals()[name], 80, fault)[0] - r.y).max())
        print(f"{fault:14s} {name:15s} err {err:.2e}  bound {r.bound:.2e} {'*' if err > r.bound else ''}")
        if err > r.bound:
            caught.append(name)
    assert caught, fault


def test_a_maximum_shared_by_the_batch_exceeds_the_bound_on_the_quiet_clip():
    S = L.cached_signals()
    loud, quiet = L.reference(L.LOUD, 80), L.reference(L.QUIET, 80)
    shared = max(L.emulate_f32(S[L.LOUD], 80)[1], L.emulate_f32(S[L.QUIET], 80)[1])
    y_loud, _ = L.emulate_f32(S[L.LOUD], 80, shared_max=shared)
    y_quiet, _ = L.emulate_f32(S[L.QUIET], 80, shared_max=shared)
    e_loud, e_quiet = float(np.abs(y_loud - loud.y).max()), float(np.abs(y_quiet - quiet.y).max())
    print(f"shared maximum {shared:.3f}: loud err {e_loud:.2e} (bound {loud.bound:.2e})  quiet err {e_quiet:.2e} (bound {quiet.bound:.2e})")
    assert e_loud <= loud.bound and e_quiet > quiet.bound
