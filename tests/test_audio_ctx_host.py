"""CPU: the short audio context (``Whisper.audio_ctx`` -> ``wipa_model_cfg.n_audio_ctx`` = N, 1..1500) where no GPU is needed: the
native size queries accept N, grow with it, give the 30 s values at 1500 and refuse 0 and 1501; ``audio_ctx_for_seconds``; the count
of clips a context cuts; and the round trip of ``--audio-ctx`` through ``training_config.json``."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTXS = (33, 75, 256, 300, 1500)
B = 3

# name -> (cfg fields, the sizes at n_audio_ctx = 1500 as the library returned them while 1500 was the only value it accepted:
# decoder layout, teacher-forced workspace (T = 16), prompt workspace (P = 8), alignment workspace (T = 16, 4 heads), prompted-admission
# workspace (2 rows, W = 8))
MODELS = {
    "small2_bf16": (dict(d=768, H=12, dtype=1, absorbed=0), (41059840, 14708736, 954368, 24723200, 14119680)),
    "small2_bf16_absorbed": (dict(d=768, H=12, dtype=1, absorbed=1), (20989952, 14708736, 14778368, 24723200, 14119680)),
    "micro_f32": (dict(d=128, H=2, dtype=0, absorbed=0), (14049280, 4878336, 720896, 14874368, 4698880)),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    return _lib


def _cfg(_lib, n_ctx, d, H, dtype, absorbed):
    return _lib.ModelCfg(n_mels=80, n_audio_ctx=n_ctx, n_audio_state=d, n_audio_head=H, n_audio_layer=2, n_vocab=51865, n_text_ctx=448,
                         n_text_state=d, n_text_head=H, n_text_layer=2, dtype=dtype, dec_cross_absorbed=absorbed)


def _sizes(_lib, cfg):
    L = _lib.lib()
    lay = _lib.DecLayout()
    rc = L.wipa_decoder_layout(C.byref(cfg), B, C.byref(lay))
    return (L.wipa_encoder_workspace_bytes(C.byref(cfg), B), rc, lay.total_bytes if rc == 0 else 0,
            L.wipa_decoder_logits_workspace_bytes(C.byref(cfg), B, 16), L.wipa_decoder_prompt_workspace_bytes(C.byref(cfg), B, 8),
            L.wipa_decoder_align_workspace_bytes(C.byref(cfg), B, 16, 4, 0), L.wipa_decoder_admit_prompted_workspace_bytes(C.byref(cfg), 2, 8))


def _encoder_workspace_at_1500(d, e):
    """the encoder workspace of the 30 s context, restated with its literal sizes: 3002 padded frames and a 1536-key V^T row per clip"""
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    M = B * 1500
    v = B * d * 1536 * e + 256 if e == 2 else M * d * e
    return a((B * 3002 + 4) * d * e) + a(M * d * 4) + a(M * d * e) + a(M * 2 * d * e) + a(v) + a(M * d * e) + a(M * 4 * d * e)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_size_queries_accept_every_context_grow_with_it_and_keep_the_30s_values(lib, name):
    kw, at_1500 = MODELS[name]
    rows = [_sizes(lib, _cfg(lib, n, **kw)) for n in CTXS]
    for n, r in zip(CTXS, rows):
        assert r[1] == 0 and all(v > 0 for v in (r[0],) + r[2:]), (name, n, r, lib.lib().wipa_last_error())
    for lo, hi in zip(rows, rows[1:]):  # monotone in N, the encoder workspace strictly
        assert hi[0] > lo[0] and all(b >= a for a, b in zip(lo[2:], hi[2:])), (name, lo, hi)
    assert rows[-1][0] == _encoder_workspace_at_1500(kw["d"], 2 if kw["dtype"] == 1 else 4)
    assert rows[-1][2:] == at_1500, (name, rows[-1][2:], at_1500)
    # the cross-attention state is what shrinks: one copy of the features (absorbed) or K and V of both layers (cached), N rows each
    e = 2 if kw["dtype"] == 1 else 4
    per_pos = B * kw["d"] * e * (1 if kw["absorbed"] else 2 * 2)
    saved = rows[-1][2] - rows[3][2]  # 1500 -> 300
    assert saved >= 1200 * per_pos, (name, saved, per_pos)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("n_ctx", [0, 1501, -5])
def test_size_queries_refuse_a_context_outside_1_to_1500_by_name(lib, name, n_ctx):
    r = _sizes(lib, _cfg(lib, n_ctx, **MODELS[name][0]))
    assert r[1] != 0 and b"n_audio_ctx" in lib.lib().wipa_last_error() and b"1500" in lib.lib().wipa_last_error()
    assert r[0] == 0 and r[2:] == (0, 0, 0, 0, 0), r


def test_logmel_frames_workspace_query_and_padded_rows(lib):
    from whisper_ipa_amd.audio import padded_mel_rows

    L = lib.lib()
    base = L.wipa_logmel_workspace_bytes(2, 80)
    for frames in (1, 150, 600, 3000):
        assert L.wipa_logmel_frames_workspace_bytes(2, 80, frames) >= base + (2 * 3002 + 4) * 80 * 4
    assert L.wipa_logmel_frames_workspace_bytes(2, 80, 0) == 0 and L.wipa_logmel_frames_workspace_bytes(2, 80, 3001) == 0
    assert padded_mel_rows(2) == 2 * 3002 + 4 and padded_mel_rows(2, 3000) == 2 * 3002 + 4
    assert padded_mel_rows(3, 150) == 3 * 152 + 4 and padded_mel_rows(1, 600) == 606


def test_audio_ctx_for_seconds():
    from whisper_ipa_amd.audio import audio_ctx_for_seconds

    assert audio_ctx_for_seconds(6.0) == 300
    assert audio_ctx_for_seconds(30.0) == 1500
    assert audio_ctx_for_seconds(0.02) == 1 and audio_ctx_for_seconds(0.001) == 1
    assert audio_ctx_for_seconds(0.021) == 2
    assert audio_ctx_for_seconds(1.5) == 75 and audio_ctx_for_seconds(5.12) == 256 and audio_ctx_for_seconds(5.121) == 257
    for s in np.linspace(0.05, 30.0, 97):  # the smallest N whose N * 320 samples cover the clip
        n = audio_ctx_for_seconds(float(s))
        samples = int(np.ceil(s * 16000 - 1e-6))
        assert n * 320 >= samples > (n - 1) * 320, (s, n)
    for bad in (0.0, -1.0, 30.5):
        with pytest.raises(ValueError):
            audio_ctx_for_seconds(bad)


def test_over_length_count():
    from whisper_ipa_amd.audio import PcmBatch, PcmClip, count_longer_than_audio_ctx

    counts = [96000, 96001, 320, 480000, 24000, 0]
    assert count_longer_than_audio_ctx(counts, 300) == 2  # 96001 and the 30 s clip exceed 300 * 320 = 96000 samples
    assert count_longer_than_audio_ctx(counts, 75) == 3 and count_longer_than_audio_ctx(counts, 1) == 4
    assert count_longer_than_audio_ctx(counts, 1500) == 0 and count_longer_than_audio_ctx(counts, None) == 0
    # a packed batch knows its clips' lengths in 16 kHz samples, whatever their source rate: 6 s at 16 kHz, 6.5 s at 8 kHz, 1 s
    def clip(seconds, rate):
        n = int(seconds * rate)
        return PcmClip(data=np.zeros(n, dtype="<i2").tobytes(), n_frames=n, n_channels=1, width=2, rate=rate)

    batch = PcmBatch([clip(6.0, 16000), clip(6.5, 8000), clip(1.0, 16000)], pin=False)
    assert batch.sample_counts() == [96000, 104000, 16000]
    assert count_longer_than_audio_ctx(batch.sample_counts(), 300) == 1
    assert count_longer_than_audio_ctx(batch.sample_counts(), 50) == 2


def test_audio_ctx_round_trip_through_training_config(tmp_path):
    """train_whisper_ipa.py records --audio-ctx in training_config.json (training_args.audio_ctx); the evaluation scripts read it back
    from the checkpoint's run directory: no request -> the recorded value; another value -> that value and one warning line"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_whisper_ipa as T

    from whisper_ipa_amd.load_models import resolve_audio_ctx, trained_audio_ctx

    run = tmp_path / "run"
    (run / "checkpoint-10").mkdir(parents=True)
    T.save_training_config(run, {"model_name": "m", "num_steps": 10, "audio_ctx": 300}, {"gpu": "none"})
    assert json.load(open(run / "training_config.json"))["training_args"]["audio_ctx"] == 300
    for ckpt in (run / "checkpoint-10", run):  # the file lies beside the checkpoint directories
        assert trained_audio_ctx(str(ckpt)) == (True, 300)
        assert resolve_audio_ctx(None, str(ckpt)) == (300, None)
        assert resolve_audio_ctx(300, str(ckpt)) == (300, None)
        n, warning = resolve_audio_ctx(750, str(ckpt))
        assert n == 750 and warning and "\n" not in warning and "750" in warning and "300" in warning and "audio_ctx" in warning
    # a run without the setting (or from before it existed): the 30 s context, and a request for a short one is warned about
    old = tmp_path / "old"
    (old / "best-checkpoint").mkdir(parents=True)
    T.save_training_config(old, {"model_name": "m", "num_steps": 10}, {})
    assert trained_audio_ctx(str(old / "best-checkpoint")) == (True, None)
    assert resolve_audio_ctx(None, str(old / "best-checkpoint")) == (None, None)
    n, warning = resolve_audio_ctx(300, str(old / "best-checkpoint"))
    assert n == 300 and warning and "300" in warning
    # no training_config.json at all: nothing to compare with
    assert trained_audio_ctx(str(tmp_path / "nowhere" / "checkpoint-1")) == (False, None)
    assert resolve_audio_ctx(75, str(tmp_path / "nowhere" / "checkpoint-1")) == (75, None)
    assert resolve_audio_ctx(None, None) == (None, None)
    # the three scripts take --audio-ctx, default none
    for script in ("train_whisper_ipa.py", "evaluate_model.py", "transcribe_single.py"):
        src = open(os.path.join(ROOT, "scripts", script)).read()
        assert '"--audio-ctx", type=int, default=None' in src, script
