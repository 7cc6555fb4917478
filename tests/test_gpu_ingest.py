"""GPU: device-side audio ingest (csrc/resample.hip through audio.load_audio_batch and the C ABI) against the host path
``pad_or_trim(load_audio(file))``.  ``pytest -m gpu`` on an MI355X.

Tolerance for resampled clips: the kernel sums 2K+1 f32 products of an f32-rounded table in order, the host the same terms in
float64 -- the classical bound of such a sum, (2K+1 + 2) * 2^-24 * max_p sum_k |T[p][k]| * max|x| (one unit for the table's
rounding, one for the result's), computed here from the table: 0.5e-5 .. 1.1e-5 at these rates.  A wrong phase or a tap off by
one gives errors above 1e-2 on this input (full-scale noise).  16 kHz input must be bit-identical."""
import gc
import os
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 480000
FMT = {1: np.uint8, 2: "<i2", 4: "<i4"}


def write_wav(path, rate, width, n_ch, n_frames, seed):
    """full-scale uniform noise in the file's own sample format"""
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if width == 1 else (-(1 << (8 * width - 1)), 1 << (8 * width - 1))
    pcm = rng.integers(lo, hi, n_frames * n_ch, dtype=np.int64).astype(FMT[width])
    with wave.open(str(path), "wb") as w:
        w.setnchannels(n_ch)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return str(path)


def host(path):
    from whisper_ipa_amd import audio as A

    return np.asarray(A.pad_or_trim(A.load_audio(path)), dtype=np.float32)


def bound(rate, peak=1.0):
    from whisper_ipa_amd import audio as A

    S, D, K, T = A.resample_table(rate)
    return (2 * K + 1 + 2) * 2.0 ** -24 * float(np.abs(T.astype(np.float32)).sum(axis=1).max()) * peak


def device(paths_or_batch):
    """load_audio_batch into a NaN-filled output: every element must have been written"""
    from whisper_ipa_amd import audio as A

    batch = paths_or_batch if isinstance(paths_or_batch, A.PcmBatch) else A.PcmBatch(paths_or_batch)
    out = torch.full((len(batch), N), float("nan"), dtype=torch.float32, device="cuda")
    got = A.load_audio_batch(batch, out=out)
    assert got.data_ptr() == out.data_ptr()
    y = got.cpu().numpy()
    assert np.isfinite(y).all()
    return y


RATES = (8000, 22050, 44100, 48000)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """every WAV the array tests read, with its host reference, made once"""
    from whisper_ipa_amd import audio as A

    d = tmp_path_factory.mktemp("ingest")
    f = {}
    for name, (rate, width, n_ch, n) in {
        "s16_mono": (16000, 2, 1, 3301), "s16_stereo": (16000, 2, 2, 2207), "u8_mono": (16000, 1, 1, 1999), "s32_mono": (16000, 4, 1, 1603),
        # 0.1 - 0.3 s at every rate, mono and stereo
        **{f"r{r}_{c}": (r, 2, c, int(r * (0.1 + 0.05 * i)) + 3) for i, r in enumerate(RATES) for c in (1, 2)},
        "tile_48k": (48000, 2, 1, 3 * 512 + 1),   # n_out = 513: one output into the second tile
        "tile_44k": (44100, 2, 2, 2823),          # n_out = 1025: one output into the third tile
        "short": (44100, 2, 1, 20),               # fewer frames than K = 45
        "empty": (44100, 2, 1, 0),
    }.items():
        p = write_wav(d / f"{name}.wav", rate, width, n_ch, n, seed=len(f) + 1)
        S, D, _, _ = A.resample_table(rate)
        f[name] = (p, rate, host(p), -(-n * D // S))
    return f


@pytest.mark.parametrize("name", ["s16_mono", "s16_stereo", "u8_mono", "s32_mono"])
def test_16khz_formats_are_bit_exact(files, name):
    path, _, ref, _ = files[name]
    got = device([path])
    assert got.shape == (1, N) and np.array_equal(got[0].view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", [f"r{r}_{c}" for r in RATES for c in (1, 2)])
def test_rates_within_the_f32_bound(files, name):
    path, rate, ref, n_out = files[name]
    got = device([path])[0]
    err, tol = float(np.abs(got - ref).max()), bound(rate)
    print(f"{name}: max err {err:.3e}  bound {tol:.3e}")
    assert tol < 1.2e-5 and err <= tol
    assert np.abs(ref[:n_out]).max() > 0.1 and not got[n_out:].any()  # pad_or_trim's zeros start where the host's do


def test_mixed_batch_and_edges(files):
    """every rate, format and channel count in ONE batch beside full-scale neighbours; n_out one past a tile boundary; a clip
    shorter than the filter; an empty clip between two loud ones (its row must be all zeros)"""
    names = ["r44100_2", "s16_stereo", "tile_48k", "empty", "r8000_1", "u8_mono", "short", "r22050_2", "tile_44k", "s32_mono",
             "r48000_1", "r44100_1", "r8000_2", "s16_mono", "r22050_1", "r48000_2"]
    got = device([files[n][0] for n in names])
    for row, n in zip(got, names):
        _, rate, ref, _ = files[n]
        if rate == 16000:
            assert np.array_equal(row.view(np.uint32), ref.view(np.uint32)), n
        else:
            err = float(np.abs(row - ref).max())
            print(f"{n}: max err {err:.3e}  bound {bound(rate):.3e}")
            assert err <= bound(rate), n
    assert not got[names.index("empty")].any()
    from whisper_ipa_amd import audio as A

    assert files["tile_48k"][3] == A.RESAMPLE_TILE + 1 and files["tile_44k"][3] == 2 * A.RESAMPLE_TILE + 1
    for n, last in (("tile_48k", 512), ("tile_44k", 1024)):  # the lone output of the last tile is there, nothing after it
        assert files[n][2][last] != 0 and got[names.index(n)][last] != 0 and not got[names.index(n)][last + 1:].any()
    assert files["short"][3] == 8 and got[names.index("short")][:8].all()


def test_position_past_2_31(tmp_path):
    """44 099 Hz is 44099 / 16000 in lowest terms: m * S passes 2^31 after m = 48 696; 3.2 s reaches m = 51 200"""
    p = write_wav(tmp_path / "odd.wav", 44099, 2, 1, int(3.2 * 44099), seed=11)
    ref = host(p)
    got = device([p])[0]
    n_out = -(-int(3.2 * 44099) * 16000 // 44099)
    assert n_out > 48696 + 1000 and (n_out - 1) * 44099 > 2 ** 31
    err_tail = float(np.abs(got[n_out - 1000: n_out] - ref[n_out - 1000: n_out]).max())
    err = float(np.abs(got - ref).max())
    print(f"44099 Hz: max err {err:.3e} (last 1000: {err_tail:.3e})  bound {bound(44099):.3e}")
    assert err_tail <= bound(44099) and err <= bound(44099)
    assert np.abs(ref[n_out - 1000: n_out]).max() > 0.1


def test_trim_resamples_then_cuts(tmp_path):
    """8 kHz, 30.5 s: exactly 480 000 outputs, and the last of them still see input past the 30 s mark, as the host's
    resample-then-trim does"""
    from whisper_ipa_amd import audio as A

    n = int(30.5 * 8000)
    p = write_wav(tmp_path / "long.wav", 8000, 2, 1, n, seed=12)
    clip = A.read_pcm(p)
    assert clip.n_frames == A.pcm_frame_cap(8000) == 240017 and clip.total_frames == n
    ref = A.load_audio(p)
    assert len(ref) == 2 * n
    got = device(A.PcmBatch([clip]))
    assert got.shape == (1, N)
    err = float(np.abs(got[0] - ref[:N]).max())
    print(f"8000 Hz trim: max err {err:.3e}  bound {bound(8000):.3e}")
    assert err <= bound(8000)
    # cutting the INPUT at 30 s first would change the last outputs by far more than the bound
    x = np.frombuffer(clip.data, dtype="<i2").astype(np.float32) / 32768.0
    S, D, K, T = A.resample_table(8000)
    m = np.arange(N - 8, N)
    q, ph = (m * S) // D, (m * S) % D
    idx = q[:, None] + np.arange(-K, K + 1)[None, :]
    cut_first = (T[ph] * np.where(idx < 240000, x[np.minimum(idx, len(x) - 1)], 0.0)).sum(axis=1)
    assert np.abs(cut_first - ref[N - 8: N]).max() > 100 * bound(8000)


def test_entry_point_refuses_an_unsupported_rate():
    """3 999 Hz through the C ABI: an error code and a message, nothing launched"""
    import ctypes as C

    from whisper_ipa_amd import _lib

    lib = _lib.lib()
    d = (_lib.PcmClipDesc * 1)()
    d[0].byte_offset, d[0].table_offset, d[0].n_frames, d[0].n_out = 0, 0, 0, 0
    d[0].n_channels, d[0].format, d[0].rate, d[0].S, d[0].D, d[0].K = 1, 2, 3999, 3999, 16000, 16
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, N, device="cuda")
    rc = lib.wipa_resample_pad(buf.data_ptr(), 1024, buf.data_ptr(), d, 1, out.data_ptr(), 256, out.data_ptr(), None)
    assert rc == -1 and b"3999 Hz" in lib.wipa_last_error()
    d[0].rate, d[0].S = 192001, 192001
    rc = lib.wipa_resample_pad(buf.data_ptr(), 1024, buf.data_ptr(), d, 1, out.data_ptr(), 256, out.data_ptr(), None)
    assert rc == -1 and b"192001 Hz" in lib.wipa_last_error()
    d[0].rate, d[0].S, d[0].D, d[0].K, d[0].n_frames = 16000, 1, 1, 0, 1000  # 2000 bytes in a 1024-byte buffer
    rc = lib.wipa_resample_pad(buf.data_ptr(), 1024, buf.data_ptr(), d, 1, out.data_ptr(), 256, out.data_ptr(), None)
    assert rc == -1 and b"outside the 1024-byte buffer" in lib.wipa_last_error()
    torch.cuda.synchronize()


# ---- through the pipeline and the evaluation script ------------------------------------------------------------------------------

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)


@pytest.fixture(scope="module")
def micro_model():
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=torch.float32)
    m.load_weights(R.synthetic_weights(MICRO, seed=7))
    return m


@pytest.fixture(scope="module")
def speech_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("clips16k")
    paths = []
    for i in range(6):
        a = R.synthetic_clip(i, 0.4 + 0.3 * i)
        pcm = np.clip(np.round(a * 32767.0), -32768, 32767).astype("<i2")
        p = d / f"c{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
        paths.append(str(p))
    return paths


def test_pipeline_takes_pcm_batches_from_a_generator(micro_model, speech_files):
    """transcribe_batches fed PcmBatches by a generator that keeps no batch alive, two passes in flight: the ids are those of
    the host-loaded arrays"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import audio as A

    opts = wipa.DecodingOptions(language="en", without_timestamps=True, fp16=False)
    groups = [speech_files[0:2], speech_files[2:4], speech_files[4:6]]
    want = [r.tokens for r in wipa.transcribe_batches(micro_model, [torch.from_numpy(np.stack([host(p) for p in g])) for g in groups],
                                                       opts, passes_in_flight=2, max_new_tokens=6, stop_on_eot=False)]

    def gen():
        for i, g in enumerate(groups):
            yield A.PcmBatch(g) if i != 1 else {"pcm": A.PcmBatch(g)}
            gc.collect()  # nothing here holds the batch any more

    got = [r.tokens for r in wipa.transcribe_batches(micro_model, gen(), opts, passes_in_flight=2, max_new_tokens=6, stop_on_eot=False)]
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert a.shape == (2, 4 + 6) and np.array_equal(a, b)


def test_evaluate_model_ingest_modes_agree(micro_model, speech_files, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import evaluate_model as EM

    opts = EM.DecodingOptions(language="en", without_timestamps=True, sample_len=8)
    paths = speech_files[:3] + [str(tmp_path / "missing.wav")] + speech_files[3:5]
    dev = EM.transcribe_clips(micro_model, paths, opts, batch_size=2, passes_in_flight=2, ingest="device")
    hst = EM.transcribe_clips(micro_model, paths, opts, batch_size=2, passes_in_flight=2, ingest="host")
    assert dev == hst and len(dev) == 6 and dev[3] == ""
    assert capsys.readouterr().out.count("Error transcribing") == 2
    with pytest.raises(ValueError):
        EM.load_clips(paths[:1], ingest="gpu")
