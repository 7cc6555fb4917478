"""CPU: the host side of the device audio ingest (whisper_ipa_amd.audio) -- the polyphase table that restates ``_resample``,
``read_pcm`` and the packing of a ``PcmBatch``.  No GPU, no library call."""
import ctypes as C
import wave

import numpy as np
import pytest

from whisper_ipa_amd import _lib
from whisper_ipa_amd import audio as A


def apply_table(x, src, dst=16000):
    """y[m] = sum_k T[p][k+K] x[q+k] with q = (m S) div D, p = (m S) mod D in integers, zeros outside the clip, float64 sums"""
    S, D, K, T = A.resample_table(src, dst)
    n_out = -(-len(x) * D // S)
    m = np.arange(n_out, dtype=np.int64)
    q, p = (m * S) // D, (m * S) % D
    idx = q[:, None] + np.arange(-K, K + 1, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    xs = np.where(ok, np.asarray(x, dtype=np.float64)[np.clip(idx, 0, len(x) - 1)], 0.0)
    return (T[p].astype(np.float64) * xs).sum(axis=1)


@pytest.mark.parametrize("src", [8000, 11025, 22050, 44100, 48000, 44099])
def test_resample_table_restates_resample(src):
    """0.1 s of uniform noise: the table form, summed in float64 and rounded to f32 as ``_resample`` rounds its own float64
    sums, is ``_resample`` to 1e-9 (what is left is the float rounding of the position m * (src / dst) against the exact p / D)."""
    x = np.random.default_rng(src).uniform(-1.0, 1.0, src // 10).astype(np.float32)
    ref = A._resample(x, src, 16000)
    y = apply_table(x, src)
    assert y.shape == ref.shape
    err = np.abs(y.astype(np.float32).astype(np.float64) - ref.astype(np.float64)).max()
    print(f"{src} Hz: max |table - _resample| = {err:.3e}")
    assert err <= 1e-9


def test_resample_table_shapes_and_identity():
    S, D, K, T = A.resample_table(16000)
    assert (S, D, K) == (1, 1, 0) and T.tolist() == [[1.0]]
    for src, shape in ((44100, (160, 91)), (48000, (1, 97)), (22050, (320, 47)), (44099, (16000, 91))):
        S, D, K, T = A.resample_table(src)
        assert T.shape == shape == (D, 2 * K + 1) and S * 16000 == D * src
    assert A.pcm_frame_cap(16000) == 480001 and A.pcm_frame_cap(8000) == 240000 + 16 + 1
    assert A.pcm_frame_cap(44100) == 1323000 + 45 + 1


def _clip(n_frames, n_ch, width, rate, seed=0, total=None):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, n_frames * n_ch * width, dtype=np.uint8).tobytes()
    return A.PcmClip(data, n_frames, n_ch, width, rate, total)


def test_pcm_batch_packing():
    """offsets, alignment, the per-clip frame cap, mixed widths and channel counts, a zero-length clip, shared tables"""
    cap8k = A.pcm_frame_cap(8000)
    clips = [_clip(1601, 1, 2, 16000, 1), _clip(333, 2, 1, 44100, 2), _clip(0, 1, 2, 48000, 3), _clip(77, 2, 4, 44100, 4),
             _clip(cap8k + 500, 1, 1, 8000, 5), _clip(100, 1, 2, 22050, 6, total=5000)]
    b = A.PcmBatch(clips, pin=False)
    assert len(b) == 6 and b.buffer.dtype.is_floating_point is False and b.buffer.numel() == b.nbytes
    raw = b.buffer.numpy()
    descs = (_lib.PcmClipDesc * 6).from_buffer_copy(raw[: 6 * C.sizeof(_lib.PcmClipDesc)].tobytes())
    end = 6 * C.sizeof(_lib.PcmClipDesc)
    for d, h, c in zip(descs, b.descs, clips):
        assert all(getattr(d, f) == getattr(h, f) for f, _ in _lib.PcmClipDesc._fields_)  # the buffer carries the descriptors
        assert d.byte_offset % 16 == 0 and d.byte_offset >= end  # no overlap with the previous clip or the descriptors
        assert (d.n_channels, d.format, d.rate) == (c.n_channels, c.width, c.rate)
        S, D, K, T = A.resample_table(c.rate)
        assert (d.S, d.D, d.K) == (S, D, K)
        n = d.n_frames * c.n_channels * c.width
        assert raw[d.byte_offset: d.byte_offset + n].tobytes() == c.data[:n]
        end = d.byte_offset + n
        assert d.table_offset % 4 == 0 and d.table_offset + T.size <= b.table_floats
    assert end <= b.nbytes
    assert [d.n_frames for d in descs] == [1601, 333, 0, 77, cap8k, 100]  # the 8 kHz clip is cut to what 30 s can touch
    assert descs[0].n_out == 1601 and descs[1].n_out == -(-333 * 160 // 441) and descs[2].n_out == 0
    assert descs[4].n_out == 480000  # longer than 30 s: trimmed
    assert descs[5].n_out == -(-5000 * 320 // 441)  # the head of a longer clip: its end is where the whole clip ends
    assert b.rates == [16000, 44100, 48000, 8000, 22050]
    assert descs[1].table_offset == descs[3].table_offset == b.table_offsets[1] == 4  # after the identity table, rounded to 4
    assert b.table_offsets[2] == 4 + 160 * 91 and b.table_floats == b.table_offsets[4] + 320 * 47


def test_pcm_batch_refuses_what_the_kernel_does_not_take():
    with pytest.raises(ValueError):
        A.PcmBatch([], pin=False)
    for bad in (_clip(10, 1, 3, 16000), _clip(10, 1, 2, 3999), _clip(10, 1, 2, 192001), _clip(10, 9, 2, 16000),
                A.PcmClip(b"\0" * 10, 10, 1, 2, 16000)):
        with pytest.raises(ValueError):
            A.PcmBatch([bad], pin=False)
    A.PcmBatch([_clip(10, 1, 2, 4000), _clip(10, 8, 2, 192000)], pin=False)


def test_read_pcm_reads_header_and_raw_frames(tmp_path):
    pcm = np.random.default_rng(0).integers(-32768, 32768, 2 * 700, dtype=np.int16)
    p = tmp_path / "a.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100); w.writeframes(pcm.astype("<i2").tobytes())
    c = A.read_pcm(str(p))
    assert (c.n_frames, c.n_channels, c.width, c.rate, c.total_frames) == (700, 2, 2, 44100, 700)
    assert c.data == pcm.astype("<i2").tobytes()
    long = tmp_path / "long.wav"   # 8 kHz u8, 31 s: only the frames the 30 s window can touch are read
    with wave.open(str(long), "wb") as w:
        w.setnchannels(1); w.setsampwidth(1); w.setframerate(8000); w.writeframes(bytes(8000 * 31))
    c = A.read_pcm(str(long))
    assert c.n_frames == A.pcm_frame_cap(8000) == len(c.data) and c.total_frames == 8000 * 31
    odd = tmp_path / "odd.wav"
    with wave.open(str(odd), "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(16000); w.writeframes(bytes(30))
    with pytest.raises(ValueError):
        A.read_pcm(str(odd))


def test_descriptor_layout_matches_c(tmp_path):
    """the ctypes mirror of wipa_pcm_clip against the compiler's layout"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = tmp_path / "lay.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wipa.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", '
                    "sizeof(wipa_pcm_clip), offsetof(wipa_pcm_clip, table_offset), offsetof(wipa_pcm_clip, n_frames), "
                    "offsetof(wipa_pcm_clip, format), offsetof(wipa_pcm_clip, K), WIPA_RESAMPLE_TILE);return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    D = _lib.PcmClipDesc
    assert got == [C.sizeof(D), D.table_offset.offset, D.n_frames.offset, D.format.offset, D.K.offset, _lib.RESAMPLE_TILE]
    assert A.RESAMPLE_TILE == _lib.RESAMPLE_TILE
