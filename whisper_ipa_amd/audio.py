"""Audio front-end with the call surface of ``mlx_whisper.audio`` used by the reference
(scripts/ipa_data_loader.py:14,48,80-82; scripts/transcribe_single.py:6,43-45):
``load_audio``, ``pad_or_trim``, ``log_mel_spectrogram`` and the constants.

``log_mel_spectrogram`` runs on the GPU (K1, csrc/logmel.hip).  ``load_audio`` reads WAV
files directly: the reference shells out to ffmpeg, which this image does not have.

``load_audio_batch`` is ``pad_or_trim(load_audio(file))`` for a batch of files on the GPU (K0, csrc/resample.hip): the host only
reads the PCM bytes (``read_pcm``) and packs them (``PcmBatch``); sample conversion, channel mix-down, resampling to 16 kHz and the
30 s pad / cut are one copy and one launch.  ``load_audio`` / ``_resample`` stay as the host path and as the kernel's reference.

``SpecAugment`` / ``spec_augment``: time and mel-bin masks for fine-tuning, drawn per clip from a counter-based generator and stored
into an f32 mel on the GPU (csrc/spec_augment.hip).  Training only: nothing on the inference path calls it.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import wave
from collections import OrderedDict
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .runtime import device, dt_code, on_stream, ptr, sptr, stream_id

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE
N_FRAMES = N_SAMPLES // HOP_LENGTH
PADDED_FRAMES = N_FRAMES + 2  # one zero halo row either side (conv1 padding=1)

ArrayLike = Union[np.ndarray, torch.Tensor]


def load_audio(file: str, sr: int = SAMPLE_RATE) -> np.ndarray:
    """Decode a PCM WAV file to mono float32 in [-1, 1) at ``sr`` Hz (s16 -> /32768 like the
    reference's ffmpeg pipe).  Other containers need an external decoder."""
    with wave.open(file, "rb") as w:
        n_ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f"unsupported WAV sample width {width}")
    if n_ch > 1:
        a = a.reshape(-1, n_ch).mean(axis=1)
    if rate != sr:
        a = _resample(a, rate, sr)
    return np.ascontiguousarray(a, dtype=np.float32)


def _sinc_window(dt: np.ndarray, cutoff: float, half: float) -> np.ndarray:
    """weight of a tap ``dt`` input samples away from the output position: the low-pass sinc at ``cutoff`` (of the input Nyquist)
    under a Hann window of half-width ``half`` -- the one spelling ``_resample`` and ``resample_table`` share"""
    return cutoff * np.sinc(cutoff * dt) * (0.5 + 0.5 * np.cos(np.pi * np.clip(dt / half, -1.0, 1.0)))


def _resample(a: np.ndarray, src: int, dst: int, zero_crossings: int = 16) -> np.ndarray:
    """Windowed-sinc (Hann, ``zero_crossings`` lobes each side) resampling, evaluated per OUTPUT sample -- the polyphase
    form: output m sits at input position m*src/dst and sums the 2*zero_crossings/cutoff input samples around it, so the work
    is n_out x taps whatever the ratio (44.1 kHz -> 16 kHz is up 160 / down 441: the zero-stuffed form would convolve
    211 M samples with a 14 k-tap filter).  Host side, numpy, chunked to bound memory."""
    n_in = len(a)
    n_out = int(np.ceil(n_in * dst / src))
    if n_in == 0 or n_out == 0:
        return np.zeros(0, dtype=np.float32)
    cutoff = min(1.0, dst / src)              # of the input Nyquist: low-pass at the lower of the two rates
    half = zero_crossings / cutoff            # filter half-width in input samples
    k = np.arange(-int(np.ceil(half)), int(np.ceil(half)) + 1)
    x = np.asarray(a, dtype=np.float64)
    y = np.empty(n_out, dtype=np.float64)
    step = max(1, (1 << 22) // len(k))        # ~32 MB of float64 per chunk
    for m0 in range(0, n_out, step):
        m = np.arange(m0, min(m0 + step, n_out))
        pos = m * (src / dst)
        base = np.floor(pos).astype(np.int64)
        idx = base[:, None] + k[None, :]
        dt = pos[:, None] - idx                # distance of every tap from the output position, in input samples
        w = _sinc_window(dt, cutoff, half)
        ok = (idx >= 0) & (idx < n_in)
        y[m] = (w * np.where(ok, x[np.clip(idx, 0, n_in - 1)], 0.0)).sum(axis=1)
    return y.astype(np.float32)


def pad_or_trim(array: ArrayLike, length: int = N_SAMPLES, axis: int = -1) -> ArrayLike:
    """Zero-pad or cut ``axis`` to ``length`` (ipa_data_loader.py:80)."""
    if isinstance(array, torch.Tensor):
        n = array.shape[axis]
        if n > length:
            array = array.narrow(axis, 0, length)
        elif n < length:
            pad = [0, 0] * array.ndim
            pad[2 * (array.ndim - 1 - (axis % array.ndim)) + 1] = length - n
            array = torch.nn.functional.pad(array, pad)
        return array
    array = np.asarray(array)
    n = array.shape[axis]
    if n > length:
        array = array.take(indices=range(length), axis=axis)
    elif n < length:
        widths = [(0, 0)] * array.ndim
        widths[axis] = (0, length - n)
        array = np.pad(array, widths)
    return array


# ---- device-side ingest (K0, csrc/resample.hip): raw PCM -> [B, 480000] f32 at 16 kHz on the GPU ---------------------------------

MIN_RATE, MAX_RATE = 4000, 192000     # source rates wipa_resample_pad accepts
RESAMPLE_TILE = _lib.RESAMPLE_TILE    # consecutive outputs per workgroup (WIPA_RESAMPLE_TILE)
TABLE_CACHE_ENTRIES = 8               # resampling tables kept per process (44 099 Hz -> 16 kHz is 5.8 MB; common rates are KBs)


def _resample_geometry(src: int, dst: int = SAMPLE_RATE, zero_crossings: int = 16) -> Tuple[int, int, int]:
    """(S, D, K): src / dst in lowest terms and the filter half-width in input samples, as ``_resample`` takes it"""
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError(f"sample rates must be positive, got {src} -> {dst}")
    g = math.gcd(src, dst)
    if src == dst:
        return 1, 1, 0
    half = zero_crossings / min(1.0, dst / src)
    return src // g, dst // g, int(np.ceil(half))


def resample_table(src: int, dst: int = SAMPLE_RATE) -> Tuple[int, int, int, np.ndarray]:
    """``_resample`` as an exact polyphase table.  Output m sits at input position m S / D (S / D = src / dst in lowest terms):
    with q = (m S) div D and p = (m S) mod D,  y[m] = sum_{k=-K..K} T[p][k + K] x[q + k]  (x = 0 outside the clip).
    Returns (S, D, K, T [D, 2K+1]) with T in float64, as ``_resample`` evaluates it; the device copy is T rounded once to f32.
    src == dst is (1, 1, 0, [[1.0]]).  Host only."""
    S, D, K = _resample_geometry(src, dst)
    if K == 0:
        return S, D, K, np.ones((1, 1), dtype=np.float64)
    cutoff = min(1.0, dst / src)
    half = 16 / cutoff
    dt = np.arange(D, dtype=np.float64)[:, None] / D - np.arange(-K, K + 1, dtype=np.float64)[None, :]
    return S, D, K, _sinc_window(dt, cutoff, half)


def pcm_frame_cap(rate: int, sr: int = SAMPLE_RATE) -> int:
    """frames of a clip at ``rate`` Hz that the 30 s output window can touch: the last output sits at input position
    479 999 S / D and reaches K frames further"""
    S, D, K = _resample_geometry(rate, sr)
    return -(-N_SAMPLES * S // D) + K + 1


@dataclass
class PcmClip:
    """The PCM of one file as stored: ``data`` holds ``n_frames`` interleaved frames of ``n_channels`` samples of ``width`` bytes
    (1: unsigned, 2 / 4: signed little-endian) at ``rate`` Hz.  ``total_frames``: frames of the whole clip when ``data`` is only
    its head (None: ``n_frames``) -- it sets where the resampled clip ends."""
    data: bytes
    n_frames: int
    n_channels: int
    width: int
    rate: int
    total_frames: Optional[int] = None


def _check_pcm_format(n_channels: int, width: int, rate: int) -> None:
    if width not in (1, 2, 4):
        raise ValueError(f"unsupported WAV sample width {width}")
    if not 1 <= n_channels <= 8:
        raise ValueError(f"unsupported channel count {n_channels} (1..8)")
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"unsupported sample rate {rate} Hz ({MIN_RATE}..{MAX_RATE} Hz)")


def read_pcm(file: str, sr: int = SAMPLE_RATE) -> PcmClip:
    """The header and the raw frames of a PCM WAV file, unconverted; no more frames than the 30 s window can touch
    (``pcm_frame_cap``).  Host only."""
    with wave.open(file, "rb") as w:
        n_ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        _check_pcm_format(n_ch, width, rate)
        cap = pcm_frame_cap(rate, sr)
        raw = w.readframes(min(n, cap))
    got = len(raw) // (n_ch * width)
    return PcmClip(raw, got, n_ch, width, rate, total_frames=n if (n > cap and got == cap) else got)


class PcmBatch:
    """Clips packed for ONE host-to-device copy: ``buffer`` (uint8, pinned when a GPU is present) = the ``wipa_pcm_clip``
    descriptors, then every clip's bytes (16-byte aligned, cut to ``pcm_frame_cap`` frames).  ``rates`` lists the distinct source
    rates in order of first appearance; their tables are expected back to back (each start rounded up to 4 floats) in that
    order -- ``table_offsets`` -- which is how ``load_audio_batch`` lays them out.  Host only: no GPU work happens here."""

    ALIGN = 16

    def __init__(self, clips: Iterable[Union[str, "os.PathLike", PcmClip]], sr: int = SAMPLE_RATE, pin: Optional[bool] = None):
        if sr != SAMPLE_RATE:
            raise ValueError(f"the device path resamples to {SAMPLE_RATE} Hz")
        clips = [c if isinstance(c, PcmClip) else read_pcm(os.fspath(c), sr) for c in clips]
        if not clips:
            raise ValueError("PcmBatch needs at least one clip")
        self.B = len(clips)
        self.descs = (_lib.PcmClipDesc * self.B)()
        self.rates: List[int] = []
        self.table_offsets: List[int] = []
        self.table_floats = 0
        off = -(-C.sizeof(self.descs) // 256) * 256
        for d, c in zip(self.descs, clips):
            _check_pcm_format(c.n_channels, c.width, c.rate)
            frame = c.n_channels * c.width
            if c.n_frames < 0 or len(c.data) < c.n_frames * frame:
                raise ValueError(f"PcmClip holds {len(c.data)} bytes, fewer than its {c.n_frames} frames of {frame}")
            S, D, K = _resample_geometry(c.rate, sr)
            if c.rate not in self.rates:
                self.rates.append(c.rate)
                self.table_offsets.append(self.table_floats)
                self.table_floats += -(-D * (2 * K + 1) // 4) * 4
            total = c.n_frames if c.total_frames is None else max(int(c.total_frames), c.n_frames)
            d.byte_offset, d.table_offset = off, self.table_offsets[self.rates.index(c.rate)]
            d.n_frames = min(c.n_frames, pcm_frame_cap(c.rate, sr))
            d.n_out = min(N_SAMPLES, -(-total * D // S))
            d.n_channels, d.format, d.rate, d.S, d.D, d.K = c.n_channels, c.width, c.rate, S, D, K
            off += -(-d.n_frames * frame // self.ALIGN) * self.ALIGN
        self.nbytes = max(off, self.ALIGN)
        pin = torch.cuda.is_available() if pin is None else pin
        self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=bool(pin))
        view = self.buffer.numpy()
        view[: C.sizeof(self.descs)] = np.frombuffer(self.descs, dtype=np.uint8)
        for d, c in zip(self.descs, clips):
            n = d.n_frames * c.n_channels * c.width
            view[d.byte_offset: d.byte_offset + n] = np.frombuffer(c.data, dtype=np.uint8, count=n)

    def __len__(self) -> int:
        return self.B

    def sample_counts(self) -> List[int]:
        """every clip's length in 16 kHz samples, capped at the 30 s window"""
        return [int(d.n_out) for d in self.descs]


_resample_tables: "OrderedDict" = OrderedDict()   # (device index, src, dst) -> device table; small LRU
_table_sets: "OrderedDict" = OrderedDict()        # (device index, rates) -> (concatenated tables, the single tables it was built from)


def _device_table(dev: torch.device, src: int, dst: int = SAMPLE_RATE) -> torch.Tensor:
    """the table of one rate on the device, built on the host once per (device, src, dst) and kept in an LRU"""
    key = (dev.index, int(src), int(dst))
    t = _resample_tables.get(key)
    if t is not None:
        _resample_tables.move_to_end(key)
        return t
    T = resample_table(src, dst)[3]
    t = torch.from_numpy(T.astype(np.float32).reshape(-1)).to(dev)
    torch.cuda.current_stream().synchronize()  # once per rate: other library streams read it without ordering against this one
    _resample_tables[key] = t
    if len(_resample_tables) > TABLE_CACHE_ENTRIES:
        torch.cuda.synchronize(dev)  # a launch on another stream may still read what is dropped
        old, _ = _resample_tables.popitem(last=False)
        for k in [k for k in _table_sets if k[0] == old[0] and old[1] in k[1]]:
            del _table_sets[k]
    return t


def _tables_for(dev: torch.device, batch: PcmBatch) -> torch.Tensor:
    """the batch's tables as one buffer laid out as its descriptors say (``PcmBatch.table_offsets``)"""
    if len(batch.rates) == 1:
        return _device_table(dev, batch.rates[0])
    key = (dev.index, tuple(batch.rates))
    hit = _table_sets.get(key)
    if hit is not None:
        _table_sets.move_to_end(key)
        return hit
    buf = torch.zeros(batch.table_floats, dtype=torch.float32, device=dev)
    for rate, off in zip(batch.rates, batch.table_offsets):
        t = _device_table(dev, rate)
        buf[off: off + t.numel()].copy_(t)
    torch.cuda.current_stream().synchronize()
    _table_sets[key] = buf
    if len(_table_sets) > TABLE_CACHE_ENTRIES:
        torch.cuda.synchronize(dev)
        _table_sets.popitem(last=False)
    return buf


def _ingest(batch: PcmBatch, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, tuple]:
    """copy + launch on the current library stream; returns (audio, what must stay alive until the launch has run)"""
    L = _lib.lib()
    dev = device()
    with on_stream() as s:
        tables = _tables_for(dev, batch)
        pcm = torch.empty(batch.nbytes, dtype=torch.uint8, device=dev)
        pcm.copy_(batch.buffer, non_blocking=True)  # descriptors and samples: one copy
        if out is None:
            out = torch.empty(batch.B, N_SAMPLES, dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (batch.B, N_SAMPLES) and out.is_contiguous()
        _lib.check(L.wipa_resample_pad(ptr(pcm), batch.nbytes, ptr(pcm), batch.descs, batch.B, ptr(tables), tables.numel(), ptr(out),
                                       sptr(s)), "wipa_resample_pad")
    return out, (batch, pcm, tables)


def load_audio_batch(clips: Union[PcmBatch, Sequence[Union[str, PcmClip]]], out: Optional[torch.Tensor] = None,
                     audio_ctx: Optional[int] = None, report: Optional[dict] = None) -> torch.Tensor:
    """``pad_or_trim(load_audio(file))`` for a batch, on the GPU: files (PCM WAV), ``PcmClip``s or a ``PcmBatch`` ->
    audio [B, 480000] f32 on the device.  One host-to-device copy and one launch (csrc/resample.hip) on the current library
    stream; 16 kHz input is bit-identical to the host path, other rates agree to f32 rounding of the same filter.
    ``out``: an existing [B, 480000] f32 device tensor to write into (every element is written).
    ``report`` (a dict): receives ``"longer_than_audio_ctx"``, the clips of the batch that exceed ``audio_ctx`` * 320 samples and are
    therefore CUT by a model running on ``audio_ctx`` positions (``count_longer_than_audio_ctx``), and ``"sample_counts"``, every clip's
    length in 16 kHz samples, capped at the 30 s window (``PcmBatch.sample_counts``)."""
    batch = clips if isinstance(clips, PcmBatch) else PcmBatch(clips)
    if report is not None:
        counts = batch.sample_counts()
        report["longer_than_audio_ctx"] = count_longer_than_audio_ctx(counts, audio_ctx)
        report["sample_counts"] = counts
    return _ingest(batch, out)[0]


_tables = {}
_workspaces = {}


def _get_tables(n_mels: int) -> torch.Tensor:
    dev = device()
    key = (dev.index, n_mels)
    t = _tables.get(key)
    if t is None:
        L = _lib.lib()
        with on_stream() as s:
            t = torch.empty(L.wipa_logmel_tables_bytes(n_mels), dtype=torch.uint8, device=dev)
            _lib.check(L.wipa_logmel_init(ptr(t), n_mels, sptr(s)), "wipa_logmel_init")
        _tables[key] = t
    return t


def padded_mel_rows(batch: int, n_frames: int = N_FRAMES) -> int:
    return batch * (n_frames + 2) + 4


def audio_ctx_for_seconds(seconds: float) -> int:
    """the smallest ``audio_ctx`` (encoder positions of 20 ms = 320 samples) that covers ``seconds`` of audio: 6.0 -> 300"""
    if not 0.0 < seconds <= CHUNK_LENGTH:
        raise ValueError(f"audio_ctx_for_seconds: {seconds!r} s is outside (0, {CHUNK_LENGTH}]")
    per = 2 * HOP_LENGTH
    return max(1, -(-int(np.ceil(seconds * SAMPLE_RATE - 1e-6)) // per))


def count_longer_than_audio_ctx(n_samples: Iterable[int], audio_ctx: Optional[int]) -> int:
    """how many clips (by their sample counts at 16 kHz) exceed ``audio_ctx`` * 320 samples, i.e. are CUT by a model running on
    ``audio_ctx`` positions (None: the 30 s window)"""
    limit = N_SAMPLES if audio_ctx is None else int(audio_ctx) * 2 * HOP_LENGTH
    return sum(1 for n in n_samples if int(n) > limit)


def log_mel_padded(audio: torch.Tensor, n_mels: int = 80, dtype: torch.dtype = torch.float32,
                   n_frames: Optional[int] = None) -> torch.Tensor:
    """audio [B, 480000] f32 on the GPU -> padded mel [B*3002 + 4, n_mels] in ``dtype``
    (frame t of clip b at row b*3002 + t + 1): the layout the encoder consumes directly.
    ``n_frames`` (a model with ``audio_ctx`` = N passes 2N): the first n_frames frames of the same 30 s log-mel in the layout
    [B*(n_frames + 2) + 4, n_mels], zero halo rows at 0 and n_frames + 1 of every clip."""
    if n_frames is not None:
        return _log_mel_padded_frames(audio, n_mels, dtype, int(n_frames))
    L = _lib.lib()
    assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2 and audio.shape[1] == N_SAMPLES
    audio = audio.contiguous()
    B = audio.shape[0]
    tables = _get_tables(n_mels)
    with on_stream() as s:
        key = (audio.device.index, stream_id())
        ws = _workspaces.get(key)
        need = L.wipa_logmel_workspace_bytes(B, n_mels)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=audio.device)  # one per library stream
            _workspaces[key] = ws
        mel = torch.empty(padded_mel_rows(B), n_mels, dtype=dtype, device=audio.device)
        _lib.check(L.wipa_logmel(ptr(audio), B, n_mels, ptr(tables), ptr(mel), dt_code(dtype), ptr(ws), ws.numel(), sptr(s)),
                   "wipa_logmel")
    return mel


def _log_mel_padded_frames(audio: torch.Tensor, n_mels: int, dtype: torch.dtype, n_frames: int) -> torch.Tensor:
    L = _lib.lib()
    assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 2 and audio.shape[1] == N_SAMPLES
    if not 1 <= n_frames <= N_FRAMES:
        raise ValueError(f"log_mel_padded: n_frames={n_frames} (1..{N_FRAMES})")
    audio = audio.contiguous()
    B = audio.shape[0]
    tables = _get_tables(n_mels)
    with on_stream() as s:
        key = (audio.device.index, stream_id(), "frames")
        ws = _workspaces.get(key)
        need = L.wipa_logmel_frames_workspace_bytes(B, n_mels, n_frames)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=audio.device)  # one per library stream
            _workspaces[key] = ws
        mel = torch.empty(padded_mel_rows(B, n_frames), n_mels, dtype=dtype, device=audio.device)
        _lib.check(L.wipa_logmel_frames(ptr(audio), B, n_mels, ptr(tables), ptr(mel), dt_code(dtype), n_frames, ptr(ws), ws.numel(),
                                        sptr(s)), "wipa_logmel_frames")
    return mel


def log_mel_spectrogram(audio: ArrayLike, n_mels: int = 80, padding: int = 0) -> torch.Tensor:
    """mlx_whisper.audio.log_mel_spectrogram: [n] -> [n_frames, n_mels] f32 (time-major), or
    [B, n] -> [B, n_frames, n_mels].  Clips are processed in the 30 s window the reference
    always uses (``pad_or_trim`` first, ipa_data_loader.py:80-82); returned tensors live on the GPU."""
    if isinstance(audio, np.ndarray):
        audio = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    if padding:
        audio = torch.nn.functional.pad(audio, (0, padding))
    single = audio.dim() == 1
    if single:
        audio = audio[None]
    if audio.shape[-1] != N_SAMPLES:
        raise ValueError(f"log_mel_spectrogram expects {N_SAMPLES} samples per clip (use pad_or_trim), got {audio.shape[-1]}")
    audio = audio.to(device=device(), dtype=torch.float32)
    B = audio.shape[0]
    padded = log_mel_padded(audio, n_mels, torch.float32)
    mel = padded[: B * PADDED_FRAMES].view(B, PADDED_FRAMES, n_mels)[:, 1 : N_FRAMES + 1]
    return mel[0] if single else mel


# ---- SpecAugment (csrc/spec_augment.hip): time and mel-bin masks for fine-tuning ---------------------------------------------------

SPEC_AUGMENT_MAX_SPANS = _lib.SPEC_AUGMENT_MAX_SPANS


class SpecAugment:
    """Settings of the augmentation, named as in ``transformers`` (``mask_time_prob`` / ``_length`` / ``_min_masks``,
    ``mask_feature_*``): on each axis about ``prob * L / length`` spans of ``length`` positions (at least ``min_masks``, at most 64)
    become ``fill``; L is the clip's OWN frame count on the time axis (``n_frames``), so a 3 s clip in the 30 s window is masked over
    its 300 frames, not over 2700 frames of padding.  The draw is a pure function of (``seed``, the clip's stream, L): include/wipa.h
    states it in integers, ``plan`` returns it from the host without touching the GPU."""

    def __init__(self, mask_time_prob: float = 0.05, mask_time_length: int = 10, mask_time_min_masks: int = 2,
                 mask_feature_prob: float = 0.0, mask_feature_length: int = 10, mask_feature_min_masks: int = 0, fill: float = 0.0,
                 seed: int = 0):
        self.cfg = _lib.SpecAugmentCfg()
        for a, axis, prob, length, min_masks in ((0, "time", mask_time_prob, mask_time_length, mask_time_min_masks),
                                                 (1, "feature", mask_feature_prob, mask_feature_length, mask_feature_min_masks)):
            if isinstance(length, bool) or int(length) != length or int(length) < 1:
                raise _lib.WipaError(f"SpecAugment: mask_{axis}_length = {length!r}, must be an integer >= 1")
            if not 0.0 <= float(prob) <= 1.0:  # also refuses NaN
                raise _lib.WipaError(f"SpecAugment: mask_{axis}_prob = {prob!r}, outside [0, 1]")
            if isinstance(min_masks, bool) or int(min_masks) != min_masks or not 0 <= int(min_masks) <= SPEC_AUGMENT_MAX_SPANS:
                raise _lib.WipaError(f"SpecAugment: mask_{axis}_min_masks = {min_masks!r}, outside 0..{SPEC_AUGMENT_MAX_SPANS}")
            self.cfg.length[a], self.cfg.min_masks[a] = int(length), int(min_masks)
            self.cfg.rate_q16[a] = min(65536, round(float(prob) / int(length) * 65536))
        self.cfg.fill = float(fill)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.settings = dict(mask_time_prob=float(mask_time_prob), mask_time_length=int(mask_time_length),
                             mask_time_min_masks=int(mask_time_min_masks), mask_feature_prob=float(mask_feature_prob),
                             mask_feature_length=int(mask_feature_length), mask_feature_min_masks=int(mask_feature_min_masks),
                             fill=float(fill), seed=self.seed)

    @staticmethod
    def _host_rows(streams, n_frames) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        st = np.ascontiguousarray((np.asarray(streams, dtype=np.int64).reshape(-1, 2) & 0xFFFFFFFF).astype(np.uint32))
        if n_frames is None:
            return st, None
        nf = np.ascontiguousarray(np.clip(np.asarray(n_frames, dtype=np.int64).reshape(-1), 0, 2 ** 31 - 1).astype(np.int32))
        if nf.shape[0] != st.shape[0]:
            raise _lib.WipaError(f"SpecAugment: {st.shape[0]} streams but {nf.shape[0]} frame counts")
        return st, nf

    def plan(self, streams, n_frames, frames: int, n_mels: int) -> np.ndarray:
        """The spans every clip draws, from the host (wipa_spec_augment_plan: the text the kernel compiles).  ``streams`` [B, 2]
        (lo, hi), ``n_frames`` [B] or None -> int32 [B, 2, 65]: per clip and axis (0 time, 1 bins) the count, then the starts (-1
        in the unused places); every span covers min(length, L) positions."""
        st, nf = self._host_rows(streams, n_frames)
        out = np.empty((st.shape[0], 2, SPEC_AUGMENT_MAX_SPANS + 1), dtype=np.int32)
        _lib.check(_lib.lib().wipa_spec_augment_plan(C.byref(self.cfg), st.ctypes.data, None if nf is None else nf.ctypes.data, st.shape[0],
                                                     int(frames), int(n_mels), self.seed, out.ctypes.data), "wipa_spec_augment_plan")
        return out

    def mask_in_place(self, buf: torch.Tensor, offset: int, ld_clip: int, ld_frame: int, B: int, frames: int, n_mels: int, streams,
                      n_frames=None) -> None:
        """One launch on the current library stream: element (b, t, m) of the mask lands on the f32 tensor ``buf`` at flat element
        ``offset + b*ld_clip + t*ld_frame + m``.  Streams and frame counts go up in one non-blocking copy from pinned memory."""
        st, nf = self._host_rows(streams, n_frames)
        if st.shape[0] != B:
            raise _lib.WipaError(f"SpecAugment: {st.shape[0]} streams for {B} clips")
        assert buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()
        assert offset >= 0 and offset + (B - 1) * ld_clip + (frames - 1) * ld_frame + n_mels <= buf.numel()
        host = np.concatenate([st.reshape(-1).view(np.int32)] + ([] if nf is None else [nf]))
        with on_stream() as s:
            dev = torch.from_numpy(host).pin_memory().to(buf.device, non_blocking=True)
            _lib.check(_lib.lib().wipa_spec_augment(buf.data_ptr() + 4 * offset, ld_clip, ld_frame, B, frames, n_mels, C.byref(self.cfg),
                                                    dev.data_ptr(), None if nf is None else dev.data_ptr() + 8 * B, self.seed, sptr(s)),
                       "wipa_spec_augment")


def spec_augment(mel: torch.Tensor, aug: SpecAugment, streams, n_frames=None, frames: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A masked copy of ``mel`` [B, T, n_mels] f32 on the GPU; ``out=mel`` masks in place.  ``streams`` [B, 2]: the (lo, hi) stream
    of every clip; ``n_frames`` [B]: every clip's own length in frames (None: the whole time axis); ``frames`` (default T): the
    frames the time axis spans -- a model with ``audio_ctx`` = N sees the first 2N."""
    if not (mel.is_cuda and mel.dtype == torch.float32 and mel.dim() == 3):
        raise _lib.WipaError(f"spec_augment: an f32 device mel [B, T, n_mels] is expected, got {mel.dtype} {tuple(mel.shape)}")
    B, T, n_mels = mel.shape
    frames = T if frames is None else int(frames)
    if not 1 <= frames <= T:
        raise _lib.WipaError(f"spec_augment: frames={frames} (1..{T})")
    with on_stream():
        if out is None:
            out = mel.clone(memory_format=torch.contiguous_format)
        elif out is not mel:
            if out.shape != mel.shape or out.dtype != mel.dtype or not out.is_cuda:
                raise _lib.WipaError("spec_augment: out must match mel")
            out.copy_(mel)
        if not out.is_contiguous():
            raise _lib.WipaError("spec_augment: a contiguous tensor is expected")
        aug.mask_in_place(out, 0, T * n_mels, n_mels, B, frames, n_mels, streams, n_frames)
    return out


def frames_of_samples(n_samples: Iterable[int]) -> List[int]:
    """log-mel frames that carry a clip's own samples: ceil(samples / 160), capped at the 3000 of the 30 s window"""
    return [min(N_FRAMES, -(-int(n) // HOP_LENGTH)) for n in n_samples]
