"""numpy restatement of the log-mel front end (csrc/logmel.hip), twice, and the clips its tests run on.  No GPU, numpy only.

  reference64    the pipeline in float64 from the f32 samples: reflect-pad 200 | periodic Hann(400) | hop 160 | rfft | power of
                 frames 0..2999 | Slaney filterbank (oracle.whisper_ref.mel_filters widened to float64) | log10(max(., 1e-10)) |
                 max(., clip_max - 8) | (. + 4) / 4.  What the kernels are held to.
  emulate_f32    the same pipeline the way the fused kernel spells it, as numpy-f32 matrix products: the window lives inside
                 the cos / sin tables (float64 values rounded once to f32), the real frame is folded in half (e[k] = x[k] +
                 x[400-k], o[k] = x[k] - x[400-k], e[200] = x[200], k = 0 dropped because w[0] = 0), power -> mel is a second
                 f32 product.  ``fault`` plants one of FAULTS; ``shared_max`` replaces the clip's own maximum ("the batch
                 shares one maximum").  An unfaulted emulation is a second f32 reference beside the oracle's FFT path.
  signals        the seeded clips
  bound          the rule both the references and the kernels are held to: max(4 * e_ref, 2e-6), e_ref = the larger error of the
                 two f32 references against reference64.  The 4 covers another summation order of f32 sums of the same length
                 (BLAS blocks; the kernel runs folded 200-term chains on the MFMA); 2e-6 is 8 f32 ulps at |y| <= 2, what log10f
                 and the final divide can cost where the sums themselves are exact (silence, impulses).
"""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from oracle import whisper_ref as R

N_FFT = 400
HOP = 160
N_SAMPLES = 480000
N_FRAMES = 3000
N_BINS = 201
SR = 16000

FAULTS = ("cos_entry", "tables_10bit", "mel_tile_drop", "reflect_edge", "k200_twice", "floor_decade")
BOUND_FLOOR = 2e-6
BOUND_MARGIN = 4.0


def _frames(x: np.ndarray, edge_repeated_at_end: bool = False) -> np.ndarray:
    """[480000] -> [3000, 400] view of the reflect-padded clip (edge not repeated), in the dtype of ``x``"""
    assert x.shape == (N_SAMPLES,)
    pad = N_FFT // 2
    xp = np.pad(x, (pad, pad), mode="reflect")
    if edge_repeated_at_end:  # planted fault: the mirror at the end starts ON the last sample
        xp[pad + N_SAMPLES:] = x[::-1][:pad]
    return np.lib.stride_tricks.sliding_window_view(xp, N_FFT)[::HOP][:N_FRAMES]


def _finish(logmel: np.ndarray, floor_span: float, shared_max: Optional[float]) -> Tuple[np.ndarray, float]:
    dt = logmel.dtype.type
    mx = logmel.max() if shared_max is None else dt(shared_max)
    y = (np.maximum(logmel, mx - dt(floor_span)) + dt(4.0)) / dt(4.0)
    return y, float(mx)


def reference64(audio_f32: np.ndarray, n_mels: int) -> Tuple[np.ndarray, float]:
    """-> (y [3000, n_mels] float64, the clip's maximum of log10(mel))"""
    x = np.asarray(audio_f32, dtype=np.float32).astype(np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    spec = np.fft.rfft(_frames(x) * win, axis=-1)
    power = spec.real ** 2 + spec.imag ** 2
    mel = power @ R.mel_filters(n_mels).astype(np.float64).T
    return _finish(np.log10(np.maximum(mel, 1e-10)), 8.0, None)


def _tables() -> Tuple[np.ndarray, np.ndarray]:
    """cos / sin tables of the folded DFT with the window inside: [201 bins, 200] for k = 1..200, float64 -> f32 once; the sine
    column of k = 200 is zero (o[200] = 0)"""
    k = np.arange(1, 201)
    f = np.arange(N_BINS)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / N_FFT)
    ang = 2.0 * np.pi * ((f[:, None] * k[None, :]) % N_FFT) / N_FFT  # exact angle reduction
    c = win * np.cos(ang)
    s = -win * np.sin(ang)
    s[:, 199] = 0.0
    return c.astype(np.float32), s.astype(np.float32)


def _round_mantissa(a: np.ndarray, bits: int) -> np.ndarray:
    """f32 rounded (half up in magnitude) to ``bits`` explicit mantissa bits"""
    drop = 23 - bits
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + (1 << (drop - 1))) >> drop) << drop
    return u.astype(np.uint32).view(np.float32)


def _mel_tile_ranges(w: np.ndarray) -> np.ndarray:
    """[13, 2]: the mel tiles (16 mels) each frequency tile (16 bins) has a non-zero weight in, as wipa_logmel_init finds them"""
    n_mels = w.shape[0]
    out = np.zeros((13, 2), dtype=np.int64)
    for p in range(13):
        hit = [jt for jt in range((n_mels + 15) // 16) if np.any(w[16 * jt: 16 * jt + 16, 16 * p: 16 * p + 16] != 0)]
        if hit:
            out[p] = hit[0], hit[-1] + 1
    return out


def emulate_f32(audio_f32: np.ndarray, n_mels: int, fault: Optional[str] = None,
                shared_max: Optional[float] = None) -> Tuple[np.ndarray, float]:
    """-> (y [3000, n_mels] float32, the maximum it clamped against)"""
    assert fault is None or fault in FAULTS, fault
    x = np.asarray(audio_f32, dtype=np.float32)
    fr = _frames(x, edge_repeated_at_end=(fault == "reflect_edge"))
    a, c = fr[:, 1:201], fr[:, 399:199:-1]          # x[k] and x[400 - k] for k = 1..200
    e = a + c
    o = a - c
    e[:, 199] = fr[:, 200] * np.float32(2.0 if fault == "k200_twice" else 1.0)  # k = 200 pairs with itself
    o[:, 199] = 0.0
    ct, st = _tables()
    if fault == "cos_entry":
        ct[37, 92] *= np.float32(1.0 + 1e-3)       # bin 37 (1480 Hz), k = 93
    if fault == "tables_10bit":
        ct, st = _round_mantissa(ct, 10), _round_mantissa(st, 10)
    re = e @ ct.T
    im = o @ st.T
    power = re * re + im * im
    w = R.mel_filters(n_mels).copy()
    if fault == "mel_tile_drop":  # a mel tile that straddles two frequency tiles is handed only the first
        for p, (lo, hi) in enumerate(_mel_tile_ranges(w)):
            if hi - lo > 1:
                w[16 * (hi - 1): 16 * hi, 16 * p: 16 * p + 16] = 0.0
    mel = power @ w.T
    logmel = np.log10(np.maximum(mel, np.float32(1e-10)))
    return _finish(logmel, 7.0 if fault == "floor_decade" else 8.0, shared_max)


def bound(e_oracle: float, e_emulation: float) -> float:
    return max(BOUND_MARGIN * max(e_oracle, e_emulation), BOUND_FLOOR)


def reference_errors(audio_f32: np.ndarray, n_mels: int, ref: Optional[np.ndarray] = None) -> Tuple[float, float]:
    """(oracle-f32 error, unfaulted-emulation error) against reference64, max |dy| on the output scale"""
    if ref is None:
        ref = reference64(audio_f32, n_mels)[0]
    e_o = float(np.abs(R.log_mel_spectrogram(audio_f32, n_mels).astype(np.float64) - ref).max())
    e_e = float(np.abs(emulate_f32(audio_f32, n_mels)[0].astype(np.float64) - ref).max())
    return e_o, e_e


class Ref(NamedTuple):
    y: np.ndarray        # reference64's output [3000, n_mels] float64 (read-only)
    max: float           # the clip's maximum of log10(mel)
    floor_y: float       # (max - 8 + 4) / 4
    n_clamped: int       # elements the floor raised
    e_oracle: float
    e_emulation: float
    bound: float


@functools.lru_cache(maxsize=None)
def cached_signals() -> Dict[str, np.ndarray]:
    return signals()  # shared: not to be written to


@functools.lru_cache(maxsize=None)
def reference(name: str, n_mels: int) -> Ref:
    """reference64 of signals()[name] with the bound it sets, computed once per process and shared (arrays are read-only)"""
    a = cached_signals()[name]
    y, mx = reference64(a, n_mels)
    y.setflags(write=False)
    floor_y = (mx - 8.0 + 4.0) / 4.0
    e_o, e_e = reference_errors(a, n_mels, y)
    return Ref(y, mx, floor_y, int((y <= floor_y).sum()), e_o, e_e, bound(e_o, e_e))


IMPULSES_AT = (0, 1, 199, 200, 201, 20479, 20480, 20481, N_SAMPLES - 201, N_SAMPLES - 200, N_SAMPLES - 2, N_SAMPLES - 1)
SHORT_SAMPLES = 2 * SR + 77

# the batch order of the GPU tests: quiet clips sit between loud ones
ORDER = ("tone_1k", "silence", "chirp", "noise_1e-4", "speech", "impulses", "speech_2s", "tone_440_floor", "noise_clipped")
LOUD, QUIET = "tone_1k", "noise_1e-4"


def signals() -> Dict[str, np.ndarray]:
    """name -> [480000] f32, seeded, in ORDER"""
    rng = np.random.default_rng(20240611)
    t = np.arange(N_SAMPLES, dtype=np.float64) / SR
    s: Dict[str, np.ndarray] = {}
    s["tone_1k"] = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    s["silence"] = np.zeros(N_SAMPLES)
    s["chirp"] = 0.4 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (7900.0 - 50.0) / 30.0 * t * t))  # 50 Hz -> 7.9 kHz, linear
    s["noise_1e-4"] = 1e-4 * rng.standard_normal(N_SAMPLES)
    # harmonic, amplitude-modulated: a 110-150 Hz fundamental that wanders, 24 harmonics under two formant-like humps, a 3 Hz
    # syllable envelope that closes completely, a DC offset and a 1e-5 floor
    f0 = 130.0 + 20.0 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / SR
    voiced = np.zeros(N_SAMPLES)
    for h in range(1, 25):
        fh = 130.0 * h
        amp = np.exp(-0.5 * ((fh - 700.0) / 300.0) ** 2) + 0.5 * np.exp(-0.5 * ((fh - 2300.0) / 400.0) ** 2) + 0.01
        voiced += amp / h ** 0.5 * np.sin(h * phase + rng.uniform(0, 2 * np.pi))
    env = np.maximum(0.0, np.sin(2 * np.pi * 3.0 * t)) ** 2
    speech = 0.2 * env * voiced / np.abs(voiced).max() + 0.02 + 1e-5 * rng.standard_normal(N_SAMPLES)
    s["speech"] = speech
    imp = np.zeros(N_SAMPLES)
    for i, at in enumerate(IMPULSES_AT):
        imp[at] = (0.75, -0.5, 1.0)[i % 3]
    s["impulses"] = imp
    short = speech.copy()
    short[SHORT_SAMPLES:] = 0.0
    s["speech_2s"] = short
    s["tone_440_floor"] = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 1e-4 * rng.standard_normal(N_SAMPLES)
    s["noise_clipped"] = np.clip(0.8 * rng.standard_normal(N_SAMPLES), -1.0, 1.0)
    assert tuple(s) == ORDER
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in s.items()}
