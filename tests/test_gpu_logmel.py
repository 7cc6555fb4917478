"""The log-mel front end (csrc/logmel.hip) against a float64 statement of the pipeline (tests/logmel_ref.py) on tonal, quiet and
mixed batches: the fused kernel at every mel-tile count it is built for, the GEMM form behind WIPA_LOGMEL=gemm (in a child
process: the switch is read once) and as the fall-back for n_mels > 128 or n_mels % 4 != 0, bf16 output, batch independence,
the raw ABI call and its refusals.

The bound per clip and n_mels is ``logmel_ref.bound``: max(4 * e_ref, 2e-6) with e_ref the larger error of two f32 CPU references
against float64 -- never a figure taken from the kernel.  tests/test_logmel_host.py shows what that bound catches.
``pytest -m gpu`` on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logmel_ref as L

pytestmark = pytest.mark.gpu

ROWS = L.N_FRAMES + 2  # rows of a clip in the padded layout
ODD_CLIPS = ("chirp", "speech_2s", "silence")
FUSED_WS_BYTES = 256   # the fused form needs the per-clip maxima only
QUIET_ROW = L.ORDER.index(L.QUIET)


@pytest.fixture(scope="module")
def batch():
    S = L.cached_signals()
    return torch.from_numpy(np.stack([S[k] for k in L.ORDER])).cuda()


@pytest.fixture(scope="module")
def odd_batch():
    S = L.cached_signals()
    return torch.from_numpy(np.stack([S[k] for k in ODD_CLIPS])).cuda()


def _ws_bytes(B, n_mels):
    from whisper_ipa_amd import _lib

    return _lib.lib().wipa_logmel_workspace_bytes(B, n_mels)


def _check_clips(got, names, n_mels, form):
    """got [B, 3000, n_mels] f32 (numpy) against reference64 under the bound, and the maximum each clip clamped against"""
    failures = []
    for i, name in enumerate(names):
        r = L.reference(name, n_mels)
        y = got[i].astype(np.float64)
        err = float(np.abs(y - r.y).max())
        e_floor = abs(float(y.min()) - r.floor_y) if r.n_clamped else 0.0
        print(f"logmel {form} n_mels={n_mels} {name}: err {err:.2e}  floor err {e_floor:.2e}  e_ref {max(r.e_oracle, r.e_emulation):.2e}  "
              f"bound {r.bound:.2e}")
        if not (np.isfinite(y).all() and err <= r.bound and e_floor <= r.bound):
            failures.append((name, err, e_floor, r.bound))
    assert not failures, (form, n_mels, failures)


def _frames_of(padded, B, n_mels):
    return padded[: B * ROWS].view(B, ROWS, n_mels)[:, 1: L.N_FRAMES + 1]


def _assert_layout(padded, B, n_mels):
    assert tuple(padded.shape) == (B * ROWS + 4, n_mels)
    v = padded[: B * ROWS].view(B, ROWS, n_mels)
    assert (v[:, 0] == 0).all() and (v[:, ROWS - 1] == 0).all() and (padded[B * ROWS:] == 0).all()


@pytest.mark.parametrize("n_mels", [80, 128])
def test_fused_form_matches_float64_on_a_mixed_batch(batch, n_mels):
    from whisper_ipa_amd import audio as A

    assert _ws_bytes(len(L.ORDER), n_mels) == FUSED_WS_BYTES, "WIPA_LOGMEL=gemm is set: this test is about the fused form"
    p = A.log_mel_padded(batch, n_mels, torch.float32)
    _assert_layout(p, len(L.ORDER), n_mels)
    _check_clips(_frames_of(p, len(L.ORDER), n_mels).cpu().numpy(), L.ORDER, n_mels, "fused")


@pytest.mark.parametrize("n_mels", [80, 128])
def test_each_clip_alone_equals_its_row_of_the_batch(batch, n_mels):
    """the per-clip maximum is per clip, and reset per call: a quiet clip alone, then the batch (a loud clip in slot 0 of the
    workspace), then the quiet clip again on the same stream and workspace"""
    import whisper_ipa_amd as wipa

    lone_before = wipa.log_mel_spectrogram(batch[QUIET_ROW], n_mels=n_mels).clone()
    full = wipa.log_mel_spectrogram(batch, n_mels=n_mels).clone()
    lone_after = wipa.log_mel_spectrogram(batch[QUIET_ROW], n_mels=n_mels)
    assert torch.equal(lone_before, full[QUIET_ROW]) and torch.equal(lone_after, full[QUIET_ROW])
    for i, name in enumerate(L.ORDER):
        assert torch.equal(wipa.log_mel_spectrogram(batch[i: i + 1], n_mels=n_mels)[0], full[i]), name


@pytest.mark.parametrize("n_mels", [4, 64, 100, 132, 82, 32, 48, 96, 256])
def test_other_mel_counts_match_float64(odd_batch, n_mels):
    """4, 64, 100: 1, 4 and 7 mel tiles of the fused kernel, the last tile of 100 partly outside n_mels; 32, 48, 96: the 2, 3
    and 6 tile instantiations (80 and 128 are 5 and 8); 132 (> 128) and 82 (not a multiple of 4) take the GEMM form, as does
    256, the largest count, where filters narrower than a bin are empty.  bf16 output == the rounded f32 output over the whole
    padded buffer."""
    from whisper_ipa_amd import audio as A

    B = len(ODD_CLIPS)
    fused = n_mels <= 128 and n_mels % 4 == 0
    assert (_ws_bytes(B, n_mels) == FUSED_WS_BYTES) == fused
    p = A.log_mel_padded(odd_batch, n_mels, torch.float32)
    _assert_layout(p, B, n_mels)
    _check_clips(_frames_of(p, B, n_mels).cpu().numpy(), ODD_CLIPS, n_mels, "fused" if fused else "fall-back")
    assert torch.equal(A.log_mel_padded(odd_batch, n_mels, torch.bfloat16), p.to(torch.bfloat16))


@pytest.mark.parametrize("n_mels", [80, 128])
def test_bf16_output_is_the_rounded_f32_output(batch, n_mels):
    """both kernels are the same arithmetic templated on the output type and both conversions round to nearest even; the fused
    form clamps AFTER rounding, which logmel.hip claims is bit-identical to clamping first.  Halo and tail rows included."""
    from whisper_ipa_amd import audio as A

    f = A.log_mel_padded(batch, n_mels, torch.float32)
    b = A.log_mel_padded(batch, n_mels, torch.bfloat16)
    assert b.dtype == torch.bfloat16 and torch.equal(b, f.to(torch.bfloat16))


_GEMM_FORM_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import logmel_ref as L
from whisper_ipa_amd import _lib, audio as A
S = L.cached_signals()
a = torch.from_numpy(np.stack([S[k] for k in L.ORDER])).cuda()
q = L.ORDER.index(L.QUIET)
out = {}
for n in (80, 128):
    assert _lib.lib().wipa_logmel_workspace_bytes(len(L.ORDER), n) > (1 << 20), "the switch did not select the GEMM form"
    out[f"f32_{n}"] = A.log_mel_padded(a, n, torch.float32).cpu().numpy()
    out[f"bf16_{n}"] = A.log_mel_padded(a, n, torch.bfloat16).view(torch.int16).cpu().numpy()
    out[f"lone_{n}"] = A.log_mel_padded(a[q: q + 1], n, torch.float32).cpu().numpy()  # smaller batch on the reused workspace
np.savez(sys.argv[2], **out)
print("OK")
'''


def test_gemm_form_in_a_subprocess_matches_float64(tmp_path):
    """WIPA_LOGMEL=gemm (read once per process): reflect-pad kernel, f32 STFT GEMM over overlapping rows, mel / log and
    normalise kernels.  Compared with float64 under the same bound, never with the fused form."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "gemm_form.npz")
    env = dict(os.environ, WIPA_LOGMEL="gemm", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", _GEMM_FORM_CHILD, os.path.join(root, "tests"), path], capture_output=True, text=True,
                       timeout=300, env=env, cwd=root)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:] + r.stdout[-500:]
    g = np.load(path)
    B = len(L.ORDER)
    for n_mels in (80, 128):
        p = torch.from_numpy(g[f"f32_{n_mels}"])
        _assert_layout(p, B, n_mels)
        _check_clips(_frames_of(p, B, n_mels).numpy(), L.ORDER, n_mels, "gemm")
        assert torch.equal(torch.from_numpy(g[f"bf16_{n_mels}"]), p.to(torch.bfloat16).view(torch.int16))
        lone = torch.from_numpy(g[f"lone_{n_mels}"])
        _assert_layout(lone, 1, n_mels)
        assert torch.equal(lone[:ROWS], p[QUIET_ROW * ROWS: (QUIET_ROW + 1) * ROWS])


def _raw_call(audio, n_mels, mel, dtype_code, ws, ws_bytes=None):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd import audio as A
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    tables = A._get_tables(n_mels)
    with on_stream() as s:
        rc = _lib.lib().wipa_logmel(ptr(audio), audio.shape[0], n_mels, ptr(tables), ptr(mel), dtype_code, ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, sptr(s))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n_mels", [80, 82])
def test_direct_abi_call_writes_every_row_it_owns(odd_batch, n_mels):
    """mel pre-filled with NaN, the workspace with 0xFF (a maximum key above every real one, NaN spectra): halo rows and the 4
    tail rows come back zero, everything else finite -- in the fused form and in the fall-back"""
    from whisper_ipa_amd import _lib

    B = len(ODD_CLIPS)
    mel = torch.full((B * ROWS + 4, n_mels), float("nan"), device="cuda")
    ws = torch.full((_ws_bytes(B, n_mels),), 0xFF, dtype=torch.uint8, device="cuda")
    assert _raw_call(odd_batch, n_mels, mel, _lib.WIPA_F32, ws) == 0
    _assert_layout(mel, B, n_mels)
    assert torch.isfinite(mel).all()
    _check_clips(_frames_of(mel, B, n_mels).cpu().numpy(), ODD_CLIPS, n_mels, "raw call")


def test_init_refuses_mel_counts_outside_1_to_256():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    lib = _lib.lib()
    tables = torch.full((lib.wipa_logmel_tables_bytes(256),), 0xAB, dtype=torch.uint8, device="cuda")
    for n_mels in (0, 257):
        with on_stream() as s:
            rc = lib.wipa_logmel_init(ptr(tables), n_mels, sptr(s))
        torch.cuda.synchronize()
        assert rc != 0 and b"wipa_logmel_init" in lib.wipa_last_error(), (n_mels, rc)
        assert (tables == 0xAB).all()  # nothing was copied in


@pytest.mark.parametrize("n_mels", [80, 82])
def test_call_refuses_a_short_workspace_and_an_unknown_dtype_before_any_launch(odd_batch, n_mels):
    """in the fused form and in the fall-back: an error code, wipa_last_error set, and neither mel nor the workspace touched"""
    from whisper_ipa_amd import _lib

    lib = _lib.lib()
    B = len(ODD_CLIPS)
    need = _ws_bytes(B, n_mels)
    mel = torch.full((B * ROWS + 4, n_mels), float("nan"), device="cuda")
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool(torch.isnan(mel).all()) and bool((ws == 0xFF).all())

    rc = _raw_call(odd_batch, n_mels, mel, _lib.WIPA_F32, ws, ws_bytes=need - 1)
    assert rc != 0 and b"workspace too small" in lib.wipa_last_error(), rc
    assert untouched()
    for code in (_lib.WIPA_FP8_E4M3, 7, -1):
        rc = _raw_call(odd_batch, n_mels, mel, code, ws)
        assert rc != 0 and b"bad mel dtype" in lib.wipa_last_error(), (code, rc)
        assert untouched(), code
    assert _raw_call(odd_batch, n_mels, mel, _lib.WIPA_F32, ws) == 0 and bool(torch.isfinite(mel).all())  # the same buffers do serve
