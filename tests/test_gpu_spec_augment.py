"""GPU tests of SpecAugment (csrc/spec_augment.hip, audio.SpecAugment / spec_augment, DecoderTrainer(spec_augment=...)).

The kernel against the mask of the numpy restatement (tests/spec_augment_ref.py), as bits: a masked element holds ``fill``'s bits,
every other element of the buffer -- halo rows, frames beyond the time axis, padding -- holds what it held.  The trainer against a
trainer without an augmenter that is fed the restatement's masked mel: the same bytes of loss, gradients and parameters, because the
mask is exact and everything after it is the same launches on the same values."""
import functools
import itertools

import numpy as np
import pytest
import torch

import spec_augment_ref as SA
from oracle import whisper_ref as R
from spec_augment_cases import FRAMES, MIN_MASKS, N_MELS, SEED, augmenter, grid, refused, streams_for

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
EOT = 50257
FILLS = (0.0, -1.5, 0.0)  # by the grid point's min_masks index: the default and one whose bits are not zero


def _bits(x: float) -> int:
    return int(np.float32(x).view(np.int32))


class Layout:
    """where element (b, t, m) of a [B, frames, n_mels] mask lands in a flat buffer, and how large that buffer is"""

    def __init__(self, kind: str, B: int, frames: int, n_mels: int):
        self.kind, self.B, self.frames, self.n_mels = kind, B, frames, n_mels
        if kind == "dense":
            self.rows, self.offset, self.ld_clip = B * frames, 0, frames * n_mels
        elif kind == "prefix":  # the first ``frames`` frames of a 3000-frame mel
            self.rows, self.offset, self.ld_clip = B * 3000, 0, 3000 * n_mels
        else:  # "padded": frame t of clip b at row b*(frames + 2) + t + 1, four tail rows (wipa_mel_pad_cast_frames)
            self.rows, self.offset, self.ld_clip = B * (frames + 2) + 4, n_mels, (frames + 2) * n_mels

    def embed(self, mask: np.ndarray) -> torch.Tensor:
        """the mask [B, frames, n_mels] in the buffer's layout [rows, n_mels], False on every element that must stay"""
        full = np.zeros(self.rows * self.n_mels, dtype=bool)
        for b in range(self.B):
            lo = self.offset + b * self.ld_clip
            full[lo: lo + self.frames * self.n_mels] = mask[b].reshape(-1)
        return torch.from_numpy(full.reshape(self.rows, self.n_mels)).cuda()


@functools.lru_cache(maxsize=None)
def _poison(rows: int, n_mels: int) -> torch.Tensor:
    """random bits (NaN patterns among them); shared, never written: every test masks a clone"""
    g = torch.Generator().manual_seed(rows * 131 + n_mels)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, n_mels), generator=g, dtype=torch.int64).to(torch.int32).cuda()


def _run(aug, lay: Layout, streams, n_frames):
    """(the buffer after the launch, the buffer before) as int32 [rows, n_mels]"""
    before = _poison(lay.rows, lay.n_mels)
    work = before.clone()
    aug.mask_in_place(work.view(torch.float32).view(-1), lay.offset, lay.ld_clip, lay.n_mels, lay.B, lay.frames, lay.n_mels, streams, n_frames)
    torch.cuda.synchronize()
    return work, before


def _expect(before: torch.Tensor, lay: Layout, mask: np.ndarray, fill: float) -> torch.Tensor:
    return torch.where(lay.embed(mask), torch.full_like(before, _bits(fill)), before)


LAYOUTS = [(f, m, k) for f, m in itertools.product(FRAMES, N_MELS) for k in ("dense", "padded")] + [(66, m, "prefix") for m in N_MELS]


@pytest.mark.parametrize("frames,n_mels,kind", LAYOUTS)
def test_kernel_writes_the_restatements_mask_and_nothing_else(frames, n_mels, kind):
    from whisper_ipa_amd import audio

    checked = masked = 0
    for i, (B, length, nf, pkind, mm, rates) in enumerate(grid(frames, n_mels)):
        if refused(rates, frames, n_mels):
            continue  # the refusal itself: tests/test_spec_augment_host.py and test_refusals below
        fill = FILLS[MIN_MASKS.index(mm)]
        aug = augmenter(audio, rates, length, mm, fill=fill)
        streams = streams_for(B, i)
        n_frames = None if nf is None else [nf] * B
        lay = Layout(kind, B, frames, n_mels)
        work, before = _run(aug, lay, streams, n_frames)
        m = SA.mask(rates, (length, length), (mm, mm), streams, n_frames, frames, n_mels, SEED)
        assert torch.equal(work, _expect(before, lay, m, fill)), (B, length, nf, pkind, mm, rates)
        checked += 1
        masked += int(m.any())
    assert checked > 300 and masked > 100


def _find_stream(aug, frames, n_mels, n_frames, want):
    """the first stream (lo, 0) whose plan satisfies ``want(plan [2, 65])``, by the host plan"""
    lo = np.arange(4096)
    plans = aug.plan(np.stack([lo, np.zeros_like(lo)], axis=1), None if n_frames is None else [n_frames] * len(lo), frames, n_mels)
    for s, p in zip(lo, plans):
        if want(p):
            return int(s), p
    raise AssertionError("no stream of 4096 draws the wanted plan")


@pytest.mark.parametrize("n_mels", N_MELS)
def test_span_edges_and_overlaps(n_mels):
    """a bin span that ends at the last bin, a time span that ends at frame L - 1 (the clip's own last frame, inside a chunk and
    at 3000), and overlapping spans on both axes: found by the host plan, checked against the restatement's mask"""
    from whisper_ipa_amd import audio

    aug = audio.SpecAugment(0.05, 10, 2, 0.2, 10, 2, fill=7.25, seed=SEED)
    rates, lengths, mins = tuple(aug.cfg.rate_q16), (10, 10), (2, 2)

    def starts(p, a):
        return p[a, 1:1 + p[a, 0]]

    def overlap(p, a):
        s = np.sort(starts(p, a))
        return len(s) >= 2 and (np.diff(s) < 10).any() and (np.diff(s) > 0).any()

    cases = [
        (3000, 437, lambda p: (starts(p, 1) == n_mels - 10).any()),
        (3000, 437, lambda p: (starts(p, 0) == 437 - 10).any()),
        (3000, 3000, lambda p: (starts(p, 0) == 2990).any()),
        (150, 131, lambda p: overlap(p, 0) and overlap(p, 1)),
    ]
    for frames, L, want in cases:
        s, _ = _find_stream(aug, frames, n_mels, L, want)
        streams, n_frames = [[s, 0], [s + 1, 0]], [L, L]
        for kind in ("dense", "padded"):
            lay = Layout(kind, 2, frames, n_mels)
            work, before = _run(aug, lay, streams, n_frames)
            m = SA.mask(rates, lengths, mins, streams, n_frames, frames, n_mels, SEED)
            assert m[0].any() and not m[0].all() and not m[0, L:].all(axis=1).any()  # no time span beyond the clip's own frames
            assert torch.equal(work, _expect(before, lay, m, 7.25))


def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_runs_agree():
    from whisper_ipa_amd import audio

    aug = audio.SpecAugment(0.2, 10, 2, 0.1, 27, 1, seed=3)
    streams, n_frames = [[11, 2], [12, 2], [13, 2]], [3000, 517, 129]
    mel = _poison(3 * 3000, 80).view(torch.float32).view(3, 3000, 80)
    keep = mel.clone()
    a = audio.spec_augment(mel, aug, streams, n_frames)
    b = audio.spec_augment(mel, aug, streams, n_frames)
    torch.cuda.synchronize()
    assert torch.equal(mel.view(torch.int32), keep.view(torch.int32))  # a masked COPY: the input keeps its bits
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a.view(torch.int32), keep.view(torch.int32))
    for i in range(3):
        alone = audio.spec_augment(mel[i:i + 1], aug, streams[i:i + 1], n_frames[i:i + 1])
        assert torch.equal(alone[0].view(torch.int32), a[i].view(torch.int32))
    m = SA.mask(tuple(aug.cfg.rate_q16), (10, 27), (2, 1), streams, n_frames, 3000, 80, 3)
    assert torch.equal(a.view(torch.int32).cpu(), torch.from_numpy(SA.apply(keep.cpu().numpy(), m).view(np.int32)))
    # out=mel masks in place; frames= shortens the time axis (a model with audio_ctx = 33 sees 66 frames)
    work = keep.clone()
    assert audio.spec_augment(work, aug, streams, n_frames, frames=66, out=work) is work
    m66 = SA.mask(tuple(aug.cfg.rate_q16), (10, 27), (2, 1), streams, n_frames, 66, 80, 3)
    want = keep.cpu().numpy().copy()
    want[:, :66] = SA.apply(want[:, :66], m66)
    assert torch.equal(work.view(torch.int32).cpu(), torch.from_numpy(want.view(np.int32)))


def test_a_layout_without_16_byte_alignment():
    """rows of 81 floats from an odd element offset: the one-dword-per-thread instantiation writes the same mask, the gaps between
    rows and clips stay"""
    from whisper_ipa_amd import audio

    aug = audio.SpecAugment(0.2, 10, 2, 0.2, 10, 2, fill=-3.0, seed=5)
    B, frames, n_mels, offset, ld_frame = 3, 150, 80, 3, 81
    ld_clip = frames * ld_frame + 5
    streams, n_frames = streams_for(B, 9), [150, 77, 10]
    before = _poison(1, offset + B * ld_clip).view(-1)
    work = before.clone()
    aug.mask_in_place(work.view(torch.float32), offset, ld_clip, ld_frame, B, frames, n_mels, streams, n_frames)
    torch.cuda.synchronize()
    m = SA.mask(tuple(aug.cfg.rate_q16), (10, 10), (2, 2), streams, n_frames, frames, n_mels, 5)
    full = np.zeros(before.numel(), dtype=bool)
    idx = offset + np.arange(B)[:, None, None] * ld_clip + np.arange(frames)[None, :, None] * ld_frame + np.arange(n_mels)[None, None, :]
    full[idx[m]] = True
    assert m.any() and torch.equal(work, torch.where(torch.from_numpy(full).cuda(), torch.full_like(before, _bits(-3.0)), before))


def test_an_empty_plan_leaves_every_byte_alone():
    from whisper_ipa_amd import audio

    aug = audio.SpecAugment(0.0, 10, 0, 0.0, 10, 0, fill=9.0)
    for kind in ("dense", "padded"):
        lay = Layout(kind, 3, 150, 128)
        work, before = _run(aug, lay, streams_for(3, 5), [0, 70, 150])
        assert torch.equal(work, before)
    aug = audio.SpecAugment(0.5, 10, 64)  # spans wanted, but no frame to put them on and no bin probability
    lay = Layout("padded", 2, 66, 80)
    work, before = _run(aug, lay, streams_for(2, 6), [0, 0])
    assert torch.equal(work, before)


# ====================================================================== the trainer
def _model(W, **kw):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=torch.float32, f32_split=False, **kw)
    m.load_weights(W)
    return m


def _batch(B: int, T: int = 8, seed: int = 11):
    """mel [B, 3000, 80] in the front end's range and tokens [B, T + 1]: rows end in EOT at different lengths"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, 3000, 80, generator=g) * 2.0 - 1.0
    rng = np.random.default_rng(seed)
    sot = [50258, 50259, 50359, 50363]
    rows = []
    for b in range(B):
        row = sot + rng.integers(0, 50257, size=T + 1 - len(sot) - 1 - (b % 2) * 2).tolist() + [EOT]
        rows.append(row + [EOT] * (T + 1 - len(row)))
    return mel, torch.tensor(rows, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _weights():
    """shared; never modified (load_weights copies)"""
    return R.synthetic_weights(MICRO, seed=7)


def _augmenter():
    from whisper_ipa_amd import audio

    return audio.SpecAugment(0.2, 10, 2, 0.1, 8, 1, seed=77)


def _ref_masked(aug, mel: torch.Tensor, streams, n_frames, frames: int) -> torch.Tensor:
    """the restatement's masked mel: the first ``frames`` frames masked, the rest as they were"""
    m = SA.mask(tuple(aug.cfg.rate_q16), tuple(aug.cfg.length), tuple(aug.cfg.min_masks), streams, n_frames, frames, mel.shape[2], aug.seed)
    assert m.any() and not m.all()
    out = mel.numpy().copy()
    out[:, :frames] = SA.apply(out[:, :frames], m, aug.cfg.fill)
    return torch.from_numpy(out)


def _state(tr, loss):
    torch.cuda.synchronize()
    return loss.detach().cpu().numpy().tobytes(), tr.flat_g.cpu().numpy().tobytes(), tr.flat_p.cpu().numpy().tobytes()


@pytest.mark.parametrize("layers,n_ctx", [(0, None), ("all", None), (0, 33), ("all", 33)])
def test_train_step_equals_a_plain_trainer_on_the_restatements_masked_mel(layers, n_ctx):
    """two steps on the same clips: loss, gradients and updated parameters byte for byte; step 2 draws other masks than step 1;
    the caller's mel is not modified"""
    from whisper_ipa_amd.training import DecoderTrainer

    aug = _augmenter()
    mel, tokens = _batch(2)
    frames = 3000 if n_ctx is None else 2 * n_ctx
    n_frames = [137, 3000] if n_ctx is None else [41, 3000]
    mel_dev, keep = mel.cuda(), mel.clone()
    tr_a = DecoderTrainer(_model(_weights(), audio_ctx=n_ctx), train_encoder_layers=layers, spec_augment=aug)
    tr_p = DecoderTrainer(_model(_weights(), audio_ctx=n_ctx), train_encoder_layers=layers)
    seen = []
    for step in range(2):
        streams = [(b, step) for b in range(2)]
        masked = _ref_masked(aug, mel, streams, n_frames, frames)
        seen.append(masked)
        loss_a, _ = tr_a.train_step(mel_dev, tokens.cuda(), EOT, n_frames=n_frames)
        loss_p, _ = tr_p.train_step(masked.cuda(), tokens.cuda(), EOT)
        assert _state(tr_a, loss_a) == _state(tr_p, loss_p), (layers, n_ctx, step)
        assert torch.equal(mel_dev.cpu().view(torch.int32), keep.view(torch.int32))
    assert not torch.equal(seen[0], seen[1])
    # and the masks do matter: a plain trainer on the unmasked mel ends elsewhere
    tr_u = DecoderTrainer(_model(_weights(), audio_ctx=n_ctx), train_encoder_layers=layers)
    loss_u, _ = tr_u.train_step(mel_dev, tokens.cuda(), EOT)
    tr_u.train_step(mel_dev, tokens.cuda(), EOT)
    assert _state(tr_u, loss_u)[2] != _state(tr_p, loss_p)[2]


@pytest.mark.parametrize("layers", [0, "all"])
def test_clip_keys_name_the_streams_and_an_empty_plan_is_the_plain_step(layers):
    from whisper_ipa_amd import audio
    from whisper_ipa_amd.training import DecoderTrainer

    aug = _augmenter()
    mel, tokens = _batch(2)
    keys, n_frames = [4242, 17], [66, 30]
    tr_a = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=layers, spec_augment=aug)
    tr_p = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=layers)
    loss_a, _ = tr_a.train_step(mel.cuda(), tokens.cuda(), EOT, clip_keys=keys, n_frames=n_frames)
    loss_p, _ = tr_p.train_step(_ref_masked(aug, mel, [(k, 0) for k in keys], n_frames, 66).cuda(), tokens.cuda(), EOT)
    assert _state(tr_a, loss_a) == _state(tr_p, loss_p)
    empty = audio.SpecAugment(0.0, 10, 0, 0.0, 10, 0)
    tr_e = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=layers, spec_augment=empty)
    tr_n = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=layers, spec_augment=None)
    loss_e, _ = tr_e.train_step(mel.cuda(), tokens.cuda(), EOT, n_frames=n_frames)
    loss_n, _ = tr_n.train_step(mel.cuda(), tokens.cuda(), EOT)
    assert _state(tr_e, loss_e) == _state(tr_n, loss_n)


def test_refusals():
    from whisper_ipa_amd import _lib, audio
    from whisper_ipa_amd.training import DecoderTrainer

    aug = _augmenter()
    mel, tokens = _batch(2)
    tr = DecoderTrainer(_model(_weights(), audio_ctx=33), spec_augment=aug)
    with pytest.raises(_lib.WipaError, match="enable_feature_cache.*spec_augment"):
        tr.enable_feature_cache(4)
    with pytest.raises(_lib.WipaError, match=r"loss_and_grads\(audio_features.*spec_augment"):
        tr.loss_and_grads(tr.model.embed_audio(mel.cuda()), tokens.cuda(), EOT)
    cached = DecoderTrainer(_model(_weights(), audio_ctx=33))
    cached.enable_feature_cache(4)
    with pytest.raises(_lib.WipaError, match="spec_augment.*feature cache"):
        cached.spec_augment = aug
    with pytest.raises(_lib.WipaError, match="clip_keys"):
        tr.train_step(mel.cuda(), tokens.cuda(), EOT, clip_keys=[1, 2, 3])
    with pytest.raises(_lib.WipaError, match="too many spans"):  # the launch checks what the plan checks
        audio.spec_augment(mel.cuda(), audio.SpecAugment(1.0, 1, 0), [[0, 0], [1, 0]])
    with pytest.raises(_lib.WipaError, match="f32"):
        audio.spec_augment(mel.cuda().bfloat16(), aug, [[0, 0], [1, 0]])


# ====================================================================== data parallel
def _dp_worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    from whisper_ipa_amd.training import DecoderTrainer

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # one GPU box: gloo moves the CUDA tensors
    try:
        mel, tokens = _batch(4, seed=23)
        tr = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=1, spec_augment=_augmenter())
        lo, hi = rank * 2, rank * 2 + 2
        loss, _, n = tr.loss_and_grads_from_mel(mel[lo:hi].cuda(), tokens[lo:hi].cuda(), EOT, n_frames=[50, 66, 31, 3000][lo:hi])
        torch.cuda.synchronize()
        q.put((rank, float(loss), float(n), tr.flat_g.cpu().numpy(), tr._augment_streams(2, None)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_draw_disjoint_streams_and_equal_one_process_with_the_same_streams():
    """two ranks on one GPU, each half of 4 clips, K = 1, without clip_keys: rank r's rows draw from the streams (2r + b, step), so
    one process on the whole batch with clip_keys 0..3 masks the same way and gives the same statistics and gradients (bounds of
    test_data_parallel_two_ranks_equal_single_process_at_k1)"""
    import os

    import torch.multiprocessing as mp

    from whisper_ipa_amd.training import DecoderTrainer

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 90
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert res[0][4] == [(0, 0), (1, 0)] and res[1][4] == [(2, 0), (3, 0)]
    mel, tokens = _batch(4, seed=23)
    tr = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=1, spec_augment=_augmenter())
    loss, _, n = tr.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT, clip_keys=[0, 1, 2, 3], n_frames=[50, 66, 31, 3000])
    torch.cuda.synchronize()
    full = tr.flat_g.cpu().numpy()
    plain = DecoderTrainer(_model(_weights(), audio_ctx=33), train_encoder_layers=1)
    plain.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert np.abs(plain.flat_g.cpu().numpy() - full).max() > 1e-3 * np.abs(full).max()  # the masks move the gradients far more than the bound
    for r in res:
        assert abs(r[1] - float(loss)) < 1e-5 and r[2] == float(n)
        assert np.abs(r[3] - full).max() < 1e-5 * (np.abs(full).max() + 1e-9) + 1e-7
    assert np.array_equal(res[0][3], res[1][3])


# ====================================================================== lengths and the script
def _write_wavs(tmp_path, lengths):
    import wave

    rng = np.random.default_rng(0)
    paths = []
    for i, n in enumerate(lengths):
        p = tmp_path / f"c{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((0.1 * rng.standard_normal(n) * 32767).astype("<i2").tobytes())
        paths.append(str(p))
    return paths


def _scripts():
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "scripts") not in sys.path:
        sys.path.insert(0, os.path.join(root, "scripts"))


def test_get_batch_reports_the_frames_of_the_clips_it_read(tmp_path):
    import json

    from whisper_ipa_amd import audio

    _scripts()
    import ipa_data_loader as D

    lengths = (16000 * 2, 161, 16000 * 3 + 7, 160)
    paths = _write_wavs(tmp_path, lengths)
    report = {}
    audio.load_audio_batch(paths, report=report)
    assert report["sample_counts"] == list(lengths) and report["longer_than_audio_ctx"] == 0
    (tmp_path / "d.json").write_text(json.dumps([{"audio_path": p, "ipa_transcription": "kæt"} for p in paths]))
    ds = D.create_data_loader(str(tmp_path / "d.json"), allow_byte_fallback=True)
    assert ds.get_batch([0, 1, 2, 3])["n_frames"] == [200, 2, 301, 1]
    flagged = ds.get_batch([3, 2, 0], audio_for=[True, False, True])  # rows for the flagged clips only, like mel_features
    assert flagged["n_frames"] == [1, 200] and flagged["mel_features"].shape[0] == 2
    assert ds.get_batch([1], audio_for=[False])["n_frames"] == []


def test_train_script_with_spec_augment(tmp_path, capsys):
    """scripts/train_whisper_ipa.py --spec-augment --test-run on WAV clips, in the style of test_train_script_end_to_end_artefacts:
    the settings are recorded, the console says what is masked and that no cache is kept, the steps run"""
    import json
    import sys

    from whisper_ipa_amd.load_models import save_model

    _scripts()
    import train_whisper_ipa as T

    dims = R.ModelDimensions(80, 1500, 64, 1, 1, 51865, 448, 64, 1, 1)
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.float32)
    m.load_weights(R.synthetic_weights(dims, seed=4))
    model_dir = tmp_path / "whisper-micro"
    save_model(m, str(model_dir))
    paths = _write_wavs(tmp_path, [16000 * 2] * 4)
    entries = [{"audio_path": p, "ipa_transcription": "kæt " + "ab" * (i + 1), "speaker_id": f"s{i}"} for i, p in enumerate(paths)]
    (tmp_path / "train.json").write_text(json.dumps(entries))
    (tmp_path / "test.json").write_text(json.dumps(entries[:2]))
    out = tmp_path / "out"
    argv = ["train_whisper_ipa.py", "--model", str(model_dir), "--train-data", str(tmp_path / "train.json"), "--test-data",
            str(tmp_path / "test.json"), "--output-dir", str(out), "--steps", "2", "--batch-size", "2", "--validate-every", "2",
            "--save-every", "2", "--allow-byte-fallback", "--audio-ctx", "150", "--test-run", "--spec-augment", "--mask-time-prob", "0.1",
            "--mask-time-length", "7", "--mask-feature-prob", "0.05", "--mask-feature-length", "5", "--mask-feature-min-masks", "1",
            "--augment-seed", "9"]
    old = sys.argv
    sys.argv = argv
    try:
        T.main()
    finally:
        sys.argv = old
    text = capsys.readouterr().out
    assert "SpecAugment: time spans of 7 frames" in text and "No encoder feature cache: --spec-augment" in text
    assert "Step 2/2 | Loss:" in text
    cfg = json.load(open(out / "training_config.json"))["training_args"]
    assert cfg["test_run"] is True
    assert cfg["spec_augment"] == dict(mask_time_prob=0.1, mask_time_length=7, mask_time_min_masks=2, mask_feature_prob=0.05,
                                       mask_feature_length=5, mask_feature_min_masks=1, fill=0.0, seed=9)
    assert (out / "checkpoint-2" / "model.safetensors").exists()
    sys.argv = argv + ["--feature-cache-clips", "4"]
    try:
        with pytest.raises(SystemExit, match="--spec-augment with --feature-cache-clips"):
            T.main()
    finally:
        sys.argv = old
