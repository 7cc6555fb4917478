"""GPU: the short audio context -- ``Whisper(audio_ctx=N)`` -> ``wipa_model_cfg.n_audio_ctx`` = N: the model runs on the first N of its
1500 audio positions (whisper.cpp's --audio-ctx).  The reference is always the CPU oracle on ``mel[:, :2N]``: the same Whisper with
n_audio_ctx = N (``R.encoder_forward`` adds ``pos[:N]``, the decoder takes features of any length).  ``pytest -m gpu`` on an MI355X.

N = 33 lies below two 32-frame tiles (one frame split and a tail group in the absorbed cross-attention, one key tile in the encoder's
flash attention), 75 ends in a tail tile, 256 is an exact multiple of 64 (no tail code runs), 300 is the workload's N (6 s clips)."""
import functools

import numpy as np
import pytest
import torch

import alignment_ref as AR
import beam_cases as BC
import beam_ref as BM
import best_of_ref as BR
import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R
from parity_util import BF16_LOGIT_ERR_CEILING, check_low_precision_decode

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
SMALL2 = R.ModelDimensions(80, 1500, 768, 12, 2, 51865, 448, 768, 12, 2)  # whisper-small width, 2+2 layers
DIMS = {"micro": (MICRO, 7), "small2": (SMALL2, 11)}
SP = R.SpecialTokens.multilingual()
EOT, TB, NT, V = SP.eot, SP.timestamp_begin, SP.no_timestamps, 51865
INIT = list(SP.sot_sequence_including_notimestamps(0))
SOT_SEQ = [SP.sot, SP.lang_first, SP.transcribe]
F32_TOL = 1e-3  # the project's f32 bound on features, logits and loss


def _model(dims_o, W, dtype, audio_ctx=None, **kw):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype, audio_ctx=audio_ctx, **kw)
    m.load_weights(W)
    return m


# ---------------------------------------------------------------- references, computed once and shared
@functools.lru_cache(maxsize=None)
def clips():
    return np.stack([R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0), R.synthetic_clip(2, 12.0)])


@functools.lru_cache(maxsize=None)
def mels() -> torch.Tensor:
    """the oracle's log-mel of the three clips [3, 3000, 80]"""
    return torch.from_numpy(np.stack([R.log_mel_spectrogram(a) for a in clips()]))


@functools.lru_cache(maxsize=None)
def weights(name):
    dims, seed = DIMS[name]
    return R.synthetic_weights(dims, seed=seed)


@functools.lru_cache(maxsize=None)
def oracle_features(name, n_ctx, n_clips=2):
    """the oracle's encoder on the first 2N frames: [n_clips, N, d]"""
    with torch.no_grad():
        return R.encoder_forward(weights(name), DIMS[name][0], mels()[:n_clips, : 2 * n_ctx])


@functools.lru_cache(maxsize=None)
def oracle_greedy(name, n_ctx, n_new, keep_logits=False):
    always, first = R.suppress_lists(SP)
    with torch.no_grad():
        return R.greedy_decode(weights(name), DIMS[name][0], oracle_features(name, n_ctx), INIT, always, first, EOT, sample_len=n_new,
                               stop_on_eot=False, keep_logits=keep_logits)


# ---------------------------------------------------------------- 1. the padded layout for 2N frames
@pytest.mark.parametrize("n_ctx", [75, 300])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_padded_layout_for_2n_frames(n_ctx, dtype):
    """[B (2N + 2) + 4, n_mels]: rows 0 and 2N + 1 of every clip and the 4 trailing rows are zero -- row 2N + 1 in particular, where the
    3002-row layout holds the real frame 2N -- and rows 1..2N carry the bits of the same rows of the 3002-row layout.  The same layout
    from wipa_mel_pad_cast_frames, fed the full mel (clip stride 3000 rows) and the cut one."""
    from whisper_ipa_amd import _lib, audio
    from whisper_ipa_amd.runtime import dt_code, on_stream, ptr, sptr

    a = torch.from_numpy(clips()).cuda()
    B, F = a.shape[0], 2 * n_ctx
    full = audio.log_mel_padded(a, 80, dtype)
    short = audio.log_mel_padded(a, 80, dtype, n_frames=F)
    assert tuple(short.shape) == (B * (F + 2) + 4, 80) and short.dtype == dtype
    fv = full[: B * 3002].view(B, 3002, 80)
    sv = short[: B * (F + 2)].view(B, F + 2, 80)
    assert (sv[:, 0] == 0).all() and (sv[:, F + 1] == 0).all() and (short[B * (F + 2):] == 0).all()
    assert torch.equal(sv[:, 1: F + 1], fv[:, 1: F + 1])
    assert (fv[:, F + 1] != 0).any()  # the premise: the 3002-row layout has a real frame where the short one needs its halo
    # wipa_mel_pad_cast_frames: from a full f32 mel and from its first 2N frames
    mel = fv[:, 1:3001].float().contiguous()
    L = _lib.lib()
    for src in (mel, mel[:, :F].contiguous()):
        with on_stream() as s:
            out = torch.full((B * (F + 2) + 4, 80), float("nan"), dtype=dtype, device="cuda")
            _lib.check(L.wipa_mel_pad_cast_frames(ptr(src), src.shape[1] * 80, B, 80, F, ptr(out), dt_code(dtype), sptr(s)), "pad_cast_frames")
        assert torch.equal(out, short)
    with on_stream() as s:
        assert L.wipa_mel_pad_cast_frames(ptr(mel), 3000 * 80, B, 80, 3001, ptr(out), dt_code(dtype), sptr(s)) != 0
        assert L.wipa_mel_pad_cast_frames(ptr(mel), F * 80 - 1, B, 80, F, ptr(out), dt_code(dtype), sptr(s)) != 0  # clips would overlap


# ---------------------------------------------------------------- 2. the encoder, f32
@pytest.mark.parametrize("n_ctx", [33, 75, 256, 300])
@pytest.mark.parametrize("name", ["micro", "small2"])
def test_encoder_f32_matches_the_oracle_on_2n_frames(name, n_ctx, f32_mode):
    dims = DIMS[name][0]
    xa = oracle_features(name, n_ctx)
    # the premise, on the oracle itself: the N-position model is NOT the first N rows of the full-context model -- conv1 at frame
    # 2N - 1 and conv2 at position N - 1 see zero padding where the 30 s model sees frame 2N, and attention spreads that
    full = oracle_features(name, 1500)[:, :n_ctx]
    premise = (xa - full).abs().max().item()
    assert premise > 100 * F32_TOL, premise
    m = _model(dims, weights(name), torch.float32, audio_ctx=n_ctx, f32_split=(f32_mode == "split"))
    assert m.dims.n_audio_ctx == 1500 and m.n_audio_ctx == n_ctx and m.packed()["cfg"].n_audio_ctx == n_ctx
    mel = mels()[:2].cuda()
    feats = m.encoder(mel)
    assert tuple(feats.shape) == (2, n_ctx, dims.n_audio_state)
    err = (feats.cpu() - xa).abs().max().item()
    err_last = (feats.cpu()[:, -1] - xa[:, -1]).abs().max().item()  # on its own: an edge-frame mistake must not hide in a max
    print(f"\n{name} N={n_ctx} {f32_mode}: features within {err:.2e} of the oracle, last position {err_last:.2e}; "
          f"oracle(mel[:2N]) vs oracle(mel)[:N] differ by {premise:.2e}")
    assert err < F32_TOL and err_last < F32_TOL, (err, err_last)
    # a mel already cut to 2N frames is the same input
    assert torch.equal(m.embed_audio(mel[:, : 2 * n_ctx].contiguous()), feats)
    # a clip alone == the clip in the batch, where both run in the tile GEMMs (more than 256 rows: one summation order).  At
    # B N <= 256 rows wipa_gemm takes the weight-streaming kernel, whose K split differs: equal to f32 rounding only
    alone = m.encoder(mel[1:2])[0]
    if n_ctx > 256:
        assert torch.equal(alone, feats[1])
    assert (alone - feats[1]).abs().max().item() < 1e-4


def test_encoder_from_audio_through_the_frames_log_mel():
    """audio -> wipa_logmel_frames -> encoder, the path transcribe_batches takes, equals mel -> embed_audio"""
    from whisper_ipa_amd import audio

    m = _model(MICRO, weights("micro"), torch.float32, audio_ctx=75)
    a = torch.from_numpy(clips()[:2]).cuda()
    mel = audio.log_mel_spectrogram(a, n_mels=80)
    direct = m.encode_padded(audio.log_mel_padded(a, 80, torch.float32, n_frames=150), 2)
    assert torch.equal(direct, m.embed_audio(mel))
    assert (direct.cpu() - oracle_features("micro", 75)).abs().max().item() < F32_TOL


# ---------------------------------------------------------------- 3. audio_ctx = 1500 is audio_ctx = None
@pytest.mark.parametrize("name,dtype,cross", [("micro", torch.float32, "auto"), ("small2", torch.bfloat16, "absorbed"),
                                              ("small2", torch.bfloat16, "cached")])
def test_audio_ctx_1500_is_the_default_bit_for_bit(name, dtype, cross):
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    dims = DIMS[name][0]
    always, first = R.suppress_lists(SP)
    mel = mels()[:2].cuda()
    out = []
    for n in (None, 1500):
        m = _model(dims, weights(name), dtype, audio_ctx=n, cross_attention=cross)
        assert m.n_audio_ctx == 1500 and m.audio_ctx == n
        feats = m.encoder(mel)
        g = greedy_decode_tokens(m, feats, INIT, always, first, EOT, max_new_tokens=12, stop_on_eot=False)
        out.append((feats, g.tokens, g.sum_logprobs.copy(), g.last_logits.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert (out[0][1] == out[1][1]).all() and np.array_equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])


# ---------------------------------------------------------------- 4. greedy, f32
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("n_ctx", [75, 300])
@pytest.mark.parametrize("name", ["micro", "small2"])
def test_greedy_f32_ids_equal_the_oracles(name, n_ctx, use_graph):
    """mel -> encoder -> 24 greedy tokens on N positions.  The oracle's smallest top-1 margins over these steps were measured on the
    CPU at 5.8e-3 (MICRO) and 2.0e-2 (SMALL2) and more, against an f32 logit error of 3e-5 (exact products) .. 2.1e-4 (split): the
    ids can be compared exactly."""
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    dims = DIMS[name][0]
    ref = oracle_greedy(name, n_ctx, 24)
    print(f"\n{name} N={n_ctx}: oracle min top-1 margin {ref.margins.min():.3e}")
    always, first = R.suppress_lists(SP)
    m = _model(dims, weights(name), torch.float32, audio_ctx=n_ctx)
    feats = m.encoder(mels()[:2].cuda())
    res = greedy_decode_tokens(m, feats, INIT, always, first, EOT, max_new_tokens=24, stop_on_eot=False, use_graph=use_graph)
    assert res.tokens.shape == ref.tokens.shape
    assert (res.tokens == ref.tokens).all(), (res.tokens.tolist(), ref.tokens.tolist(), float(ref.margins.min()))
    assert np.abs(res.sum_logprobs - ref.sum_logprobs).max() < 1e-2


# ---------------------------------------------------------------- 5. bf16, cached and absorbed with 1, 2 and 4 frame splits
@pytest.mark.parametrize("form", ["cached", "absorbed1", "absorbed2", "absorbed4"])
@pytest.mark.parametrize("n_ctx", [33, 75, 300])
def test_bf16_small_width_under_the_measured_error_rule(n_ctx, form):
    """tests/parity_util.check_low_precision_decode at N keys: every differing id sits where the oracle's margin is within twice the
    MEASURED logit error, and that error stays under BF16_LOGIT_ERR_CEILING (a regression guard measured at 1500 keys).  The split
    count the launch uses is wipa_cross_absorbed_splits(want, N): at N = 33 every request runs one split with a tail group."""
    from whisper_ipa_amd import _lib

    cross = "cached" if form == "cached" else "absorbed"
    m = _model(SMALL2, weights("small2"), torch.bfloat16, audio_ctx=n_ctx, cross_attention=cross)
    if cross == "absorbed":
        m.cross_splits = int(form[-1])
        used = _lib.lib().wipa_cross_absorbed_splits(m.cross_splits, n_ctx)
        assert used == max(1, min(m.cross_splits, ((n_ctx + 31) // 32) // 2)), (n_ctx, used)
    feats = m.encoder(mels()[:2].cuda())
    xa = oracle_features("small2", n_ctx)
    assert feats.dtype == torch.bfloat16 and tuple(feats.shape) == (2, n_ctx, 768)
    rel = ((feats.float().cpu() - xa).abs().max() / xa.abs().max()).item()
    assert rel < 5e-2, rel
    always, first = R.suppress_lists(SP)
    ref = oracle_greedy("small2", n_ctx, 16, keep_logits=True)
    err, rep = check_low_precision_decode(m, feats, ref, INIT, always, first, EOT, f"small width bf16, N={n_ctx}, {form}",
                                          ceiling=BF16_LOGIT_ERR_CEILING)
    print(f"\nN={n_ctx} {form}: features rel {rel:.3e}; rel_err {rep['rel_err']:.4f} of the logit std (ceiling {BF16_LOGIT_ERR_CEILING})")


# ---------------------------------------------------------------- 6. batch invariance at N = 300, absorbed bf16
@pytest.mark.parametrize("use_graph", [True, False])
def test_a_clip_alone_equals_the_clip_in_a_batch_of_three_absorbed_bf16(use_graph):
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    always, first = R.suppress_lists(SP)
    m = _model(SMALL2, weights("small2"), torch.bfloat16, audio_ctx=300, cross_attention="absorbed")
    mel = mels().cuda()
    feats = m.encoder(mel)
    three = greedy_decode_tokens(m, feats, INIT, always, first, EOT, max_new_tokens=12, stop_on_eot=False, use_graph=use_graph)
    t3, l3 = three.tokens.copy(), three.last_logits.clone()
    for i in range(3):
        f1 = m.encoder(mel[i: i + 1])
        assert torch.equal(f1[0], feats[i]), i
        one = greedy_decode_tokens(m, f1, INIT, always, first, EOT, max_new_tokens=12, stop_on_eot=False, use_graph=use_graph)
        assert (one.tokens[0] == t3[i]).all(), (i, one.tokens.tolist(), t3[i].tolist())
        assert torch.equal(one.last_logits[0], l3[i]), i


# ---------------------------------------------------------------- 7. nothing unwritten is read
# every step form of MICRO (WIPA_DECODE_FUSED 0 / 1 / 2) in both dtypes; at d = 768 the default step with either cross-attention form
POISON_CASES = [("micro", dt, "auto", mode) for dt in (torch.float32, torch.bfloat16) for mode in ("0", "1", "2")] + [
    ("small2", torch.bfloat16, "absorbed", "0"), ("small2", torch.bfloat16, "cached", "0")]


@pytest.mark.parametrize("name,dtype,cross,mode", POISON_CASES)
def test_decode_and_encoder_never_read_unwritten_memory_at_75_positions(monkeypatch, name, dtype, cross, mode):
    """as tests/test_gpu_model.py::test_decode_never_reads_unwritten_state, at N = 75: the decode blob and the encoder workspace are
    filled with 0xFF bytes (NaN in f32 and bf16) before the run; results are finite and equal those on zeroed memory.  A walk past
    the 75 keys -- into the next clip's rows or the region behind the last clip -- would show here even where a softmax masks it
    arithmetically, because NaN survives a multiplication by zero."""
    from whisper_ipa_amd.decoding import _packed_for, _state_for, greedy_decode_tokens
    from whisper_ipa_amd.runtime import on_stream

    dims = DIMS[name][0]
    always, first = R.suppress_lists(SP)
    monkeypatch.setenv("WIPA_DECODE_FUSED", mode)
    m = _model(dims, weights(name), dtype, audio_ctx=75, cross_attention=cross)
    mel = mels()[:2].cuda()
    enc = {}
    for fill in (0x00, 0xFF):
        m.encoder(mel[:1])  # makes the workspace
        with on_stream():
            for ws in m._enc_ws.values():
                ws.fill_(fill)
        enc[fill] = m.encoder(mel)
    assert torch.isfinite(enc[0xFF].float()).all() and torch.equal(enc[0x00], enc[0xFF])
    feats = enc[0x00]
    out = {}
    for prompt in (INIT, INIT[:1]):
        for fill in (0x00, 0xFF):
            with on_stream():
                _state_for(m, 2, _packed_for(m, 2, 10)).blob.fill_(fill)
            r = greedy_decode_tokens(m, feats, prompt, always, first, EOT, max_new_tokens=10, stop_on_eot=False)
            out[(len(prompt), fill)] = (r.tokens, r.sum_logprobs.copy(), r.last_logits.clone())
        a, b = out[(len(prompt), 0x00)], out[(len(prompt), 0xFF)]
        assert np.isfinite(b[1]).all() and (a[0] == b[0]).all() and np.array_equal(a[1], b[1]), (mode, len(prompt))
        assert torch.equal(a[2], b[2])


# ---------------------------------------------------------------- 8. one test per decode mode at N = 75, MICRO f32
N_MODE = 75
STEPS = 20


def _rules():
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(TB, NT, 50)


@functools.lru_cache(maxsize=None)
def scripted():
    """the scripted MICRO weights of tests/prompt_ref.py (every rule branch fires) and the oracle's features of them at N = 75"""
    W = PR.weights(MICRO, 7, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, MICRO, mels()[:2, : 2 * N_MODE])
    return W, xa


@pytest.mark.parametrize("which", ["lively", "scripted"])
def test_timestamp_rules_at_75_positions(which):
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    W, xa = (weights("micro"), oracle_features("micro", N_MODE)) if which == "lively" else scripted()
    always, first = R.suppress_lists(SP)
    ref = TR.greedy_with_rules(R, W, MICRO, xa, SOT_SEQ, always, first, EOT, TB, NT, STEPS)
    print(f"\n{which}: branch counts {ref.counts}; min top-2 margin {ref.margins.min():.4f}, min mass gap {ref.mass_gaps.min():.4f}")
    # before any GPU result: every choice is decided by more than twice the f32 path's logit error (2.1e-4 with split products, README)
    assert all(n >= 1 for n in ref.counts.values()) and ref.margins.min() > 1e-3 and ref.mass_gaps.min() > 1e-3
    m = _model(MICRO, W, torch.float32, audio_ctx=N_MODE)
    feats = m.encoder(mels()[:2].cuda())
    for use_graph in (True, False):
        res = greedy_decode_tokens(m, feats, SOT_SEQ, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, use_graph=use_graph,
                                   rules=_rules())
        assert (res.tokens == ref.tokens).all(), (use_graph, res.tokens.tolist(), ref.tokens.tolist())
        assert np.abs(res.sum_logprobs - ref.sum_logprobs).max() < 1e-2


SAMPLE = dict(seed=5, temperature=0.7, attempt=2)
STREAMS = [(40, 1), (7, 0)]


@functools.lru_cache(maxsize=None)
def sampled_rows(n_group):
    """tests/prompt_ref.sample_row_loop on the oracle's N-row features: clip-major, candidate k of a clip on its candidate stream"""
    W, xa = weights("micro"), oracle_features("micro", N_MODE)
    return [PR.sample_row_loop(W, MICRO, xa[c: c + 1], INIT, STEPS, SAMPLE["seed"], SAMPLE["temperature"], BR.candidate_stream(STREAMS[c], k),
                               SAMPLE["attempt"], with_rules=False) for c in range(2) for k in range(n_group)]


def _options(**kw):
    import whisper_ipa_amd as wipa

    return wipa.DecodingOptions(**{**dict(language="en", without_timestamps=True, fp16=False, sample_len=STEPS), **kw})


def _cut(row):
    row = [int(t) for t in row]
    return row[: row.index(EOT)] if EOT in row else row


def test_sampling_with_a_seed_at_75_positions():
    import whisper_ipa_amd as wipa

    loops = sampled_rows(1)
    margin = min(float(l.key_margins.min()) for l in loops)
    print(f"\nsampling: smallest key margin of the restatement {margin:.3e} (needed: {BR.MARGIN})")
    assert margin > BR.MARGIN  # before any GPU result: every draw is decided by more than an f32 key can move
    m = _model(MICRO, weights("micro"), torch.float32, audio_ctx=N_MODE)
    feats = m.encoder(mels()[:2].cuda())
    res = wipa.decode(m, feats, _options(temperature=SAMPLE["temperature"], seed=SAMPLE["seed"], sample_attempt=SAMPLE["attempt"],
                                         sample_streams=STREAMS))
    for c, (r, l) in enumerate(zip(res, loops)):
        want = _cut(l.tokens[len(INIT):])
        assert r.tokens == want, (c, r.tokens, want)
        assert abs(r.avg_logprob * (len(r.tokens) + 1) - l.sum_logprob) < 1e-2


def test_best_of_3_at_75_positions():
    import whisper_ipa_amd as wipa

    loops = sampled_rows(3)
    margin = min(float(l.key_margins.min()) for l in loops)
    assert margin > BR.MARGIN, margin
    toks = np.array([list(l.tokens[len(INIT):]) + [EOT] for l in loops], dtype=np.int64)
    sums = np.array([l.sum_logprob for l in loops], dtype=np.float32)
    winner, _, scores = BR.rank(toks, sums, 3, 0, STEPS + 1, EOT, None)
    gaps = [sorted(s)[-1] - sorted(s)[-2] for s in scores]
    print(f"\nbest_of 3: winners {winner.tolist()}, scores {scores}, smallest key margin {margin:.3e}")
    assert min(gaps) > 1e-3, gaps  # the ranking is decided by more than the 1e-2 / 20 tokens the sums may move
    m = _model(MICRO, weights("micro"), torch.float32, audio_ctx=N_MODE)
    feats = m.encoder(mels()[:2].cuda())
    res = wipa.decode(m, feats, _options(best_of=3, temperature=SAMPLE["temperature"], seed=SAMPLE["seed"], sample_attempt=SAMPLE["attempt"],
                                         sample_streams=STREAMS))
    for c in range(2):
        want = _cut(loops[3 * c + int(winner[c])].tokens[len(INIT):])
        assert res[c].tokens == want, (c, int(winner[c]), res[c].tokens, want)


@functools.lru_cache(maxsize=None)
def beam_fixture():
    """the beam tests' MICRO weights (tests/beam_cases.py: a scaled final LayerNorm, so that the restatement's decisions are wide
    enough for an f32 device) with the oracle's features at N = 75, and the restatement's decode of both clips with 3 beams"""
    W, _ = BC.micro_fixture()
    with torch.no_grad():
        xa = R.encoder_forward(W, MICRO, mels()[:2, : 2 * N_MODE])
    initial, always, first, rules = BC.decode_inputs(False)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    want = [BM.decode_clip(BM.oracle_logits_fn(R, W, MICRO, xa[c]), initial, 3, None, None, EOT, BC.SAMPLE_LEN, m_first, m_always, rules)
            for c in range(2)]
    return W, xa, want


def test_beam_size_3_at_75_positions():
    import whisper_ipa_amd as wipa

    W, xa, want = beam_fixture()
    print(f"\nbeams: the restatement's smallest decision margin {BM.min_margin(want):.3e} (needed: {BC.required_margin():.3e})")
    assert BM.min_margin(want) >= BC.required_margin()
    m = _model(MICRO, W, torch.float32, audio_ctx=N_MODE, cross_attention="cached")
    feats = m.encoder(mels()[:2].cuda())
    assert (feats.cpu() - xa).abs().max().item() < F32_TOL
    res = wipa.decode(m, feats, wipa.DecodingOptions(language="en", without_timestamps=True, beam_size=3, sample_len=BC.SAMPLE_LEN, fp16=False))
    for r, w in zip(res, want):
        assert r.tokens == w.tokens, (r.tokens, w.tokens)
        assert abs(r.avg_logprob - float(w.sum_logprob) / (len(w.tokens) + 1)) < 1e-3


def test_per_row_prompts_at_75_positions():
    """five rows with histories of 0, 1, 17, 70 and 223 tokens over the two clips, each against the per-row CPU loop of
    tests/prompt_ref.py on the N-row features"""
    from whisper_ipa_amd.decoding import ragged_decode_tokens

    W, xa = scripted()
    rows = PR.initial_rows()
    refs = PR.per_row_reference(W, MICRO, xa, rows)
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32, audio_ctx=N_MODE)
    f2 = m.encoder(mels()[:2].cuda())
    feats = torch.stack([f2[b % 2] for b in range(len(rows))]).contiguous()
    g = ragged_decode_tokens(m, feats, rows, always, first, EOT, max_new_tokens=PR.STEPS, stop_on_eot=False, rules=_rules())
    for b, ref in enumerate(refs):
        got = g.tokens[b, g.n_init:].tolist()
        want = ref.loop.tokens[0, len(rows[b]):].tolist()
        assert got == want, (b, got, want)
        assert abs(float(g.sum_logprobs[b]) - float(ref.loop.sum_logprobs[0])) < 1e-2


LENS = [5, 17, 2, 9, 12]


def test_decode_continuous_2_slots_5_clips_at_75_positions():
    from whisper_ipa_amd.continuous import decode_continuous

    W = weights("micro")
    xa = oracle_features("micro", N_MODE)
    w = torch.linspace(0.0, 1.0, len(LENS))[:, None, None]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32, audio_ctx=N_MODE)
    f2 = m.encoder(mels()[:2].cuda())
    assert (f2.cpu() - xa).abs().max().item() < F32_TOL
    mix = ((1 - w) * xa[0:1] + w * xa[1:2]).contiguous()  # five different clips from the two, as tests/test_gpu_continuous.py mixes them
    rows = []
    with torch.no_grad():
        for i, n in enumerate(LENS):
            g = R.greedy_decode(W, MICRO, mix[i: i + 1], INIT, always, first, EOT, sample_len=n, stop_on_eot=True)
            rows.append((_cut(g.tokens[0, len(INIT):]), float(g.sum_logprobs[0]), float(g.margins.min())))
            # decided by more than twice the f32 path's logit error (2.1e-4 with split products, README): measured 1.3e-3 .. 8.8e-2
            assert rows[-1][2] > 1e-3, (i, rows[-1][2])
    stats = []
    res = decode_continuous(m, mix.cuda(), _options(), sample_lens=LENS, slots=2, check_every=4, stats_out=stats)
    assert len(res) == len(LENS) and [clip for _, clip, _ in stats[0].admissions] == list(range(len(LENS)))
    for i, (r, (ids, slp, _)) in enumerate(zip(res, rows)):
        assert r.tokens == ids, (i, r.tokens, ids)
        assert abs(r.avg_logprob * (len(r.tokens) + 1) - slp) < 1e-2
    # mels instead of features: the scheduler encodes at N
    res_m = decode_continuous(m, mels()[:2].cuda(), _options(), sample_lens=[6, 6], slots=2, check_every=4)
    alone = m.decode(f2, _options(sample_len=6))
    assert [r.tokens for r in res_m] == [r.tokens for r in alone]


# ---------------------------------------------------------------- 9. alignment at N = 75
TEXT = [[1200 + 37 * i for i in range(12)], [3400 + 91 * i for i in range(7)]]
ROWS = [[*SOT_SEQ, SP.no_timestamps, *t, EOT] for t in TEXT]
DELTA_CAP = 4 * 2.275e-5  # tests/test_gpu_alignment.py: 4 x the deviation measured for the default heads of f32 MICRO


def test_alignment_at_75_positions():
    """the weights matrix is [B, T, N]; frames asked for beyond N are clipped to N; the GPU's DTW path is the CPU's DTW
    (tests/alignment_ref.py) of the GPU's own matrix exactly, and the matrix is the float64 restatement on the oracle's scores"""
    from whisper_ipa_amd import timing

    W, xa = weights("micro"), oracle_features("micro", N_MODE)
    T = max(len(r) for r in ROWS)
    tok = torch.full((2, T), EOT, dtype=torch.long)
    for b, r in enumerate(ROWS):
        tok[b, :len(r)] = torch.tensor(r)
    with torch.no_grad():
        _, qks = AR.decoder_forward_qk(R, W, MICRO, tok, xa)
    m = _model(MICRO, W, torch.float32, audio_ctx=N_MODE)
    feats = m.encoder(mels()[:2].cuda())
    first, n_rows = len(SOT_SEQ), [len(t) + 1 for t in TEXT]
    asked, clipped = [1500, 60], [N_MODE, 60]  # 30 s of content is clipped to the 75 positions there are
    matrix, paths, probs = timing.align_tokens(m, ROWS, n_rows, first, EOT, feats, asked)
    assert tuple(matrix.shape) == (2, T, N_MODE)
    matrix = matrix.cpu().numpy()
    for b in range(2):
        nt, nf, N = len(ROWS[b]), clipped[b], n_rows[b]
        want = AR.alignment_matrix(qks, b, m.alignment_heads, nt, nf, np.float64)
        got = matrix[b, :nt, :nf]
        assert (matrix[b, nt:] == 0).all() and (matrix[b, :, nf:] == 0).all()
        delta = float(np.abs(got - want).max())
        print(f"\nclip {b}: matrix within {delta:.3e} of the restatement on the oracle's scores ({nf} frames)")
        assert delta <= DELTA_CAP, (b, delta)
        wi, wj, _, _ = AR.dtw_f32(-got[first:first + N])
        ti, tj = paths[b]
        assert np.array_equal(ti, wi) and np.array_equal(tj, wj), b
        assert tj.max() == nf - 1 and ti.max() == N - 1
        x = -want[first:first + N]
        excess = AR.path_cost(x, ti, tj) - AR.dtw_min_cost_f64(x)
        assert -1e-9 <= excess <= 2 * (N + nf - 1) * delta, (b, excess)
    # find_alignment: num_frames in mel frames, halved and clipped
    from whisper_ipa_amd.tokenizer import get_tokenizer

    words = timing.find_alignment(m, get_tokenizer(True, language="en", task="transcribe"), TEXT, feats, [3000, 120])
    assert len(words) == 2 and all(w.end <= N_MODE * 0.02 + 1e-6 for row in words for w in row)


# ---------------------------------------------------------------- 10. training at N = 300
def _train_tokens():
    rng = np.random.default_rng(5)
    sot = [50258, 50259, 50359, 50363]
    seqs = [sot + rng.integers(0, 50257, size=n).tolist() + [EOT] for n in (9, 5)]
    L = max(len(s) for s in seqs)
    return torch.tensor([s + [EOT] * (L - len(s)) for s in seqs], dtype=torch.int64)


def test_training_at_300_positions(f32_mode):
    """teacher-forced logits and loss within 1e-3 of the oracle, every decoder gradient within the relative 2e-3 of
    tests/test_gpu_training.py against the oracle's autograd on the N-row features, and one train_step with the feature cache
    bit-identical to one without; the cache's rows are (300, d)."""
    from whisper_ipa_amd.training import DecoderTrainer, FrozenFeatureCache

    W, xa, tokens = weights("micro"), oracle_features("micro", 300), _train_tokens()
    names = [k for k in W if k.startswith("decoder.")]
    leaves = {k: W[k].detach().clone().requires_grad_(True) for k in names}
    Wl = dict(W)
    Wl.update(leaves)
    ref_loss_t = R.loss_from_features(Wl, MICRO, xa, tokens, EOT)
    ref = dict(zip(names, torch.autograd.grad(ref_loss_t, [leaves[k] for k in names])))
    ref_loss = float(ref_loss_t.detach())
    with torch.no_grad():
        ref_logits = R.decoder_forward(W, MICRO, tokens[:, :-1], xa)
    split = f32_mode == "split"

    def make():
        m = _model(MICRO, {k: v.clone() for k, v in W.items()}, torch.float32, audio_ctx=300, f32_split=split)
        return m, DecoderTrainer(m, lr=1e-3)

    m, tr = make()
    mel = mels()[:2].cuda()
    feats = m.encoder(mel)
    assert (feats.cpu() - xa).abs().max().item() < F32_TOL
    logits = m.logits(tokens[:, :-1].cuda(), feats)
    assert (logits.cpu() - ref_logits).abs().max().item() < F32_TOL
    loss, _, n_valid = tr.loss_and_grads(feats, tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) < F32_TOL, (float(loss), ref_loss)
    assert int(n_valid) == int(R.loss_mask(tokens[:, 1:], EOT).sum())
    worst = ("", 0.0)
    for n in tr.names:
        a, b = tr.g(n).float().cpu(), ref[n].float()
        r = float((a - b).abs().max() / (b.abs().max() + 1e-12))
        worst = max(worst, (n, r), key=lambda t: t[1])
    print(f"\nN=300 {f32_mode}: loss {float(loss):.6f} vs {ref_loss:.6f}; worst relative gradient error {worst[1]:.2e} ({worst[0]})")
    assert worst[1] < 2e-3, worst
    with pytest.raises(Exception, match="audio"):
        tr.loss_and_grads(torch.zeros(2, 1500, 128, device="cuda"), tokens.cuda(), EOT)
    # the feature cache: rows of (300, d), more clips fit, and a cached step is the uncached step bit for bit
    m0, plain = make()
    m1, cached = make()
    cache = cached.enable_feature_cache(2)
    assert cache.row_shape == (300, 128)
    assert FrozenFeatureCache.clips_that_fit(m1) >= 4 * FrozenFeatureCache.clips_that_fit(_model(MICRO, W, torch.float32))
    for step in range(2):  # the first step fills the cache, the second reads it
        need = cache.missing([0, 1])
        assert need == ([True, True] if step == 0 else [False, False])
        l0, _ = plain.train_step(mel, tokens.cuda(), EOT)
        l1, _ = cached.train_step(mel[[i for i, f in enumerate(need) if f]] if any(need) else None, tokens.cuda(), EOT, clip_keys=[0, 1])
        torch.cuda.synchronize()
        assert float(l0) == float(l1)
        assert torch.equal(plain.flat_g, cached.flat_g) and torch.equal(plain.flat_p, cached.flat_p)
    assert tuple(cache.store.shape[1:]) == (300, 128)
    # changing the context drops the cached rows and their buffer
    m1.audio_ctx = 75
    assert cache.missing([0, 1]) == [True, True] and cache.row_shape == (75, 128) and cache.store is None


# ---------------------------------------------------------------- 11. fp8 at N = 300
def test_fp8_weight_model_at_300_positions():
    """tests/test_gpu_model.py::test_fp8_weight_model_matches_dequantised_reference (small width) at N = 300: against the same model
    on the dequantised bf16 weights and against the f32 oracle on them"""
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    W = R.synthetic_weights(SMALL2, seed=31)
    m8 = _model(SMALL2, W, torch.bfloat16, audio_ctx=300)
    m8.quantize_weights("fp8_e4m3")
    assert m8.weights_format == "fp8_e4m3" and m8.packed()["cfg"].dec_w_dtype == 2 and m8.packed()["cfg"].n_audio_ctx == 300
    Wdq = {k: v.float().cpu() for k, v in m8.flat_parameters().items()}
    mref = _model(SMALL2, Wdq, torch.bfloat16, audio_ctx=300)
    mel = mels()[:2].cuda()
    f8, fr = m8.encoder(mel), mref.encoder(mel)
    assert torch.equal(f8, fr)
    always, first = R.suppress_lists(SP)
    a = greedy_decode_tokens(m8, f8, INIT, always, first, EOT, max_new_tokens=12, stop_on_eot=False)
    b = greedy_decode_tokens(mref, fr, INIT, always, first, EOT, max_new_tokens=12, stop_on_eot=False)
    same = np.cumprod(a.tokens == b.tokens, axis=1).astype(bool)
    assert same[:, : 4 + 4].all(), (a.tokens.tolist(), b.tokens.tolist())
    if same.all():
        assert (a.last_logits.float() - b.last_logits.float()).abs().max().item() < 0.15
    toks = torch.from_numpy(a.tokens[:, :8]).cuda()
    assert torch.equal(m8.logits(toks, f8), mref.logits(toks, fr))
    with torch.no_grad():
        xa = R.encoder_forward(Wdq, SMALL2, mels()[:2, :600])
        ref = R.greedy_decode(Wdq, SMALL2, xa, INIT, always, first, EOT, sample_len=12, stop_on_eot=False, keep_logits=True)
    assert ((f8.float().cpu() - xa).abs().max() / xa.abs().max()).item() < 5e-2
    check_low_precision_decode(m8, f8, ref, INIT, always, first, EOT, "fp8 weights, small width, N=300")


def test_fp8_activation_encoder_at_300_positions():
    """tests/test_gpu_model.py::test_fp8_activation_encoder_on_the_fp8_mfma (small width) at N = 300: the fp8 x fp8 tile GEMM serves
    the M = B N rows, and the features stand to the emulated arithmetic and to the bf16-activation model as they do at 1500"""
    import torch.nn.functional as F

    from whisper_ipa_amd import ops
    from whisper_ipa_amd.whisper import dequantize_fp8_e4m3, quantize_fp8_e4m3

    dims = SMALL2
    W = R.synthetic_weights(dims, seed=33)
    mb = _model(dims, W, torch.bfloat16, audio_ctx=300)
    mb.quantize_weights("fp8_e4m3")
    m8 = _model(dims, W, torch.bfloat16, audio_ctx=300)
    m8.quantize_weights("fp8_e4m3", activations="fp8")
    assert m8.packed()["cfg"].enc_act_fp8 == 1 and m8.packed()["cfg"].n_audio_ctx == 300
    mel = mels()[:2].cuda()
    ops.gemm_dispatch_counts(reset=True)
    f8 = m8.encoder(mel)
    assert ops.gemm_dispatch_counts(reset=True)["tile_fp8"] == 4 * dims.n_audio_layer
    fb = mb.encoder(mel)
    assert tuple(f8.shape) == (2, 300, 768)
    Wdq = {k: v.float().cpu() for k, v in m8.flat_parameters().items()}

    def q8(t):
        shp = t.shape
        c, s = quantize_fp8_e4m3(t.reshape(-1, shp[-1]))
        return dequantize_fp8_e4m3(c, s).reshape(shp)

    def emulated_encoder(mel_t):
        x = mel_t.transpose(1, 2)
        x = F.gelu(F.conv1d(x, Wdq["encoder.conv1.weight"].permute(0, 2, 1), Wdq["encoder.conv1.bias"], padding=1))
        x = F.gelu(F.conv1d(x, Wdq["encoder.conv2.weight"].permute(0, 2, 1), Wdq["encoder.conv2.bias"], stride=2, padding=1))
        x = x.transpose(1, 2)
        x = x + R.sinusoids(dims.n_audio_ctx, dims.n_audio_state)[: x.shape[1]]
        H = dims.n_audio_head
        for i in range(dims.n_audio_layer):
            p = f"encoder.blocks.{i}"
            h = q8(R._layer_norm(x, Wdq, p + ".attn_ln"))
            q = F.linear(h, Wdq[p + ".attn.query.weight"], Wdq[p + ".attn.query.bias"])
            k = F.linear(h, Wdq[p + ".attn.key.weight"])
            v = F.linear(h, Wdq[p + ".attn.value.weight"], Wdq[p + ".attn.value.bias"])
            B_, T_, D_ = q.shape
            sc = (D_ // H) ** -0.25
            qh = q.view(B_, T_, H, -1).permute(0, 2, 1, 3) * sc
            kh = k.view(B_, T_, H, -1).permute(0, 2, 3, 1) * sc
            a = (torch.softmax(qh @ kh, -1) @ v.view(B_, T_, H, -1).permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B_, T_, D_)
            x = x + F.linear(a, Wdq[p + ".attn.out.weight"], Wdq[p + ".attn.out.bias"])
            h = q8(R._layer_norm(x, Wdq, p + ".mlp_ln"))
            u = q8(F.gelu(F.linear(h, Wdq[p + ".mlp1.weight"], Wdq[p + ".mlp1.bias"])))
            x = x + F.linear(u, Wdq[p + ".mlp2.weight"], Wdq[p + ".mlp2.bias"])
        return R._layer_norm(x, Wdq, "encoder.ln_post")

    with torch.no_grad():
        xa8 = emulated_encoder(mels()[:2, :600])
    rel_emul = ((f8.float().cpu() - xa8).abs().max() / xa8.abs().max()).item()
    rms_emul = ((f8.float().cpu() - xa8).pow(2).mean().sqrt() / xa8.pow(2).mean().sqrt()).item()
    rms_vs_bf16 = ((f8.float() - fb.float()).pow(2).mean().sqrt() / fb.float().pow(2).mean().sqrt()).item()
    print(f"\nfp8 activations, N=300: vs the emulated arithmetic {rel_emul:.3e} max / {rms_emul:.3e} rms; vs the bf16-activation model rms {rms_vs_bf16:.3e}")
    assert rms_emul < 1.5 * rms_vs_bf16 and rms_emul < 0.08 and rel_emul < 0.15, (rms_emul, rms_vs_bf16, rel_emul)  # the bounds at 1500
    assert rms_vs_bf16 < 0.15, rms_vs_bf16


# ---------------------------------------------------------------- cross_attention="auto" at a short context
def test_auto_takes_the_cached_form_up_to_300_positions():
    """the rule of Whisper.use_absorbed: measured at 300 and 750 keys (profiles/audio_ctx_bench.txt); nothing moves without audio_ctx"""
    m = _model(SMALL2, weights("small2"), torch.bfloat16)
    assert m.use_absorbed(64, 64) and m.use_absorbed() and not m.use_absorbed(64, 224)
    for n, want in ((1500, True), (750, True), (301, True), (300, False), (75, False)):
        m.audio_ctx = n
        assert m.use_absorbed(64, 64) is want and m.use_absorbed() is want, n
        assert m.packed()["cfg"].dec_cross_absorbed == int(want)
    m.cross_attention = "absorbed"  # forcing a form still works
    assert m.use_absorbed(64, 64)
    m.audio_ctx = None
    m.cross_attention = "auto"
    assert m.use_absorbed(64, 64)


# ---------------------------------------------------------------- 12. refusals, and the setter
def test_refusals_and_the_audio_ctx_setter():
    import ctypes as C

    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    W = weights("micro")
    for bad in (0, 1501, -3, 2.5, True):
        with pytest.raises(_lib.WipaError, match="audio_ctx"):
            _model(MICRO, W, torch.float32, audio_ctx=bad)
    m = _model(MICRO, W, torch.float32, audio_ctx=75)
    for bad in (0, 1501):
        with pytest.raises(_lib.WipaError, match="audio_ctx"):
            m.audio_ctx = bad
    assert m.audio_ctx == 75
    # the native layer, by name and with the bound
    for bad in (0, 1501):
        cfg = type(m.packed()["cfg"]).from_buffer_copy(m.packed()["cfg"])
        cfg.n_audio_ctx = bad
        assert _lib.lib().wipa_decoder_layout(C.byref(cfg), 2, C.byref(_lib.DecLayout())) != 0
        msg = _lib.lib().wipa_last_error()
        assert b"n_audio_ctx" in msg and b"1500" in msg
        fake = C.c_void_p(0x1000)  # never dereferenced: cfg_check comes first
        assert _lib.lib().wipa_encoder_forward(C.byref(cfg), m.packed()["enc_tab"], fake, fake, fake, 1 << 40, 2, None) != 0
        assert b"n_audio_ctx" in _lib.lib().wipa_last_error()
    # transcribe() is refused by name before any work
    with pytest.raises(NotImplementedError, match="audio_ctx"):
        wipa.transcribe(m, np.zeros(16000, dtype=np.float32), language="en")
    with pytest.raises(NotImplementedError, match="audio_ctx"):
        wipa.transcribe(m, "/nonexistent.wav", language="en", schedule="continuous")
    # features of the wrong length: the full-context ones, and the right length of another N
    always, first = R.suppress_lists(SP)
    mel = mels()[:2].cuda()
    f75 = m.encoder(mel)
    full = torch.zeros(2, 1500, 128, device="cuda")
    for wrong in (full, full[:, :300].contiguous()):
        with pytest.raises(_lib.WipaError, match="audio"):
            wipa.decode(m, wrong, _options())
        with pytest.raises(_lib.WipaError, match="audio"):
            greedy_decode_tokens(m, wrong, INIT, always, first, EOT, max_new_tokens=4)
        with pytest.raises(_lib.WipaError, match="audio"):
            m.logits(torch.tensor([INIT, INIT]).cuda(), wrong)
        with pytest.raises(_lib.WipaError, match="audio"):
            wipa.decode_continuous(m, wrong, _options())
    with pytest.raises(_lib.WipaError, match="mel"):
        m.embed_audio(mel[:, :300].contiguous())  # neither 3000 nor 2N frames
    # the setter: everything sized by N is made again, and going back gives the same bits
    base = greedy_decode_tokens(m, f75, INIT, always, first, EOT, max_new_tokens=8, stop_on_eot=False)
    t75, l75 = base.tokens.copy(), base.last_logits.clone()
    m.audio_ctx = 300
    assert m.packed()["cfg"].n_audio_ctx == 300 and not m._enc_ws
    f300 = m.encoder(mel)
    assert tuple(f300.shape) == (2, 300, 128) and (f300.cpu() - oracle_features("micro", 300)).abs().max().item() < F32_TOL
    ref = oracle_greedy("micro", 300, 24)
    r300 = greedy_decode_tokens(m, f300, INIT, always, first, EOT, max_new_tokens=24, stop_on_eot=False)
    assert (r300.tokens == ref.tokens).all()
    with pytest.raises(_lib.WipaError, match="audio"):
        greedy_decode_tokens(m, f75, INIT, always, first, EOT, max_new_tokens=4)
    m.audio_ctx = None
    assert m.n_audio_ctx == 1500 and tuple(m.encoder(mel).shape) == (2, 1500, 128)
    m.audio_ctx = 75
    again = greedy_decode_tokens(m, m.encoder(mel), INIT, always, first, EOT, max_new_tokens=8, stop_on_eot=False)
    assert (again.tokens == t75).all() and torch.equal(again.last_logits, l75)
    # load_model carries the setting
    import tempfile

    from whisper_ipa_amd.load_models import load_model, save_model

    with tempfile.TemporaryDirectory() as d:
        save_model(m, d)
        assert load_model(d).audio_ctx is None and load_model(d, audio_ctx=300).n_audio_ctx == 300
