"""Per-row adapters in one decode batch (Whisper.set_adapter_bank + row_adapters; csrc/lora_bank.hip behind the decode step) against the
CPU oracle run on lora.merged_weights of every row's own adapter.  ``pytest -m gpu``.

The MICRO float32 model (the weights tests/golden/micro_model.npz was made from), six rows with the ids [0, 1, -1, 2, 1, 0] over a bank of
three adapters with non-zero lora_B: rank 4 on (query, value) and rank 8 on all six targets.  The oracle's results are computed once per
bank and shared.  Bounds: LOGIT_BOUND is the bound tests/test_gpu_lora_training.py holds the logits of a merged adapter to; greedy ids
are compared wherever the oracle's top-2 margin exceeds twice that, which the recorded adapter seeds satisfy on at least nine (row,
step) pairs in ten (asserted on the oracle's margins before anything is compared)."""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")
IDS = (0, 1, -1, 2, 1, 0)
NAMES = ("tr", "de", "ku")
LOGIT_BOUND = 1e-3  # test_gpu_lora_training.py: merged logits against the oracle on W + s B A
STEPS = 12
# (rank, targets) -> the seeds of the three adapters (lora_A from LoRAConfig.seed, lora_B from the same seed): chosen on the CPU so that
# the oracle's own top-2 margins exceed 2 * LOGIT_BOUND on at least 9 (row, step) pairs in 10
BANKS = {"r4-qv": (4, ("query", "value"), (11, 12, 13)), "r8-all": (8, ALL, (21, 22, 23))}
ALPHAS = (16.0, 8.0, 24.0)  # a different gain for every adapter


def _sp():
    sp = R.SpecialTokens.multilingual()
    always, first = R.suppress_lists(sp)
    return sp, always, first, list(sp.sot_sequence_including_notimestamps(0))


@functools.lru_cache(maxsize=None)
def _inputs():
    W = R.synthetic_weights(MICRO, seed=7)
    torch.manual_seed(0)
    xa = torch.randn(len(IDS), 1500, 128) * 0.7
    return W, xa


@functools.lru_cache(maxsize=None)
def _adapters(key):
    """name -> (adapter tensors, LoRAConfig), in NAMES order"""
    from whisper_ipa_amd import lora

    rank, targets, seeds = BANKS[key]
    out = {}
    for name, seed, alpha in zip(NAMES, seeds, ALPHAS):
        cfg = lora.LoRAConfig(rank=rank, alpha=alpha, targets=targets, seed=seed)
        g = torch.Generator().manual_seed(seed)
        out[name] = ({n: (t if n.endswith("lora_A") else 0.2 * torch.randn(t.shape, generator=g)) for n, t in lora.init_adapter(MICRO, cfg).items()}, cfg)
    return out


def _weights_of(key, i):
    from whisper_ipa_amd import lora

    W, _ = _inputs()
    if i < 0:
        return W
    ad, cfg = _adapters(key)[NAMES[i]]
    return lora.merged_weights(W, ad, cfg)


@functools.lru_cache(maxsize=None)
def _oracle(key, ids=IDS):
    """the oracle's greedy decode of every row under its own merged weights -> (tokens [B, n_init + STEPS], margins [B, STEPS], sum_logprobs)"""
    _, xa = _inputs()
    sp, always, first, init = _sp()
    toks, margins, slp = [None] * len(ids), [None] * len(ids), [None] * len(ids)
    with torch.no_grad():
        for i in sorted(set(ids)):
            rows = [b for b, v in enumerate(ids) if v == i]
            g = R.greedy_decode(_weights_of(key, i), MICRO, xa[rows], init, always, first, sp.eot, sample_len=STEPS, stop_on_eot=False)
            for j, b in enumerate(rows):
                toks[b], margins[b], slp[b] = g.tokens[j], g.margins[j], g.sum_logprobs[j]
    return np.stack(toks), np.stack(margins), np.asarray(slp)


def _gate(key, ids=IDS):
    """(row, step) pairs the oracle decides by more than twice the logit bound, while the row's history is still the oracle's"""
    _, margins, _ = _oracle(key, ids)
    gate = np.cumprod(margins > 2 * LOGIT_BOUND, axis=1).astype(bool)
    assert gate.mean() >= 0.9, f"{key}: the oracle's own margins exclude {1 - gate.mean():.0%} of the (row, step) pairs: pick other adapter seeds"
    return gate


def _model(key, dtype=torch.float32):
    from whisper_ipa_amd import lora
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    W, _ = _inputs()
    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=dtype, f32_split=False)
    m.load_weights({k: v.clone() for k, v in W.items()})
    m.set_adapter_bank(lora.AdapterBank(m.dims, _adapters(key)))
    return m


def _decode(m, ids, **kw):
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    _, xa = _inputs()
    sp, always, first, init = _sp()
    return greedy_decode_tokens(m, xa.cuda(), init, always, first, sp.eot, max_new_tokens=STEPS, stop_on_eot=False, row_ids=list(ids), **kw)


def _check_ids(key, got, ids=IDS):
    want, _, _ = _oracle(key, ids)
    gate = _gate(key, ids)
    n_init = want.shape[1] - STEPS
    assert got.shape == want.shape and (got[:, :n_init] == want[:, :n_init]).all()
    bad = (got[:, n_init:] != want[:, n_init:]) & gate
    assert not bad.any(), (key, np.argwhere(bad).tolist(), got.tolist(), want.tolist())


@pytest.mark.parametrize("key", sorted(BANKS))
def test_teacher_forced_logits_per_row_match_the_oracle_on_each_rows_merged_weights(key):
    from whisper_ipa_amd.decoding import forced_decode_logits

    W, xa = _inputs()
    sp, always, first, init = _sp()
    rng = np.random.default_rng(5)
    tokens = np.concatenate([np.tile(np.asarray(init), (len(IDS), 1)), rng.integers(0, 50257, size=(len(IDS), 8))], axis=1)
    m = _model(key)
    trace, _ = forced_decode_logits(m, xa.cuda(), tokens, len(init), always, first, sp.eot, row_ids=list(IDS))
    base, _ = forced_decode_logits(m, xa.cuda(), tokens, len(init), always, first, sp.eot)
    got, got_base = trace.cpu().numpy(), base.cpu().numpy()
    errs, moved = [], []
    with torch.no_grad():
        for b, i in enumerate(IDS):
            ref = R.decoder_forward(_weights_of(key, i), MICRO, torch.from_numpy(tokens[b:b + 1, :-1]), xa[b:b + 1])[0, len(init) - 1:].numpy()
            errs.append(float(np.abs(got[b] - ref).max()))
            moved.append(float(np.abs(got[b] - got_base[b]).max()))
    print(f"\n{key}: per-row logit error against the oracle {['%.1e' % e for e in errs]}; moved by the adapter {['%.1e' % v for v in moved]}")
    assert max(errs) < LOGIT_BOUND, errs
    for b, i in enumerate(IDS):  # a -1 row is the base model (whose call fuses the cross block: not the same bits); an adapted row is far from it
        assert (moved[b] > 20 * LOGIT_BOUND) if i >= 0 else (moved[b] < LOGIT_BOUND), (b, i, moved[b])


@pytest.mark.parametrize("key", sorted(BANKS))
def test_greedy_ids_per_row_and_one_graph_for_every_assignment(key):
    """greedy ids of the mixed batch; then ANOTHER assignment on the same state (the replayed step graph reads the ids from the device:
    the library's graph count does not grow), then the first one again without graphs: all three are the oracle's, and eager equals
    replayed."""
    from whisper_ipa_amd import _lib

    m = _model(key)
    a = _decode(m, IDS)
    _check_ids(key, a.tokens)
    graphs = _lib.lib().wipa_decoder_graph_count()
    assert graphs >= 2  # the prompt pass and the step
    other = (2, 2, 0, -1, 0, 1)
    b = _decode(m, other)
    _check_ids(key, b.tokens, other)
    assert _lib.lib().wipa_decoder_graph_count() == graphs, "another assignment of adapters to rows captured a graph of its own"
    assert (a.tokens != b.tokens).any()
    c = _decode(m, IDS, use_graph=False)
    assert (c.tokens == a.tokens).all() and np.array_equal(c.sum_logprobs, a.sum_logprobs)
    want, _, slp = _oracle(key)
    assert np.abs(a.sum_logprobs - slp)[_gate(key).all(axis=1)].max() < 1e-2
    base = _decode(m, (-1,) * len(IDS))
    assert (base.tokens != a.tokens).any(), "the adapters do not change the greedy ids: the check is vacuous"


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "t0.6-seed3"])
@pytest.mark.parametrize("key", sorted(BANKS))
def test_a_row_does_not_depend_on_the_other_rows_adapters_bit_for_bit(key, sampled):
    from whisper_ipa_amd.decoding import Sampling

    m = _model(key)
    kw = dict(sample=Sampling(3, 0.6)) if sampled else {}
    mixed = _decode(m, IDS, **kw)
    for i in sorted(set(IDS)):
        uniform = _decode(m, (i,) * len(IDS), **kw)
        rows = [b for b, v in enumerate(IDS) if v == i]
        assert (mixed.tokens[rows] == uniform.tokens[rows]).all(), (key, i)
        assert mixed.sum_logprobs[rows].tobytes() == uniform.sum_logprobs[rows].tobytes(), (key, i)


def test_decode_options_row_adapters_best_of_timestamps_and_the_refusals():
    """decode() with row_adapters: names map to ids per clip, best_of candidates share their clip's adapter, the timestamp path runs;
    what is not served is refused by name"""
    from whisper_ipa_amd import _lib, lora
    from whisper_ipa_amd.decoding import DecodingOptions, decode

    key = "r8-all"
    m = _model(key)
    _, xa = _inputs()
    feats = xa.cuda()
    names = [None if i < 0 else NAMES[i] for i in IDS]
    opt = DecodingOptions(language="en", without_timestamps=True, sample_len=STEPS, fp16=False, row_adapters=names)
    res = decode(m, feats, opt)
    want, _, _ = _oracle(key)
    gate = _gate(key)
    sp = R.SpecialTokens.multilingual()
    for b, r in enumerate(res):
        w = want[b, -STEPS:].tolist()
        w = w[: w.index(sp.eot)] if sp.eot in w else w
        n = min(len(w), int(gate[b].sum())) if not gate[b].all() else len(w)
        assert r.tokens[:n] == w[:n], (b, r.tokens, w)
    # one adapter for every clip == the same decode through set_adapter's merged weights is the oracle's business (above); here: best_of
    # and the timestamp rules run with a bank and depend on the adapter
    kw = dict(language="en", sample_len=STEPS, fp16=False)
    for extra in (dict(without_timestamps=True, temperature=0.6, seed=3, best_of=2), dict(without_timestamps=False)):
        with_bank = decode(m, feats, DecodingOptions(**kw, **extra, row_adapters=names))
        without = decode(m, feats, DecodingOptions(**kw, **extra))
        uniform = decode(m, feats, DecodingOptions(**kw, **extra, row_adapters=[names[0]] * len(IDS)))
        assert with_bank[0].tokens == uniform[0].tokens and with_bank[5].tokens == uniform[5].tokens
        assert any(a.tokens != b.tokens for a, b in zip(with_bank, without))
    with pytest.raises(ValueError, match="row_adapters: 2 names for 6 clips"):
        decode(m, feats, DecodingOptions(**kw, row_adapters=["tr", None]))
    with pytest.raises(_lib.WipaError, match="no adapter 'fr' in the bank"):
        decode(m, feats, DecodingOptions(**kw, row_adapters=["fr"] * 6))
    with pytest.raises(NotImplementedError, match="row_adapters with beam_size"):
        decode(m, feats, DecodingOptions(**kw, beam_size=2, row_adapters=names))
    ad, cfg = _adapters(key)["tr"]
    with pytest.raises(_lib.WipaError, match="set_adapter while an adapter bank is set"):
        m.set_adapter(ad, cfg)
    m.set_adapter_bank(None)
    with pytest.raises(_lib.WipaError, match="row_adapters needs an adapter bank"):
        decode(m, feats, DecodingOptions(**kw, row_adapters=names))
    m.set_adapter(ad, cfg)
    with pytest.raises(_lib.WipaError, match="set_adapter_bank while an adapter is applied"):
        m.set_adapter_bank(lora.AdapterBank(m.dims, _adapters(key)))
    m.set_adapter(None)


@pytest.mark.parametrize("key", sorted(BANKS))
def test_rows_with_their_own_prompts_decode_under_their_own_adapters(key):
    """decode(prompts=[ids per row], row_adapters=...): the ragged prompt pass and the ragged steps carry the bank.  Every row against the
    oracle's greedy decode of that row's initial tokens ([sot_prev] + prompt + sot sequence) on that row's merged weights, wherever the
    oracle's margin exceeds twice the logit bound; and bit for bit against the same batch with every row on that row's adapter.  A
    common ``prompt`` and a ``prefix`` go the same way."""
    from whisper_ipa_amd.decoding import DecodingOptions, _suppress_lists, decode, initial_tokens
    from whisper_ipa_amd.tokenizer import get_tokenizer

    m = _model(key)
    _, xa = _inputs()
    tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    rng = np.random.default_rng(8)
    prompts = [rng.integers(1000, 40000, size=n).tolist() for n in (5, 0, 17, 3, 30, 9)]  # ragged, one row without a prompt
    names = [None if i < 0 else NAMES[i] for i in IDS]
    kw = dict(language="en", without_timestamps=True, sample_len=STEPS, fp16=False)
    got = decode(m, xa.cuda(), DecodingOptions(**kw, prompts=prompts, row_adapters=names))
    base = decode(m, xa.cuda(), DecodingOptions(**kw, prompts=prompts))
    opt = DecodingOptions(**kw)
    always_d, first_d = _suppress_lists(opt, tok)
    excluded = total = 0
    with torch.no_grad():
        for b, i in enumerate(IDS):
            row = initial_tokens(tok, list(tok.sot_sequence_including_notimestamps), prompts[b] or None, None, MICRO.n_text_ctx, STEPS)
            ref = R.greedy_decode(_weights_of(key, i), MICRO, xa[b:b + 1], row, always_d, first_d, tok.eot, sample_len=STEPS, stop_on_eot=False)
            gate = np.cumprod(ref.margins[0] > 2 * LOGIT_BOUND).astype(bool)
            want = ref.tokens[0, len(row):].tolist()
            want = want[: want.index(tok.eot)] if tok.eot in want else want
            n = min(len(want), int(gate.sum()))
            excluded, total = excluded + (len(want) - n), total + len(want)
            assert got[b].tokens[:n] == want[:n], (key, b, got[b].tokens, want)
    assert excluded <= total // 10, (excluded, total)
    assert any(a.tokens != c.tokens for a, c in zip(got, base)), "the adapters do not show in the ids"
    for i in sorted(set(IDS)):
        uniform = decode(m, xa.cuda(), DecodingOptions(**kw, prompts=prompts, row_adapters=[None if i < 0 else NAMES[i]] * len(IDS)))
        for b in [b for b, v in enumerate(IDS) if v == i]:
            assert got[b].tokens == uniform[b].tokens and got[b].avg_logprob == uniform[b].avg_logprob, (key, i, b)
    both = decode(m, xa.cuda(), DecodingOptions(**kw, prompt=prompts[0], prefix=[300, 400], row_adapters=names))
    plain = decode(m, xa.cuda(), DecodingOptions(**kw, prompt=prompts[0], prefix=[300, 400]))
    assert len(both) == len(IDS) and any(a.tokens != c.tokens for a, c in zip(both, plain))


def test_transcribe_row_adapters_per_file_equal_each_file_alone_under_set_adapter():
    """transcribe(row_adapters=[per file]) on the rounds schedule, a 70 s and a 40 s file on two adapters, with conditioning on previous
    text (every window carries its file's adapter AND its file's prompt): the segments are those of each file transcribed alone on a
    model with that adapter merged (set_adapter).  The MICRO model's margins (at least 5e-3 on the oracle's decodes above) are far above
    the 8e-6 the two paths' logits differ by, so the tokens are compared outright.  Refused by name: the continuous schedule, word
    timestamps, a custom decode_fn, a count that differs from the files'."""
    import warnings

    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import _lib

    key = "r8-all"
    m = _model(key)
    clips = [np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0), R.synthetic_clip(1, 10.0)[: 10 * 16000]]),
             np.concatenate([R.synthetic_clip(1, 30.0), R.synthetic_clip(0, 10.0)[: 10 * 16000]])]
    files = ["de", "tr"]
    kw = dict(language="en", sample_len=STEPS, fp16=False, no_speech_threshold=None, condition_on_previous_text=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        got = wipa.transcribe(m, clips, row_adapters=files, **kw)
        plain = wipa.transcribe(m, clips, **kw)
        for i, name in enumerate(files):
            alone = _model(key)
            alone.set_adapter_bank(None)
            alone.set_adapter(*_adapters(key)[name])
            want = wipa.transcribe(alone, clips[i], **kw)
            have = [(s["seek"], s["start"], s["end"], s["tokens"]) for s in got[i]["segments"]]
            assert have == [(s["seek"], s["start"], s["end"], s["tokens"]) for s in want["segments"]], (i, name)
            assert len({s["seek"] for s in got[i]["segments"]}) >= 2  # more than one window: the later ones carry a prompt
            assert [s["tokens"] for s in got[i]["segments"]] != [s["tokens"] for s in plain[i]["segments"]], "the adapter does not show"
    with pytest.raises(NotImplementedError, match="schedule='continuous'.: row_adapters is not implemented"):
        wipa.transcribe(m, clips, row_adapters=files, schedule="continuous", **kw)
    with pytest.raises(NotImplementedError, match="word_timestamps=True with row_adapters"):
        wipa.transcribe(m, clips, row_adapters=files, word_timestamps=True, **kw)
    with pytest.raises(NotImplementedError, match="a custom decode_fn takes no row_adapters"):
        wipa.transcribe(m, clips, row_adapters=files, decode_fn=lambda *a, **k: [], **kw)
    with pytest.raises(ValueError, match="row_adapters holds 1 names for 2 files"):
        wipa.transcribe(m, clips, row_adapters=["de"], **kw)
    with pytest.raises(_lib.WipaError, match="no adapter 'fr' in the bank"):
        wipa.transcribe(m, clips, row_adapters=["de", "fr"], **kw)


@pytest.mark.parametrize("key", sorted(BANKS))
def test_decode_continuous_nine_clips_through_four_slots_keep_their_adapters(key):
    """ids cycling over the three adapters and -1: every clip's tokens equal those of the lockstep decode() under the same adapter (which
    the tests above hold to the oracle) -- a slot whose id or cross K / V term is not renewed on admission decodes another model"""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import DecodingOptions, decode

    m = _model(key)
    torch.manual_seed(2)
    feats = (torch.randn(9, 1500, 128) * 0.7).cuda()
    names = [(NAMES + (None,))[i % 4] for i in range(9)]
    lens = [5, 12, 7, 9, 12, 6, 10, 8, 11]  # the slots free up at different steps
    opt = DecodingOptions(language="en", without_timestamps=True, sample_len=STEPS, fp16=False)
    stats = []
    got = decode_continuous(m, feats, opt, slots=4, sample_lens=lens, check_every=2, row_adapters=names, stats_out=stats)
    want = decode(m, feats, opt, row_adapters=names)
    base = decode(m, feats, opt)
    for i in range(9):
        assert got[i].tokens == want[i].tokens[: lens[i]], (i, names[i], got[i].tokens, want[i].tokens)
    assert sum(got[i].tokens != base[i].tokens[: lens[i]] for i in range(9) if names[i] is not None) >= 5, "the adapters do not show in the ids"
    # a prompt per clip: the prompted admission runs the clip's prompt pass under its adapter (ragged lengths, two clips without one)
    rng = np.random.default_rng(4)
    prompts = [rng.integers(1000, 40000, size=n).tolist() for n in (6, 0, 11, 3, 0, 20, 1, 8, 5)]
    got_p = decode_continuous(m, feats, opt, slots=4, sample_lens=lens, check_every=2, row_adapters=names, prompts=prompts)
    want_p = decode(m, feats, opt, row_adapters=names, prompts=prompts)
    base_p = decode(m, feats, opt, prompts=prompts)
    for i in range(9):
        assert got_p[i].tokens == want_p[i].tokens[: lens[i]], (i, names[i], got_p[i].tokens, want_p[i].tokens)
    assert sum(got_p[i].tokens != base_p[i].tokens[: lens[i]] for i in range(9) if names[i] is not None) >= 5
    assert any(got_p[i].tokens != got[i].tokens for i in range(9) if prompts[i])
    with pytest.raises(ValueError, match="row_adapters: 2 names for 9 clips"):
        decode_continuous(m, feats, opt, slots=4, row_adapters=["tr", None])


def test_cross_kv_terms_by_slot_equal_those_of_the_whole_batch():
    """wipa_decoder_adapt_cross with a list of slots (what an admission calls) leaves the cached cross K / V of those slots with the bits
    the all-clips call leaves"""
    import ctypes as C

    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import _open, _begin_with, _packed_for, _state_for, _bank_of
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    key = "r8-all"
    m = _model(key)
    _, xa = _inputs()
    _, _, _, init = _sp()
    L, B = _lib.lib(), len(IDS)
    pk = _packed_for(m, B, STEPS)
    assert not pk["cfg"].dec_cross_absorbed
    with on_stream() as s:
        st = _state_for(m, B, pk)
        bank = _bank_of(m, st, list(IDS))
        lay = st.layout
        ckv = st.blob[lay.cross_kv: lay.self_kv]
        feats, _ = _open(m, L, pk, st, xa.cuda(), B, s, _begin_with(init))
        plain = ckv.clone()
        feats, _ = _open(m, L, pk, st, xa.cuda(), B, s, _begin_with(init), bank)
        whole = ckv.clone()
        feats, _ = _open(m, L, pk, st, xa.cuda(), B, s, _begin_with(init))
        slots = (C.c_int32 * 3)(4, 0, 2)
        sub = feats[[4, 0, 2]].contiguous()
        _lib.check(L.wipa_decoder_adapt_cross(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, ptr(sub), 3, slots, C.byref(bank),
                                              sptr(s)), "wipa_decoder_adapt_cross")
        by_slot = ckv.clone()
    torch.cuda.synchronize()
    d, H, Ta, nl = 128, 2, 1500, 2
    v = lambda t: t.view(torch.float32).view(nl, B, 2 * H * Ta * 64)
    for b in range(B):
        want = whole if b in (4, 0) else plain  # slot 2 carries id -1: its bytes are left alone either way
        assert torch.equal(v(by_slot)[:, b], v(want)[:, b]), b
    assert not torch.equal(v(whole)[:, 0], v(plain)[:, 0]) and torch.equal(v(whole)[:, 2], v(plain)[:, 2])


def test_absorbed_form_serves_a_bank_off_the_cross_kv_sites_and_refuses_one_on_them():
    """bf16, whisper-small width (eligible for the absorbed form): a bank on attn.query, attn.value, cross_attn.query, mlp1 decodes on the
    absorbed form, rows independent bit for bit; a bank that includes cross_attn.value resolves "auto" to cached, and "absorbed" raises"""
    from whisper_ipa_amd import _lib, lora
    from whisper_ipa_amd.decoding import greedy_decode_tokens
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    dims = R.ModelDimensions(80, 1500, 768, 12, 1, 51865, 448, 768, 12, 1)  # WIDE "small1" of tests/golden/wide_model.npz
    W = R.synthetic_weights(dims, seed=41)
    torch.manual_seed(1)
    xa = (torch.randn(4, 1500, 768) * 0.7).cuda()
    sp, always, first, init = _sp()

    def bank_on(targets):
        out = {}
        for name, seed in zip(NAMES, (31, 32, 33)):
            cfg = lora.LoRAConfig(rank=8, alpha=16.0, targets=targets, seed=seed)
            g = torch.Generator().manual_seed(seed)
            out[name] = ({n: (t if n.endswith("lora_A") else 0.2 * torch.randn(t.shape, generator=g)) for n, t in lora.init_adapter(dims, cfg).items()}, cfg)
        return out

    def model(cross_attention):
        m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.bfloat16, cross_attention=cross_attention)
        m.load_weights({k: v.clone() for k, v in W.items()})
        return m

    m = model("absorbed")
    m.set_adapter_bank(lora.AdapterBank(m.dims, bank_on(("attn.query", "attn.value", "cross_attn.query", "mlp1"))))
    assert m.use_absorbed(4, 8)
    ids = (0, -1, 2, 1)
    dec = lambda ids: greedy_decode_tokens(m, xa, init, always, first, sp.eot, max_new_tokens=8, stop_on_eot=False, row_ids=list(ids))
    mixed, base = dec(ids), dec((-1,) * 4)
    for i in sorted(set(ids)):
        uniform = dec((i,) * 4)
        rows = [b for b, v in enumerate(ids) if v == i]
        assert (mixed.tokens[rows] == uniform.tokens[rows]).all() and mixed.sum_logprobs[rows].tobytes() == uniform.sum_logprobs[rows].tobytes()
    assert (mixed.tokens != base.tokens).any() or not np.array_equal(mixed.sum_logprobs, base.sum_logprobs)
    kv_bank = lora.AdapterBank(m.dims, bank_on(("attn.query", "cross_attn.value")))
    m.set_adapter_bank(kv_bank)
    with pytest.raises(_lib.WipaError, match="cross_attention='absorbed' with an adapter bank on cross_attn.key / cross_attn.value"):
        dec(ids)
    auto = model("auto")
    assert auto.use_absorbed(4, 8)
    auto.set_adapter_bank(lora.AdapterBank(auto.dims, bank_on(("attn.query", "cross_attn.value"))))
    assert not auto.use_absorbed(4, 8)
    got = greedy_decode_tokens(auto, xa, init, always, first, sp.eot, max_new_tokens=8, stop_on_eot=False, row_ids=list(ids))
    assert got.tokens.shape == mixed.tokens.shape


# bf16: max|logit - oracle| / rms(oracle logits) of teacher-forced decode-step logits on the WIDE "small1" model.  The bank's path adds one
# bf16 rounding per adapted bf16 output (and, at mlp1, one of the pre-activation) to the base decode's bf16 error and nothing else, so the
# bound is twice the BASE decode's error against the oracle, measured in the same run as the bank's own figure: base decode 4.52e-2
# (worst of the four rows), with the bank 5.23e-2.
BF16_BANK_BOUND = 9.1e-2


def test_bf16_bank_logits_stay_within_twice_the_base_decodes_bf16_error():
    """the bank's rows against the oracle on their merged weights, the same rows of a decode without the bank against the oracle on the
    base weights; both figures are printed"""
    from whisper_ipa_amd import lora
    from whisper_ipa_amd.decoding import forced_decode_logits
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    dims = R.ModelDimensions(80, 1500, 768, 12, 1, 51865, 448, 768, 12, 1)
    W = R.synthetic_weights(dims, seed=41)
    torch.manual_seed(1)
    xa = torch.randn(4, 1500, 768) * 0.7
    sp, always, first, init = _sp()
    ids = (0, -1, 2, 1)
    tokens = np.concatenate([np.tile(np.asarray(init), (4, 1)), np.random.default_rng(6).integers(0, 50257, size=(4, 8))], axis=1)
    ads = {}
    for name, seed in zip(NAMES, (31, 32, 33)):
        cfg = lora.LoRAConfig(rank=8, alpha=16.0, targets=("attn.query", "attn.value", "cross_attn.query", "mlp1"), seed=seed)
        g = torch.Generator().manual_seed(seed)
        ads[name] = ({n: (t if n.endswith("lora_A") else 0.05 * torch.randn(t.shape, generator=g)) for n, t in lora.init_adapter(dims, cfg).items()}, cfg)
    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.bfloat16, cross_attention="absorbed")
    m.load_weights({k: v.clone() for k, v in W.items()})
    m.set_adapter_bank(lora.AdapterBank(m.dims, ads))
    feats = xa.to(torch.bfloat16)
    with_bank, _ = forced_decode_logits(m, feats.cuda(), tokens, len(init), always, first, sp.eot, row_ids=list(ids))
    base, _ = forced_decode_logits(m, feats.cuda(), tokens, len(init), always, first, sp.eot)
    with_bank, base = with_bank.cpu().numpy(), base.cpu().numpy()
    e_base, e_bank, moved = [], [], []
    with torch.no_grad():
        for b, i in enumerate(ids):
            tk, x1 = torch.from_numpy(tokens[b:b + 1, :-1]), feats[b:b + 1].float()
            ref0 = R.decoder_forward(W, dims, tk, x1)[0, len(init) - 1:].numpy()
            ref1 = ref0 if i < 0 else R.decoder_forward(lora.merged_weights(W, *ads[NAMES[i]]), dims, tk, x1)[0, len(init) - 1:].numpy()
            rms = float(np.sqrt(np.mean(ref1.astype(np.float64) ** 2)))
            e_base.append(float(np.abs(base[b] - ref0).max()) / float(np.sqrt(np.mean(ref0.astype(np.float64) ** 2))))
            e_bank.append(float(np.abs(with_bank[b] - ref1).max()) / rms)
            moved.append(float(np.abs(ref1 - ref0).max()) / rms)
    print(f"\nbf16 logits against the oracle, max|err| / rms: base decode {['%.2e' % e for e in e_base]}, with the bank {['%.2e' % e for e in e_bank]}; "
          f"the adapters move the oracle's logits by {['%.2e' % v for v in moved]}")
    bound = BF16_BANK_BOUND
    assert max(e_bank) <= bound, (e_bank, bound)
    assert min(v for v, i in zip(moved, ids) if i >= 0) > 5 * bound, "the adapters move the logits by less than the bound: the check is vacuous"
