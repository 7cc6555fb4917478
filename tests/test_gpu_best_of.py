"""GPU: best-of-N sampling -- candidate groups that share one encoder output in the decode state (wipa_model_cfg.dec_n_group; the
grouped instantiations of the cached, fused and absorbed cross-attention kernels), wipa_rank_groups, decode(best_of=) and
transcribe(best_of=) against the restatement of tests/best_of_ref.py and against the ungrouped decode of replicated features.
Reference: upstream's DecodingTask with n_group = best_of and MaximumLikelihoodRanker.  ``pytest -m gpu`` on an MI355X."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import best_of_ref as BR
import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP = PR.MICRO, PR.W384, PR.SP
EOT = SP.eot
NEW = 16   # new tokens of the model tests
SEED = 7   # of the prompt-pass test (its docstring says what it leaves out)


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def mels():
    return PR.clip_mels()  # a 30 s and a 5 s clip, as tests/test_gpu_sampling.py builds them


@pytest.fixture(scope="module")
def models(mels):
    """(model, features [2, 1500, d] f32 on the device) per case, built once: MICRO f32 cached, W384 bf16 cached / absorbed"""
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    cache = {}

    def get(name):
        if name not in cache:
            dims, dtype, cross, seed = {"micro": (MICRO, torch.float32, "cached", 7), "w384_cached": (W384, torch.bfloat16, "cached", 1),
                                        "w384_absorbed": (W384, torch.bfloat16, "absorbed", 1)}[name]
            wkey = ("W", dims.n_text_state)
            if wkey not in cache:
                W = R.synthetic_weights(dims, seed=seed)
                with torch.no_grad():
                    cache[wkey] = (W, R.encoder_forward(W, dims, mels))
            W, xa = cache[wkey]
            m = Whisper(ModelDimensions(**dims.__dict__), dtype=dtype, cross_attention=cross)
            m.load_weights(W)
            cache[name] = (m, xa.cuda())
        return cache[name]

    return get


def _tok():
    from whisper_ipa_amd.tokenizer import get_tokenizer

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return get_tokenizer(True, language="en", task="transcribe")


def _decode_args(timed):
    from whisper_ipa_amd.decoding import timestamp_rules

    tok = _tok()
    always, first = R.suppress_lists(SP)
    init = list(tok.sot_sequence) if timed else list(tok.sot_sequence_including_notimestamps)
    return init, always, first, (timestamp_rules(tok) if timed else None)


# ---------------------------------------------------------------- 1. the ranker
def _crafted_group_rows(rng, clips, G, n, scenario, eot, ld_tok, begin):
    """rows whose EOT sits in the first generated column, in the last one, in the middle, or nowhere, by candidate; sums by scenario"""
    B = clips * G
    toks = rng.integers(0, 1000, size=(B, ld_tok)).astype(np.int32)
    sums = -(rng.random(B).astype(np.float32) * 20 + 0.5)
    for b in range(B):
        kind = (b + b // G) % 4
        if kind == 0:
            toks[b, begin] = eot
        elif kind == 1:
            toks[b, begin + n - 1] = eot
        elif kind == 2:
            toks[b, begin + n // 2] = eot
            toks[b, begin + n - 1] = eot  # a second EOT after the first changes nothing
    if scenario == "equal_sums":
        sums[:] = np.float32(-3.25)
    elif scenario == "tie" and G >= 2:
        for c in range(clips):  # the last two candidates of every clip: same length, same sum, the best score of the clip
            i, j = c * G + G - 2, c * G + G - 1
            toks[i, begin:begin + n] = 5
            toks[j, begin:begin + n] = 6
            sums[i] = sums[j] = np.float32(-0.001)
    return toks, sums


@pytest.mark.parametrize("n", [1, 63, 64, 65, 224])
def test_rank_groups_matches_the_restatement_exactly(n):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import length_penalty_table
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    ld_tok, begin, eot = 456, 3, EOT
    rng = np.random.default_rng(100 + n)
    ties = 0
    for G in (1, 2, 5, 7):
        for clips in (1, 3):
            for lp in (None, 0.6):
                for scenario in ("random", "equal_sums", "tie"):
                    toks, sums = _crafted_group_rows(rng, clips, G, n, scenario, eot, ld_tok, begin)
                    B = clips * G
                    want_w, want_len, scores = BR.rank(toks, sums, G, begin, n, eot, lp)
                    ties += sum(1 for sc in scores if sorted(sc)[-1] == sorted(sc)[-2]) if G > 1 else 0
                    with on_stream() as s:
                        d_tok, d_sum = torch.from_numpy(toks).cuda(), torch.from_numpy(sums).cuda()
                        pen = torch.from_numpy(length_penalty_table(n, lp)).cuda()
                        winner = torch.full((clips,), -1, dtype=torch.int32, device="cuda")
                        length = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                        ld_out = begin + n + 5
                        best = torch.full((clips, ld_out), -7, dtype=torch.int32, device="cuda")
                        best_sum = torch.zeros(clips, dtype=torch.float32, device="cuda")
                        _lib.check(L.wipa_rank_groups(ptr(d_tok), ld_tok, B, G, begin, n, eot, ptr(d_sum), ptr(pen), ptr(winner), ptr(length),
                                                      ptr(best), ld_out, ptr(best_sum), sptr(s)), "wipa_rank_groups")
                        got_w, got_len = winner.cpu().numpy(), length.cpu().numpy().reshape(clips, G)
                        got_best, got_sum = best.cpu().numpy(), best_sum.cpu().numpy()
                    case = (G, clips, n, lp, scenario)
                    assert got_w.tolist() == want_w.tolist(), (case, got_w, want_w, scores)
                    assert (got_len == want_len).all(), (case, got_len, want_len)
                    for c in range(clips):
                        b = c * G + int(want_w[c])
                        assert (got_best[c, :begin + n] == toks[b, :begin + n]).all(), case
                        assert (got_best[c, begin + n:] == -7).all(), case  # nothing past the generated columns
                        assert got_sum[c] == sums[b], case
    assert ties >= 8  # the tie scenarios did tie
    # rows that do not divide into groups are refused
    with on_stream() as s:
        z = torch.zeros(8, 64, dtype=torch.int32, device="cuda")
        f = torch.zeros(8, dtype=torch.float32, device="cuda")
        p = torch.ones(9, dtype=torch.float64, device="cuda")
        assert L.wipa_rank_groups(ptr(z), 64, 7, 2, 3, 8, eot, ptr(f), ptr(p), ptr(z), ptr(z), ptr(z), 64, ptr(f), sptr(s)) != 0


# ---------------------------------------------------------------- 1b. the grouped cached cross-attention launch
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grouped_cross_attention_equals_the_launch_on_replicated_kv(dtype):
    """wipa_decode_cross_attn_grouped (row b reads the K / V of clip b / G) against wipa_decode_cross_attn[_multi] on replicated K / V,
    bit for bit: 1..4 query rows per decode row, and for one query row both sides of the 512-key threshold between the short-cache
    and the streaming form of the kernel (odd key counts: the clamped tail groups)"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    H, clips, G = 3, 3, 5
    B = clips * G
    dt = 0 if dtype == torch.float32 else 1
    gen = torch.Generator().manual_seed(3)
    for Tk in (37, 512, 513, 1500):
        for n_q in (1, 2, 3, 4):
            kv = torch.randn(clips, 2 * H, Tk, 64, generator=gen).to(device="cuda", dtype=dtype)
            q = torch.randn(B * n_q, H * 64, generator=gen).to(device="cuda", dtype=dtype)
            kv_rep = kv.repeat_interleave(G, dim=0).contiguous()
            with on_stream() as s:
                got = torch.full_like(q, 7.0)
                want = torch.full_like(q, -7.0)
                _lib.check(L.wipa_decode_cross_attn_grouped(ptr(q), ptr(kv), ptr(got), B, H, Tk, n_q, G, dt, sptr(s)), "grouped")
                _lib.check(L.wipa_decode_cross_attn_multi(ptr(q), ptr(kv_rep), ptr(want), B, H, Tk, n_q, dt, sptr(s)), "replicated")
                one = torch.full_like(q, 3.0)
                _lib.check(L.wipa_decode_cross_attn_grouped(ptr(q), ptr(kv_rep), ptr(one), B, H, Tk, n_q, 1, dt, sptr(s)), "n_group 1")
                s.synchronize()
            assert torch.equal(got, want), (dtype, Tk, n_q, float((got.float() - want.float()).abs().max()))
            assert torch.equal(one, want)
            # clip 0 and clip 1 differ: the rows did read their own clip
            assert not torch.equal(got[: G * n_q], got[G * n_q: 2 * G * n_q])
    with on_stream() as s:
        assert L.wipa_decode_cross_attn_grouped(ptr(q), ptr(kv), ptr(got), B - 1, H, Tk, 1, G, dt, sptr(s)) != 0


# ---------------------------------------------------------------- 2. grouped equals replicated, stepping the prompt
G3 = 3
STREAMS = [(40, 1), (7, 0)]
_replicated = {}


def _both(models, name, timed, use_graph, splits=0, seed=21, temperature=0.8, key=None):
    """(grouped decode of 2 clips x 3 candidates, the ungrouped decode of the 6 replicated rows on the same six streams)"""
    from whisper_ipa_amd.decoding import Sampling, greedy_decode_tokens

    m, feats = models(name)
    if splits:
        m.cross_splits = splits
    init, always, first, rules = _decode_args(timed)
    kw = dict(max_new_tokens=NEW, stop_on_eot=False, rules=rules)
    rkey = (name, timed, splits, seed, key)
    if rkey not in _replicated:  # the reference: computed once per case, shared by the graph and the eager run
        rep = greedy_decode_tokens(m, feats.repeat_interleave(G3, dim=0), init, always, first, EOT,
                                   sample=Sampling(seed, temperature, BR.candidate_streams(STREAMS, G3), 1), **kw)
        _replicated[rkey] = (rep.tokens.copy(), rep.sum_logprobs.copy())
    got = greedy_decode_tokens(m, feats, init, always, first, EOT, sample=Sampling(seed, temperature, STREAMS, 1), n_group=G3,
                               use_graph=use_graph, **kw)
    return got, _replicated[rkey]


def _assert_same(got, want, what):
    toks, sums = want
    assert got.tokens.shape == toks.shape == (2 * G3, toks.shape[1]), (got.tokens.shape, toks.shape)
    assert (got.tokens == toks).all(), (what, got.tokens.tolist(), toks.tolist())
    assert (got.sum_logprobs == sums).all(), (what, got.sum_logprobs.tolist(), sums.tolist())
    # the candidates did draw apart: the streams differ in the high word only
    assert len({tuple(r) for r in got.tokens.tolist()}) >= 4, got.tokens.tolist()


@pytest.mark.parametrize("timed", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name,splits", [("micro", 0), ("w384_cached", 0), ("w384_absorbed", 2), ("w384_absorbed", 4)])
def test_grouped_decode_equals_the_replicated_decode_bit_for_bit(models, monkeypatch, name, splits, use_graph, timed):
    """a grouped row does the arithmetic of an ungrouped row on the same bytes, and a row never depends on its neighbours: any
    difference in tokens or log-prob sums is a bug, not rounding"""
    monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    got, want = _both(models, name, timed, use_graph, splits)
    _assert_same(got, want, (name, splits, use_graph, timed))


@pytest.mark.parametrize("name,env", [("micro", {"WIPA_DECODE_FUSED": "0"}), ("w384_cached", {"WIPA_DECODE_FUSED": "0"}),
                                      ("w384_cached", {"WIPA_CROSS_PRE": "0"}), ("w384_absorbed", {"WIPA_ABS_FUSED_PROLOGUE": "0"})])
def test_grouped_decode_equals_replicated_in_the_other_step_forms(models, monkeypatch, name, env):
    """the unfused cached step (wipa_decode_cross_attn_grouped), the plain fused cross block and the absorbed block in separate launches"""
    monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, want = _both(models, name, True, True, key=tuple(env.items()))
    _assert_same(got, want, (name, env))


# ---------------------------------------------------------------- 3. with the prompt pass (the default)
@pytest.mark.parametrize("name", ["micro", "w384_cached", "w384_absorbed"])
def test_grouped_decode_with_the_prompt_pass(models, name):
    """The prompt pass runs over ALL rows with the cross K / V indexed per clip (wipa_decode_cross_attn_grouped with the prompt's
    rows; the absorbed form per prompt position), so the grouped run equals the replicated run bit for bit here too.  On MICRO f32
    every candidate's history is also redrawn from the logits of its own history (forced_decode_logits on replicated features).
    Seed 7, temperature 0.8, attempt 1: the ungrouped decode of the six replicated rows -- the same bits, by the first assertion --
    leaves out 1 of its 96 sampled positions under the key margin and reproduces 95 (measured on an MI355X; the cap is max(1, 1 %);
    the test prints the count)."""
    from whisper_ipa_amd.decoding import DecodingOptions, _suppress_lists, forced_decode_logits

    got, want = _both(models, name, True, True, seed=SEED, key="prefill")
    _assert_same(got, want, name)
    if name != "micro":
        return
    m, feats = models(name)
    tok = _tok()
    always, first = _suppress_lists(DecodingOptions(language="en", without_timestamps=False), tok)
    V = MICRO.n_vocab
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    init, _, _, rules = _decode_args(True)
    n_init = len(init)
    rdict = dict(tb=tok.timestamp_begin, nt=tok.no_timestamps, eot=EOT, max_init=50)
    hist = np.concatenate([got.tokens, np.full((got.tokens.shape[0], 1), EOT, dtype=np.int64)], axis=1)
    trace, _ = forced_decode_logits(m, feats.repeat_interleave(G3, dim=0), hist, n_init, always, first, EOT, rules=rules)
    trace = trace.cpu().numpy()
    streams = BR.candidate_streams(STREAMS, G3)
    checked = left_out = 0
    for b in range(hist.shape[0]):
        c, l, slp = BR.check_history(trace[b], hist[b], n_init, EOT, SEED, 0.8, streams[b], 1, m_first, m_always, rdict, NEW)
        checked, left_out = checked + c, left_out + l
        assert abs(float(got.sum_logprobs[b]) - slp) < 1e-3, (b, got.sum_logprobs[b], slp)
    print(f"{checked} positions reproduced, {left_out} under the key margin")
    assert checked >= 10 and left_out <= max(1, 0.01 * (checked + left_out))


# ---------------------------------------------------------------- 4. decode(best_of=3) end to end
def _result_rank(singles, length_penalty=None):
    """the restatement's choice among per-candidate DecodingResults of one clip"""
    n = max(len(r.tokens) for r in singles) + 1
    toks = np.array([list(r.tokens) + [EOT] * (n - len(r.tokens)) for r in singles], dtype=np.int64)
    sums = np.array([np.float32(r.avg_logprob * (len(r.tokens) + 1)) for r in singles], dtype=np.float32)
    w, _, scores = BR.rank(toks, sums, len(singles), 0, n, EOT, length_penalty)
    return int(w[0]), scores[0]


@pytest.mark.parametrize("name,timed", [("micro", True), ("micro", False), ("w384_absorbed", True)])
def test_decode_best_of_returns_the_best_candidate_of_every_clip(models, name, timed):
    import whisper_ipa_amd as wipa

    m, feats = models(name)
    kw = dict(language="en", without_timestamps=not timed, fp16=False, sample_len=NEW, temperature=0.7, seed=5, sample_attempt=2)
    res = wipa.decode(m, feats, wipa.DecodingOptions(best_of=3, sample_streams=STREAMS, **kw))
    assert len(res) == 2
    singles = [wipa.decode(m, feats, wipa.DecodingOptions(sample_streams=[BR.candidate_stream(s, k) for s in STREAMS], **kw)) for k in range(3)]
    for c in range(2):
        cands = [singles[k][c] for k in range(3)]
        w, scores = _result_rank(cands)
        print(f"{name} clip {c}: winner {w}, scores {scores}")
        assert res[c].tokens == cands[w].tokens, (c, w, res[c].tokens, [x.tokens for x in cands])
        assert res[c].avg_logprob == cands[w].avg_logprob and res[c].text == cands[w].text
        assert res[c].compression_ratio == cands[w].compression_ratio or (np.isnan(res[c].compression_ratio) and np.isnan(cands[w].compression_ratio))
        assert res[c].temperature == 0.7
        assert scores[w] >= scores[0]  # candidate 0 is today's single draw: best_of never scores below it
    # a window decoded alone picks the same winner with the same tokens
    alone = wipa.decode(m, feats[1:2], wipa.DecodingOptions(best_of=3, sample_streams=STREAMS[1:], **kw))
    assert alone[0].tokens == res[1].tokens and alone[0].avg_logprob == res[1].avg_logprob
    # best_of = 1 is the plain sampling decode
    one = wipa.decode(m, feats, wipa.DecodingOptions(best_of=1, sample_streams=STREAMS, **kw))
    assert [r.tokens for r in one] == [r.tokens for r in singles[0]] and [r.avg_logprob for r in one] == [r.avg_logprob for r in singles[0]]
    # the length penalty changes the ranking rule, not the candidates
    lp = wipa.decode(m, feats, wipa.DecodingOptions(best_of=3, length_penalty=1.0, sample_streams=STREAMS, **kw))
    for c in range(2):
        w, _ = _result_rank([singles[k][c] for k in range(3)], 1.0)
        assert lp[c].tokens == singles[w][c].tokens


# ---------------------------------------------------------------- 5. ragged prompts
@pytest.mark.parametrize("name", ["micro", "w384_absorbed"])
def test_best_of_with_per_row_prompts(models, monkeypatch, name):
    """decode(prompts=[None, 17 ids], best_of=2) against the per-candidate ungrouped ragged decodes, bitwise with the prompt stepped.
    With the batched prompt pass (the default; P = 32, so MICRO f32 takes the f32 MFMA kernel of wipa_attention_as with the 2 x 32 query
    rows of a clip in one batch entry, W384 bf16 the VALU kernel and the per-clip K / V projection workspace) the grouped decode of
    2 clips x 2 candidates equals the ungrouped ragged decode of the 4 replicated rows on the same four streams bit for bit, in
    tokens and log-prob sums; the ranked form returns the restatement's choice among those candidates"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.decoding import Sampling, initial_tokens, ragged_decode_tokens

    m, feats = models(name)
    prompts = [None, PR.histories()[2]]
    assert len(prompts[1]) == 17
    kw = dict(language="en", without_timestamps=True, fp16=False, sample_len=NEW, temperature=0.7, seed=9, prompts=prompts)
    monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    res = wipa.decode(m, feats, wipa.DecodingOptions(best_of=2, sample_streams=STREAMS, **kw))
    singles = [wipa.decode(m, feats, wipa.DecodingOptions(sample_streams=[BR.candidate_stream(s, k) for s in STREAMS], **kw)) for k in range(2)]
    for c in range(2):
        cands = [singles[k][c] for k in range(2)]
        w, _ = _result_rank(cands)
        assert res[c].tokens == cands[w].tokens and res[c].avg_logprob == cands[w].avg_logprob, (c, w)
    monkeypatch.delenv("WIPA_NO_PREFILL")
    # the batched prompt pass: grouped rows against the UNGROUPED ragged decode of replicated features, then the ranked form
    tok = _tok()
    init, always, first, _ = _decode_args(False)
    own = [initial_tokens(tok, init, p, None, 448, NEW) for p in prompts]
    sample = Sampling(9, 0.7, STREAMS, 0)
    allrows = ragged_decode_tokens(m, feats, own, always, first, EOT, max_new_tokens=NEW, sample=sample, n_group=2, stop_on_eot=False)
    ranked = ragged_decode_tokens(m, feats, own, always, first, EOT, max_new_tokens=NEW, sample=sample, n_group=2, rank=True, stop_on_eot=False)
    rep = ragged_decode_tokens(m, feats.repeat_interleave(2, dim=0), [own[0], own[0], own[1], own[1]], always, first, EOT, max_new_tokens=NEW,
                               sample=Sampling(9, 0.7, BR.candidate_streams(STREAMS, 2), 0), stop_on_eot=False)
    P = allrows.n_init
    assert P == rep.n_init == 32 and allrows.tokens.shape == rep.tokens.shape
    assert (allrows.tokens == rep.tokens).all(), (name, allrows.tokens[:, P:].tolist(), rep.tokens[:, P:].tolist())
    assert (allrows.sum_logprobs == rep.sum_logprobs).all(), (name, allrows.sum_logprobs.tolist(), rep.sum_logprobs.tolist())
    assert len({tuple(r[P:]) for r in allrows.tokens.tolist()}) == 4  # four different draws: clips and candidates are told apart
    assert allrows.tokens.shape[0] == 4 and ranked.tokens.shape[0] == 2 and ranked.n_init == P
    w, lens, _ = BR.rank(allrows.tokens, allrows.sum_logprobs, 2, P, NEW, EOT)
    assert ranked.winner.tolist() == w.tolist() and (ranked.lengths == lens).all()
    for c in range(2):
        assert (ranked.tokens[c] == allrows.tokens[2 * c + int(w[c])]).all() and ranked.sum_logprobs[c] == allrows.sum_logprobs[2 * c + int(w[c])]
    assert (allrows.tokens[0, :P] == allrows.tokens[1, :P]).all() and (allrows.tokens[2, :P] == allrows.tokens[3, :P]).all()
    res2 = wipa.decode(m, feats, wipa.DecodingOptions(best_of=2, sample_streams=STREAMS, **kw))
    for c in range(2):
        row = ranked.tokens[c, P:].tolist()
        assert res2[c].tokens == (row[: row.index(EOT)] if EOT in row else row)


# ---------------------------------------------------------------- 6. the layout
def test_the_layout_holds_the_audio_once_per_clip(models):
    from whisper_ipa_amd import _lib

    L = _lib.lib()
    for name in ("micro", "w384_cached", "w384_absorbed"):
        m, _ = models(name)
        base = m.packed(absorbed=name == "w384_absorbed")["cfg"]

        def layout(G, B, expect_ok=True):
            cfg = _lib.ModelCfg.from_buffer_copy(base)
            cfg.dec_n_group = G
            lay = _lib.DecLayout()
            rc = L.wipa_decoder_layout(C.byref(cfg), B, C.byref(lay))
            assert (rc == 0) == expect_ok, (name, G, B, L.wipa_last_error())
            return lay

        def extents(lay):
            """the byte extent of every region, in the layout's order"""
            offs = [("tokens", lay.tokens), ("pos", lay.pos), ("not_done", lay.not_done), ("sum_logprobs", lay.sum_logprobs), ("logits", lay.logits),
                    ("cross_kv", lay.cross_kv), ("self_kv", lay.self_kv), ("scratch", lay.scratch), ("end", lay.total_bytes)]
            assert [o for _, o in offs] == sorted(o for _, o in offs)
            return {a: offs[i + 1][1] - o for i, (a, o) in enumerate(offs[:-1])}

        g, u10, u2 = extents(layout(5, 10)), extents(layout(0, 10)), extents(layout(0, 2))
        assert g["cross_kv"] == u2["cross_kv"] < u10["cross_kv"]
        assert {k: v for k, v in g.items() if k != "cross_kv"} == {k: v for k, v in u10.items() if k != "cross_kv"}
        layout(5, 9, expect_ok=False)
        assert b"dec_n_group" in L.wipa_last_error()
        one = layout(1, 10)
        assert all(getattr(one, f) == getattr(layout(0, 10), f) for f, _ in one._fields_)


# ---------------------------------------------------------------- 7. transcribe(best_of=)
def test_transcribe_passes_best_of_to_the_retries(models):
    """the micro model's windows fail the log-probability threshold (the setting of test_transcribe_retries_failing_windows_from_
    their_features): the first windows' segments are the splitter's cut of what decode(best_of=2) returns for those features, streams
    (seek, file index) and attempt; without best_of the output is today's"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.transcribe import _needs_fallback, split_segments

    m, _ = models("micro")
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]
    temps = (0.0, 0.3, 0.7)
    common = dict(language="en", sample_len=NEW, fp16=False, seed=3, temperature=temps)
    out = wipa.transcribe(m, [long, short], best_of=2, **common)
    win = np.zeros((2, 480000), dtype=np.float32)
    win[0], win[1, : len(short)] = long[:480000], short
    mel = wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80)
    kw = dict(language="en", without_timestamps=False, sample_len=NEW, fp16=False)

    def by_hand(best_of):
        res = list(wipa.decode(m, mel, wipa.DecodingOptions(**kw)))  # temperature 0: no best_of
        failing = [i for i in range(2) if _needs_fallback(res[i], 2.4, -1.0, 0.6)]
        assert failing
        for k in range(1, len(temps)):
            if not failing:
                break
            feats = torch.stack([res[i].audio_features for i in failing])
            sub = wipa.decode(m, feats, wipa.DecodingOptions(temperature=temps[k], seed=3, sample_streams=[(0, i) for i in failing], sample_attempt=k,
                                                             best_of=best_of, **kw))
            for i, r in zip(failing, sub):
                res[i] = r
            failing = [i for i in failing if _needs_fallback(res[i], 2.4, -1.0, 0.6)]
        return res

    def first_windows_match(out, res):
        for i, clip in enumerate((long, short)):
            segs, _ = split_segments(res[i].tokens, SP.timestamp_begin, 0.0, min(3000, len(clip) // 160))
            first = [s for s in out[i]["segments"] if s["seek"] == 0]
            assert [(s["start"], s["end"]) for s in first] == [(x["start"], x["end"]) for x in segs]
            for s, x in zip(first, segs):
                # transcribe() empties a segment of zero length or blank text and keeps every other segment's tokens
                blank = x["start"] == x["end"] or tok.decode([t for t in x["tokens"] if t < tok.eot]).strip() == ""
                assert s["tokens"] == ([] if blank else x["tokens"]), (i, s["tokens"], x["tokens"])
                assert s["temperature"] == res[i].temperature and s["avg_logprob"] == res[i].avg_logprob
                kept[0] += not blank

    tok, kept = _tok(), [0]
    res2 = by_hand(2)
    first_windows_match(out, res2)
    assert kept[0] >= 1  # the comparison did see tokens
    plain = wipa.transcribe(m, [long, short], **common)
    res1 = by_hand(None)
    first_windows_match(plain, res1)
    assert any(s["temperature"] > 0.0 for o in out for s in o["segments"])
    print("avg_logprob with best_of=2:", [r.avg_logprob for r in res2], "without:", [r.avg_logprob for r in res1])
