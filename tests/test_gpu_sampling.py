"""GPU: temperature sampling in the decode step's tail (csrc/elementwise.hip: row_pick<.., SAMPLE> behind wipa_sample_step /
wipa_sample_step_embed / wipa_sample_noise; wipa_decode_call.sample; decode(temperature=, seed=);
transcribe(seed=)) against the float64 restatement of tests/sampling_ref.py.  Reference: upstream's GreedyDecoder.update with
temperature > 0 under mlx_whisper.transcribe's fallback schedule.  ``pytest -m gpu`` on an MI355X."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import sampling_ref as SR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
SP = R.SpecialTokens.multilingual()
TB, NT, EOT, N_INIT = 4000, 3995, 3990, 3  # the crafted vocabularies of the step tests
MARGIN = 1e-3  # f32 keys below 256 in magnitude have an ulp <= 1.5e-5: 30 x headroom


def _record(seed, attempt, temperature, streams, B):
    """the device sampling record (include/wipa.h) of B rows"""
    from whisper_ipa_amd import _lib

    L = _lib.lib()
    n = L.wipa_sample_record_bytes(B)
    host = np.zeros(n, dtype=np.uint8)
    flat = (C.c_uint32 * (2 * B))(*[int(v) for pair in streams for v in pair])
    _lib.check(L.wipa_sample_record_fill(host.ctypes.data, n, int(seed), int(attempt), float(temperature), flat, B), "record_fill")
    return torch.from_numpy(host).cuda()


# ---------------------------------------------------------------- 1. the noise
def test_sample_noise_matches_the_reference():
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    V, seed, attempt = 4099, (0x1234ABCD << 32) | 0x9E3779B9, 3
    streams = [(17, 5), (0xFFFFFFFF, 0x80000001)]
    with on_stream() as s:
        rec = _record(seed, attempt, 0.5, streams, 2)
        out = torch.full((V + 5,), 123.0, dtype=torch.float32, device="cuda")
        for row in range(2):
            for p in (2, 447):
                out.fill_(123.0)
                _lib.check(L.wipa_sample_noise(ptr(rec), row, p, V, ptr(out), sptr(s)), "wipa_sample_noise")
                got = out.cpu().numpy().astype(np.float64)
                want = SR.gumbel_noise(seed, [streams[row]], attempt, p, V)[0]
                err = np.abs(got[:V] - want).max()
                print(f"row {row} p {p}: max |g - g_ref| {err:.2e}, g in [{got[:V].min():.3f}, {got[:V].max():.3f}]")
                assert (got[V:] == 123.0).all()  # nothing past V
                # u is exact, logf is good to about an ulp and |g| < 17
                assert err <= 1e-5


# ---------------------------------------------------------------- 2. the draw on crafted rows
def _launch_step(logits, hist, m_first, m_always, rules, rec, slp0, V):
    """one wipa_sample_step launch: ``hist`` [B, N_INIT + len], every row at the same position"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    B = logits.shape[0]
    ldl, ld_tok = (V + 3) // 4 * 4 + 4, max(16, hist.shape[1] + 2)
    with on_stream() as s:
        lg = torch.zeros(B, ldl, dtype=torch.float32, device="cuda")
        lg[:, :V] = torch.from_numpy(logits).cuda()
        tk = torch.zeros(B, ld_tok, dtype=torch.int32, device="cuda")
        tk[:, : hist.shape[1]] = torch.from_numpy(hist.astype(np.int32)).cuda()
        pos = torch.tensor([hist.shape[1] - 1], dtype=torch.int32, device="cuda")
        slp = torch.from_numpy(slp0.astype(np.float32)).cuda()
        nd = torch.zeros(1, dtype=torch.int32, device="cuda")
        mf, ma = torch.from_numpy(m_first).cuda(), torch.from_numpy(m_always).cuda()
        _lib.check(L.wipa_sample_step(ptr(lg), ldl, B, V, ptr(mf), ptr(ma), ptr(tk), ld_tok, ptr(pos), N_INIT, EOT,
                                      C.byref(rules) if rules is not None else None, ptr(rec), ptr(slp), ptr(nd), sptr(s)), "wipa_sample_step")
        out = tk[:, hist.shape[1]].cpu().numpy().astype(np.int64), slp.cpu().numpy().astype(np.float64), int(nd.cpu()[0])
    return out


def _crafted(V, B, length):
    """rows built with the case builder of tests/timestamp_ref.py; histories of ONE length that fire each branch of the rules"""
    a, b, c, d, T = 1200, 2400, 3100, 3800, TB
    pool = {0: [[]],
            6: [[T + 0, a, T + 20, T + 20, b, c],      # text after text: timestamp mass against best text
                [T + 0, a, b, c, T + 60, T + 60],      # a closed pair: text only
                [T + 0, a, b, c, d, T + 60],           # a single timestamp: EOT or a timestamp from T + 60 on
                [T + 70, T + 70, a, T + 30, T + 30, b],  # non-monotone forced history: the cut follows the last in order
                [T + 0, a, T + 50, T + 50, EOT, EOT],  # latched
                [a, b, T + 7, T + 7, c, d]]}[length]
    boosts = [[], [["ts", 3.0]], [["ts", 6.0]], [[700, 9.0]], [[V - 1, 9.0]], [[EOT, 8.0]], [[T + 40, 9.0], [NT, 12.0]], [[15, 11.0]]]
    seqs = [pool[i % len(pool)] for i in range(B)]
    logits = np.stack([TR.case_logits(1000 * length + i, 2.0, boosts[(i // len(pool)) % len(boosts)], V, TB) for i in range(B)])
    return logits, seqs


@pytest.mark.parametrize("with_rules", [True, False])
@pytest.mark.parametrize("temperature", [0.2, 1.0])
@pytest.mark.parametrize("V,B", [(4099, 64), (51865, 8)])
def test_sample_step_matches_the_reference(V, B, temperature, with_rules):
    """V = 4099: V mod 4 = 3 exercises the trailing elements and V > 4096 gives some threads a second quad"""
    from whisper_ipa_amd import _lib

    seed, attempt = 77, 2
    always, first_only = [15, 16, 2000], [EOT, 220]
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, always + first_only)
    streams = [(100 + 3 * i, i % 2) for i in range(B)]
    rules = _lib.DecodeRules(TB, NT, 50) if with_rules else None
    rdict = dict(tb=TB, nt=NT, eot=EOT, max_init=50) if with_rules else None
    rec = _record(seed, attempt, temperature, streams, B)
    fired = {k: 0 for k in TR.BRANCHES}
    rows = left_out = 0
    for length in (0, 6):
        logits, seqs = _crafted(V, B, length)
        hist = np.array([[1, 2, 3] + list(s) for s in seqs], dtype=np.int64)
        is_first, p = length == 0, hist.shape[1] - 1
        slp0 = np.linspace(-3.0, -1.0, B).astype(np.float32).astype(np.float64)
        got_tok, got_slp, got_nd = _launch_step(logits, hist, m_first, m_always, rules, rec, slp0, V)
        noise = SR.gumbel_noise(seed, streams, attempt, p, V)
        want_nd = 0
        for r in range(B):
            st = SR.sample_row(logits[r], temperature, noise[r], m_first if is_first else m_always, rdict, seqs[r], is_first)
            got, added = int(got_tok[r]), got_slp[r] - slp0[r]
            if hist[r, -1] == EOT:  # latched: EOT again, nothing added
                assert got == EOT and added == 0.0
                continue
            want_nd += got != EOT
            assert 0 <= got < V and np.isfinite(st.row[got]), (r, got)  # a dead column is never drawn
            # sum_logprobs: the untempered log-softmax at the drawn column, against float64
            assert abs(added - (st.row[got] - st.lse)) < 1e-4, (r, added, st.row[got] - st.lse)
            rows += 1
            if st.key_margin > MARGIN:
                assert got == st.next, (r, length, got, st.next, st.key_margin)
                for k, f in st.fired.items():
                    fired[k] += int(f)
            else:
                left_out += 1
        assert got_nd == want_nd
    print(f"V={V} B={B} T={temperature} rules={with_rules}: {rows} rows, {left_out} under the key margin; branches {fired}")
    assert left_out <= 0.01 * rows
    if with_rules and B >= 48:
        assert all(n >= 1 for n in fired.values()), fired


# ---------------------------------------------------------------- 3. batch independence
def test_a_rows_draw_depends_on_its_stream_not_on_the_batch():
    V, T = 4099, 1.0
    rng = np.random.default_rng(5)
    row = (rng.standard_normal(V) * 0.5).astype(np.float32)  # flat: thousands of columns compete, any change of noise shows
    mask = TR.vocab_mask(V, [3])
    stream = (4242, 9)
    others = [(i, 0) for i in range(64)]
    others[37] = stream

    def draw(B, streams, seed=5, attempt=1, length=4):
        hist = np.tile(np.array([1, 2, 3] + [1200 + i for i in range(length)], dtype=np.int64), (B, 1))
        rec = _record(seed, attempt, T, streams, B)
        tok, _, _ = _launch_step(np.tile(row, (B, 1)), hist, mask, mask, None, rec, np.zeros(B), V)
        return tok

    base = []
    for length in (0, 1, 4, 9):  # four positions
        one = draw(1, [stream], length=length)
        many = draw(64, others, length=length)
        assert one[0] == many[37], (length, one[0], many[37])
        base.append(int(one[0]))
        ref = SR.sample_row(row, T, SR.gumbel_noise(5, [stream], 1, N_INIT - 1 + length, V)[0], mask)
        assert ref.key_margin <= MARGIN or one[0] == ref.next
    assert len(set(base)) > 1  # only p changed
    many = draw(64, others)
    assert len(set(many.tolist())) > 32  # distinct streams draw apart on the same row
    assert (draw(64, others, seed=6) != many).any()
    assert (draw(64, others, attempt=2) != many).any()
    assert (draw(64, others, length=5) != many).any()


# ---------------------------------------------------------------- 4. the distribution
def test_draws_follow_softmax_of_the_tempered_row():
    l, mask, streams = SR.distribution_case()
    rec = _record(SR.DIST_SEED, 0, SR.DIST_T, streams, SR.DIST_ROWS)
    hist = np.tile(np.array([1, 2, 3, 7], dtype=np.int64), (SR.DIST_ROWS, 1))  # p = 3, as the host test of the reference
    tok, _, _ = _launch_step(np.tile(l, (SR.DIST_ROWS, 1)), hist, mask, mask, None, rec, np.zeros(SR.DIST_ROWS), SR.DIST_V)
    assert not set(tok.tolist()) & set(SR.DIST_DEAD)
    stat, df, bound = SR.chi_square_vs_softmax(tok, l.astype(np.float64) + mask, SR.DIST_T)
    print(f"chi-square {stat:.1f} on {df} degrees of freedom (bound {bound:.1f})")
    assert stat < bound


# ---------------------------------------------------------------- 5. through the model
STEPS = 20


def _model(W, dtype=torch.float32):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


@pytest.fixture(scope="module")
def micro():
    """(weights, encoder features [2, 1500, 128] of a 30 s and a 5 s clip) of the random-init micro model"""
    W = R.synthetic_weights(MICRO, seed=7)
    clips = np.stack([R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0)])
    mels = torch.from_numpy(np.stack([R.log_mel_spectrogram(x) for x in clips]))
    with torch.no_grad():
        xa = R.encoder_forward(W, MICRO, mels)
    return W, xa


def _check_against_reference(m, feats, results, timed, seed, temperature, streams, attempt):
    """the sampled history through forced_decode_logits; the restatement on those per-step logits reproduces the tokens (under the
    margin rule) and avg_logprob"""
    from whisper_ipa_amd.decoding import DecodingOptions, _suppress_lists, forced_decode_logits, timestamp_rules
    from whisper_ipa_amd.tokenizer import get_tokenizer

    V = MICRO.n_vocab
    tok = get_tokenizer(True, language="en", task="transcribe")
    opts = DecodingOptions(language="en", without_timestamps=not timed)
    always, first = _suppress_lists(opts, tok)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    init = list(tok.sot_sequence) if timed else list(tok.sot_sequence_including_notimestamps)
    n_init, eot = len(init), tok.eot
    rules = timestamp_rules(tok) if timed else None
    rdict = dict(tb=tok.timestamp_begin, nt=tok.no_timestamps, eot=eot, max_init=50) if timed else None
    n = max(len(r.tokens) for r in results) + 1
    hist = np.array([init + list(r.tokens) + [eot] * (n - len(r.tokens)) for r in results], dtype=np.int64)
    trace, _ = forced_decode_logits(m, feats, hist, n_init, always, first, eot, rules=rules)
    trace = trace.cpu().numpy()
    checked = left_out = 0
    for b, res in enumerate(results):
        slp = 0.0
        for i in range(min(len(res.tokens) + 1, STEPS)):  # the sampled positions of this row, its EOT included where it got there
            p = n_init - 1 + i  # the position whose logits these are
            noise = SR.gumbel_noise(seed, [streams[b]], attempt, p, V)[0]
            st = SR.sample_row(trace[b, i], temperature, noise, m_first if i == 0 else m_always, rdict, hist[b, n_init:n_init + i].tolist(), i == 0)
            got = int(hist[b, n_init + i])
            assert np.isfinite(st.row[got])
            slp += st.row[got] - st.lse
            if st.key_margin > MARGIN:
                assert got == st.next, (b, i, got, st.next, st.key_margin)
                checked += 1
            else:
                left_out += 1
        assert abs(res.avg_logprob - slp / (len(res.tokens) + 1)) < 1e-4, (b, res.avg_logprob, slp / (len(res.tokens) + 1))
        assert res.temperature == temperature
    print(f"timed={timed} seed={seed} T={temperature}: {checked} steps reproduced, {left_out} under the key margin")
    assert checked >= 10 and left_out <= max(1, 0.01 * (checked + left_out))
    return hist


@pytest.mark.parametrize("timed", [True, False])
def test_decode_samples_what_the_reference_draws_from_its_own_logits(micro, timed):
    """graph replay and prefill, check_every stops: p and the streams are read live inside the replayed graph; a second call with
    another seed and temperature on the same state matches ITS reference (it would repeat the first if either were baked in)"""
    import whisper_ipa_amd as wipa

    W, xa = micro
    m = _model(W)
    feats = xa.cuda()
    kw = dict(language="en", without_timestamps=not timed, fp16=False, sample_len=STEPS)
    streams = [(40, 1), (7, 0)]
    first = wipa.decode(m, feats, wipa.DecodingOptions(temperature=0.6, seed=7, sample_streams=streams, **kw))
    h1 = _check_against_reference(m, feats, first, timed, 7, 0.6, streams, 0)
    second = wipa.decode(m, feats, wipa.DecodingOptions(temperature=0.9, seed=8, sample_streams=streams, sample_attempt=2, **kw))
    h2 = _check_against_reference(m, feats, second, timed, 8, 0.9, streams, 2)
    assert h1.shape != h2.shape or (h1 != h2).any()
    # the same call again: reproducible; the default streams are (row, 0)
    again = wipa.decode(m, feats, wipa.DecodingOptions(temperature=0.6, seed=7, sample_streams=streams, **kw))
    assert [r.tokens for r in again] == [r.tokens for r in first] and [r.avg_logprob for r in again] == [r.avg_logprob for r in first]
    dflt = wipa.decode(m, feats, wipa.DecodingOptions(temperature=0.6, seed=7, **kw))
    _check_against_reference(m, feats, dflt, timed, 7, 0.6, [(0, 0), (1, 0)], 0)
    # a row alone, on its stream, draws what it drew in the batch
    alone = wipa.decode(m, feats[1:2], wipa.DecodingOptions(temperature=0.6, seed=7, sample_streams=streams[1:], **kw))
    _check_against_reference(m, feats[1:2], alone, timed, 7, 0.6, streams[1:], 0)
    # temperature 0 with a seed is the greedy path, bit for bit
    g0 = wipa.decode(m, feats, wipa.DecodingOptions(**kw))
    g1 = wipa.decode(m, feats, wipa.DecodingOptions(temperature=0.0, seed=7, sample_streams=streams, **kw))
    assert [r.tokens for r in g0] == [r.tokens for r in g1] and [r.avg_logprob for r in g0] == [r.avg_logprob for r in g1]


@pytest.mark.parametrize("use_graph,prefill,check_every", [(True, True, 3), (False, True, 8), (True, False, 5), (False, False, 20)])
def test_sampling_decode_is_the_same_eager_replayed_prefilled_or_walked(micro, monkeypatch, use_graph, prefill, check_every):
    from whisper_ipa_amd.decoding import Sampling, greedy_decode_tokens, timestamp_rules
    from whisper_ipa_amd.tokenizer import get_tokenizer

    W, xa = micro
    m = _model(W)
    tok = get_tokenizer(True, language="en", task="transcribe")
    always, first = R.suppress_lists(SP)
    sample = Sampling(21, 0.8, [(3, 3), (4, 4)], 1)
    init = list(tok.sot_sequence)
    want = greedy_decode_tokens(m, xa.cuda(), init, always, first, tok.eot, max_new_tokens=STEPS, stop_on_eot=False, rules=timestamp_rules(tok),
                                sample=sample)
    if not prefill:
        monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    got = greedy_decode_tokens(m, xa.cuda(), init, always, first, tok.eot, max_new_tokens=STEPS, stop_on_eot=True, use_graph=use_graph,
                               check_every=check_every, rules=timestamp_rules(tok), sample=sample)
    n = got.tokens.shape[1]
    assert (got.tokens == want.tokens[:, :n]).all(), (got.tokens.tolist(), want.tokens.tolist())
    assert (want.tokens[:, n:] == tok.eot).all()


def test_sampling_is_refused_where_the_step_has_no_fused_tail(micro, monkeypatch):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import Sampling, greedy_decode_tokens

    W, xa = micro
    m = _model(W)
    always, first = R.suppress_lists(SP)
    monkeypatch.setenv("WIPA_DECODE_TAIL", "0")
    with pytest.raises(_lib.WipaError, match="WIPA_DECODE_TAIL"):
        greedy_decode_tokens(m, xa.cuda(), list(SP.sot_sequence_including_notimestamps(0)), always, first, SP.eot, max_new_tokens=4,
                             stop_on_eot=False, sample=Sampling(1, 0.5))


def test_transcribe_batches_stays_greedy_only(micro):
    import whisper_ipa_amd as wipa

    W, xa = micro
    with pytest.raises(NotImplementedError, match="temperature"):
        list(wipa.transcribe_batches(_model(W), [xa], wipa.DecodingOptions(language="en", temperature=0.4, seed=1)))


# ---------------------------------------------------------------- 6. transcribe() with the fallback
def test_transcribe_retries_failing_windows_from_their_features(micro):
    """the random-init model's average log-probability is below upstream's threshold, so its windows go through the schedule: the
    first windows' segments are the splitter's cut of what decode() samples for those features, streams (seek, file index) and
    attempt; seed=None gives today's output"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.transcribe import _needs_fallback, split_segments

    W, _ = micro
    m = _model(W)
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]
    temps = (0.0, 0.3, 0.7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = wipa.transcribe(m, [long, short], language="en", sample_len=STEPS, fp16=False, seed=3, temperature=temps)
    # the same loop by hand on the first windows
    win = np.zeros((2, 480000), dtype=np.float32)
    win[0], win[1, : len(short)] = long[:480000], short
    mel = wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80)
    kw = dict(language="en", without_timestamps=False, sample_len=STEPS, fp16=False)
    res = wipa.decode(m, mel, wipa.DecodingOptions(**kw))
    greedy = list(res)
    failing = [i for i in range(2) if _needs_fallback(res[i], 2.4, -1.0, 0.6)]
    assert failing, [r.avg_logprob for r in res]  # at least one window is retried
    retried = set(failing)
    for k in range(1, len(temps)):
        if not failing:
            break
        feats = torch.stack([res[i].audio_features for i in failing])
        sub = wipa.decode(m, feats, wipa.DecodingOptions(temperature=temps[k], seed=3, sample_streams=[(0, i) for i in failing], sample_attempt=k, **kw))
        for i, r in zip(failing, sub):
            res[i] = r
        failing = [i for i in failing if _needs_fallback(res[i], 2.4, -1.0, 0.6)]
    for i, clip in enumerate((long, short)):
        segs, _ = split_segments(res[i].tokens, SP.timestamp_begin, 0.0, min(3000, len(clip) // 160))
        first = [s for s in out[i]["segments"] if s["seek"] == 0]
        assert [(s["start"], s["end"]) for s in first] == [(x["start"], x["end"]) for x in segs]
        for s, x in zip(first, segs):
            assert s["tokens"] in (x["tokens"], []) and s["temperature"] == res[i].temperature
            assert abs(s["avg_logprob"] - res[i].avg_logprob) < 1e-5
            assert ("needs_fallback" in s) == (i not in retried and _needs_fallback(res[i], 2.4, -1.0, 0.6))
    print("first windows ended at temperatures", [res[i].temperature for i in range(2)], "after retrying", sorted(retried))
    assert any(s["temperature"] > 0.0 for o in out for s in o["segments"])
    # every failing window of the call went through the schedule: no flag, no warning
    assert not [x for x in w if "needs_fallback" in str(x.message)] and not any("needs_fallback" in s for o in out for s in o["segments"])
    # seed=None: the flag and the warning, temperature 0, the greedy tokens
    with warnings.catch_warnings(record=True) as w0:
        warnings.simplefilter("always")
        plain = wipa.transcribe(m, [long, short], language="en", sample_len=STEPS, fp16=False)
    assert len([x for x in w0 if "needs_fallback" in str(x.message)]) == 1
    for i, clip in enumerate((long, short)):
        segs, _ = split_segments(greedy[i].tokens, SP.timestamp_begin, 0.0, min(3000, len(clip) // 160))
        first = [s for s in plain[i]["segments"] if s["seek"] == 0]
        assert [s["tokens"] for s in first] == [x["tokens"] if s["text"] else [] for s, x in zip(first, segs)]
        assert all(s["temperature"] == 0.0 and s.get("needs_fallback", False) == (i in retried) for s in first)
