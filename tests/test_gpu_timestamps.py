"""GPU: the timestamp rules in the decode step's tail (csrc/elementwise.hip: rules_row_pick behind wipa_timestamp_step /
wipa_timestamp_step_embed; wipa_decoder_run_ex / wipa_decoder_prefill_ex with wipa_decode_call.rules) against the numpy restatement of tests/timestamp_ref.py.
Reference: ApplyTimestampRules as mlx_whisper.transcribe applies it (the reference's scripts/evaluate_model.py:112-119).
``pytest -m gpu`` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
W384 = R.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)  # where the bf16 step would take the partials tail
SP = R.SpecialTokens.multilingual()
V, TB, NT, EOT = 51865, SP.timestamp_begin, SP.no_timestamps, SP.eot
INIT = [SP.sot, SP.lang_first, SP.transcribe]  # tok.sot_sequence: no <|notimestamps|>
STEPS = 20


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def _rules(max_init=50):
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(TB, NT, max_init)


def _weights(dims, seed, scripted):
    W = R.synthetic_weights(dims, seed=seed)
    if scripted:
        W["decoder.positional_embedding"] = TR.scripted_positional_table(W, TR.timestamp_script(dims.n_text_ctx, TB, EOT, seed=3))
    return W


@pytest.fixture(scope="module")
def mels():
    clips = np.stack([R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0)])
    return torch.from_numpy(np.stack([R.log_mel_spectrogram(a) for a in clips]))


def _cpu_loop(dims, W, mels, keep_logits=False):
    always, first = R.suppress_lists(SP)
    with torch.no_grad():
        xa = R.encoder_forward(W, dims, mels)
    return xa, TR.greedy_with_rules(R, W, dims, xa, INIT, always, first, EOT, TB, NT, STEPS, keep_logits=keep_logits)


@pytest.fixture(scope="module")
def micro_refs(mels):
    """the CPU loop, once per weight set: (W, xa, RulesLoop)"""
    out = {}
    for name, scripted in (("lively", False), ("scripted", True)):
        W = _weights(MICRO, 7, scripted)
        xa, ref = _cpu_loop(MICRO, W, mels)
        out[name] = (W, xa, ref)
    return out


# ---------------------------------------------------------------- the rule arithmetic on crafted rows
def _step(logits, hist, n_init, m_first, m_always, rules, slp0):
    """one wipa_timestamp_step launch: ``hist`` [B, n_init + len] tokens, all rows at the same position"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    B = logits.shape[0]
    ldl, ld_tok = 51868, 16
    with on_stream() as s:
        lg = torch.zeros(B, ldl, dtype=torch.float32, device="cuda")
        lg[:, :V] = torch.from_numpy(logits).cuda()
        tk = torch.zeros(B, ld_tok, dtype=torch.int32, device="cuda")
        tk[:, : hist.shape[1]] = torch.from_numpy(hist.astype(np.int32)).cuda()
        pos = torch.tensor([hist.shape[1] - 1], dtype=torch.int32, device="cuda")
        slp = torch.from_numpy(slp0.astype(np.float32)).cuda()
        nd = torch.zeros(1, dtype=torch.int32, device="cuda")
        mf, ma = torch.from_numpy(m_first).cuda(), torch.from_numpy(m_always).cuda()
        _lib.check(L.wipa_timestamp_step(ptr(lg), ldl, B, V, ptr(mf), ptr(ma), ptr(tk), ld_tok, ptr(pos), n_init, EOT, C.byref(rules),
                                         ptr(slp), ptr(nd), sptr(s)), "wipa_timestamp_step")
        out = tk[:, hist.shape[1]].cpu().numpy().astype(np.int64), slp.cpu().numpy().astype(np.float64), int(nd.cpu()[0])
    return out


def _check_rows(logits, seqs, max_init=50):
    """B rows with histories of ONE length (the position is shared by the launch) against the restatement"""
    B = len(seqs)
    n_init = len(INIT)
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    hist = np.array([INIT + list(s) for s in seqs], dtype=np.int64)
    is_first = hist.shape[1] == n_init
    slp0 = np.linspace(-3.0, -1.0, B)
    got_tok, got_slp, got_nd = _step(logits, hist, n_init, m_first, m_always, _rules(max_init), slp0)
    fired = {k: 0 for k in TR.BRANCHES}
    want_nd = 0
    for b in range(B):
        st = TR.apply_rules(logits[b], seqs[b], TB, NT, EOT, is_first, max_init, m_first if is_first else m_always)
        latched = hist[b, -1] == EOT
        want = EOT if latched else st.next
        add = 0.0 if latched else st.logprob
        print(f"row {b}: next {got_tok[b]} (want {want})  added log-prob {got_slp[b] - slp0[b]:+.6f} (want {add:+.6f})")
        assert got_tok[b] == want, (b, got_tok[b], want)
        # the existing greedy test allows 1e-2 on a sum over 24 steps: 1e-3 for one step leaves the same slack per step
        assert abs((got_slp[b] - slp0[b]) - add) < 1e-3, (b, got_slp[b] - slp0[b], add)
        want_nd += want != EOT
        for k, f in st.fired.items():
            fired[k] += int(f and not latched)
    assert got_nd == want_nd
    return got_tok, fired


def test_timestamp_step_crafted_rows():
    rng = np.random.default_rng(11)
    a, b, c, d = 1200, 3400, 5600, 7800
    T = TB
    B = 12
    base = (rng.standard_normal((B, V)) * 2.0).astype(np.float32)
    lg = base.copy()
    seqs = [None] * B
    # 0: one text logit at 5.0 against 1501 timestamp logits at 0.0: mass log(1501) = 7.3 > 5.0, a timestamp wins (the lowest allowed)
    lg[0, :] = -30.0; lg[0, 700] = 5.0; lg[0, T:] = 0.0
    seqs[0] = [T + 0, a, T + 20, T + 20, b, c]
    # 1: the same with the timestamps at -3.0: mass 4.3 < 5.0, the text token wins
    lg[1, :] = -30.0; lg[1, 700] = 5.0; lg[1, T:] = -3.0
    seqs[1] = [T + 0, a, T + 20, T + 20, b, c]
    # 2: a closed pair, the model wants another timestamp: text only
    lg[2, T + 300] = 14.0
    seqs[2] = [T + 0, a, b, c, T + 120, T + 120]
    # 3: a single timestamp, the model wants text: EOT or a timestamp >= the last one -- the same value is permitted and is the peak
    lg[3, 700] = 14.0; lg[3, T + 120] = 9.0
    seqs[3] = [T + 0, a, b, c, d, T + 120]
    # 4: a single timestamp, EOT is the peak
    lg[4, 700] = 14.0; lg[4, EOT] = 12.0
    seqs[4] = [T + 0, a, b, c, d, T + 120]
    # 5: a row latched on EOT
    lg[5, 700] = 14.0
    seqs[5] = [T + 0, a, T + 50, T + 50, EOT, EOT]
    # 6: the trailing column 51864 (V mod 4 = 1: outside the 16-byte loads) as the arg-max
    lg[6, V - 1] = 16.0
    seqs[6] = [T + 0, a, T + 20, T + 20, b, c]
    # 7: a non-monotone forced history: the last timestamp in order is T+50, so T+100 is allowed although T+200 came before;
    #    T+30, the highest peak, is not
    lg[7, T + 30] = 16.0; lg[7, T + 100] = 14.0
    seqs[7] = [T + 200, T + 200, a, T + 50, T + 50, b]
    # 8: the trailing column as the raw peak after a closed pair: killed with every timestamp, it must neither win nor count in the sum
    lg[8, V - 1] = 16.0
    seqs[8] = [T + 0, a, b, c, T + 120, T + 120]
    # 9: a suppressed text id (SuppressTokens) as the raw peak, <|notimestamps|> next: neither may win
    lg[9, R.NON_SPEECH_TOKENS_MULTI[5]] = 16.0; lg[9, NT] = 15.0
    seqs[9] = [T + 0, a, T + 20, T + 20, b, c]
    # 10, 11: plain random rows after text / after a pair
    seqs[10] = [T + 0, a, b, c, d, a]
    seqs[11] = [a, b, T + 7, T + 7, c, d]
    got, fired = _check_rows(lg, seqs)
    assert got[0] == T + 21 and got[1] == 700 and got[2] < T and got[3] == T + 120 and got[4] == EOT and got[5] == EOT
    assert got[6] == V - 1 and got[7] == T + 100 and got[8] < T and got[9] not in (R.NON_SPEECH_TOKENS_MULTI[5], NT)
    for k in ("text_after_closed_pair", "after_single_timestamp", "monotone_cut", "timestamp_mass_over_text", "text_over_timestamp_mass"):
        assert fired[k] >= 1, fired


@pytest.mark.parametrize("length,max_init", [(0, 50), (0, -1), (0, 0), (1, 50), (2, 50)])
def test_timestamp_step_short_histories(length, max_init):
    """len(seq) of 0 (the first sampled position: timestamps only, capped / uncapped / capped at <|0.00|>), 1 and 2 (``pen`` by
    length, then by the token)"""
    rng = np.random.default_rng(20 + length)
    B, T, a, b = 12, TB, 1200, 3400
    lg = (rng.standard_normal((B, V)) * 2.0).astype(np.float32)
    lg[0, 700] = 14.0            # the model wants text
    lg[1, T + 300] = 14.0        # ... a late timestamp (past the cap of 1.00 s)
    lg[2, T + 40] = 14.0         # ... an early one
    lg[3, V - 1] = 16.0          # ... the last column
    lg[4, EOT] = 14.0
    lg[5, T:] += 2.5             # the timestamp MASS on top, no single timestamp
    pool = {0: [[]], 1: [[a], [T + 10]], 2: [[a, b], [a, T + 30], [T + 5, T + 5], [T + 5, a]]}[length]
    seqs = [pool[i % len(pool)] for i in range(B)]
    got, fired = _check_rows(lg, seqs, max_init)
    if length == 0:
        assert fired["first_position"] == B and (got >= T).all()
        if max_init >= 0:
            assert (got <= T + max_init).all()
        else:
            assert got[1] == T + 300 and got[3] == V - 1


def test_rules_entry_points_refuse_bad_rules():
    from whisper_ipa_amd import _lib

    L = _lib.lib()
    bad = _lib.DecodeRules(V, NT, 50)  # timestamp_begin == V: no timestamp column at all
    fake = C.c_void_p(0x1000)  # never dereferenced: the checks come before the launch
    rc = L.wipa_timestamp_step(fake, 51868, 2, V, fake, fake, fake, 16, fake, 3, EOT, C.byref(bad), fake, fake, None)
    assert rc != 0 and b"timestamp_begin" in L.wipa_last_error()


# ---------------------------------------------------------------- f32 end to end at the oracle's micro model
@pytest.mark.parametrize("weights", ["lively", "scripted"])
@pytest.mark.parametrize("use_graph,prefill", [(True, True), (False, True), (True, False), (False, False)])
def test_decode_with_rules_f32_bit_exact_vs_cpu_loop(micro_refs, monkeypatch, weights, use_graph, prefill):
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    W, xa, ref = micro_refs[weights]
    assert all(n >= 1 for n in ref.counts.values()), ref.counts  # every branch of the rules fires on this history
    if not prefill:
        monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    res = greedy_decode_tokens(m, xa.cuda(), INIT, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, use_graph=use_graph,
                               rules=_rules())
    print(f"{weights}: branch counts {ref.counts}; min top-2 margin {ref.margins.min():.4f}, min mass gap {ref.mass_gaps.min():.4f}; "
          f"sum_logprobs {res.sum_logprobs.tolist()} vs {ref.sum_logprobs.tolist()}")
    assert res.tokens.shape == ref.tokens.shape
    assert (res.tokens == ref.tokens).all(), (res.tokens.tolist(), ref.tokens.tolist())
    assert np.abs(res.sum_logprobs - ref.sum_logprobs).max() < 1e-2


def test_null_rules_reproduce_the_plain_entry_points(micro_refs):
    """wipa_decoder_prefill_ex / wipa_decoder_run_ex with a call that holds only n_init, eot and the masks (rules = NULL, nothing else)
    against wipa_decoder_prefill / wipa_decoder_run: tokens, log-prob sums and last-step logits bit for bit.  The micro f32 model of
    tests/golden/micro_model.npz, B = 3, 6 steps, replayed and eager."""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import _mask, _packed_for, _state_for
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    W, xa, _ = micro_refs["lively"]
    always, first = R.suppress_lists(SP)
    init = list(SP.sot_sequence_including_notimestamps(0))
    m = _model(MICRO, W, torch.float32)
    L = _lib.lib()
    B, n_init, steps = 3, len(init), 6
    pk = _packed_for(m, B, steps)
    st = _state_for(m, B, pk)
    m_always, m_first = _mask(m, always), _mask(m, list(always) + list(first))
    host_init = (C.c_int32 * n_init)(*init)
    feats = torch.cat([xa, xa[:1].flip(1)]).cuda().contiguous()  # a third clip: the first one's frames backwards
    assert feats.shape[0] == B
    with on_stream() as s:
        cfg, tab, blob, nb = C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel()
        for use_graph in (1, 0):  # replayed and eager
            out = {}
            for which in ("plain", "ex"):
                _lib.check(L.wipa_decoder_set_audio(cfg, tab, ptr(feats), blob, nb, B, sptr(s)), "set_audio")
                _lib.check(L.wipa_decoder_begin(cfg, blob, nb, B, host_init, n_init, sptr(s)), "begin")
                if which == "plain":
                    _lib.check(L.wipa_decoder_prefill(cfg, tab, blob, nb, B, n_init, EOT, ptr(m_first), ptr(m_always), use_graph, sptr(s)), "prefill")
                    _lib.check(L.wipa_decoder_run(cfg, tab, blob, nb, B, n_init, EOT, ptr(m_first), ptr(m_always), steps - 1, use_graph, sptr(s)), "run")
                else:
                    call = _lib.DecodeCall(n_init=n_init, eot=EOT, mask_first=ptr(m_first), mask_always=ptr(m_always))
                    _lib.check(L.wipa_decoder_prefill_ex(cfg, tab, blob, nb, B, C.byref(call), use_graph, sptr(s)), "prefill_ex")
                    _lib.check(L.wipa_decoder_run_ex(cfg, tab, blob, nb, B, C.byref(call), steps - 1, use_graph, sptr(s)), "run_ex")
                out[which] = (st.tokens[:, : n_init + steps].cpu().numpy().copy(), st.sum_logprobs.cpu().numpy().copy(), st.logits.cpu().numpy().copy())
            toks, slp, logits = out["plain"]
            assert len({tuple(r) for r in toks[:, n_init:].tolist()}) > 1 and np.isfinite(logits).all()  # the rows differ: not a trivial comparison
            for name, a, b in zip(("tokens", "sum_logprobs", "logits"), out["plain"], out["ex"]):
                assert a.tobytes() == b.tobytes(), (use_graph, name)


def test_rules_are_refused_where_the_step_has_no_fused_tail(micro_refs, monkeypatch):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import greedy_decode_tokens

    W, xa, _ = micro_refs["lively"]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    monkeypatch.setenv("WIPA_DECODE_TAIL", "0")
    with pytest.raises(_lib.WipaError, match="WIPA_DECODE_TAIL"):
        greedy_decode_tokens(m, xa.cuda(), INIT, always, first, EOT, max_new_tokens=4, stop_on_eot=False, rules=_rules())


# ---------------------------------------------------------------- bf16 at d = 384: the row-scan tail on written logits
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_decode_with_rules_bf16_d384_follows_the_rules_on_its_own_logits(mels, weights):
    """Free-running bf16 decode with the rules, then the path's own history replayed through forced_decode_logits: the
    restatement applied to those (unfiltered) step logits must choose the ids the device chose wherever the top-2 margin and the
    mass-comparison gap both exceed 1e-3.  Scripted table, weight seed 1: on the CPU oracle at this width it fires all six
    branches (min top-2 margin 0.068, min mass gap 2.49 over 2 x 20 steps).  ``fp8``: the same model on e4m3 decoder tables
    (the unfused step's weight-streaming GEMMs write the logits, so the rules are served as they are for bf16); its own history
    may leave the oracle's where the quantisation error exceeds a margin, so the branch counts are asserted for bf16 only."""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import forced_decode_logits, greedy_decode_tokens

    W = _weights(W384, 1, True)
    xa, ref = _cpu_loop(W384, W, mels)
    assert all(n >= 1 for n in ref.counts.values()), ref.counts
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    m = _model(W384, W, torch.bfloat16)
    if weights == "fp8":
        m.quantize_weights()
    assert _lib.lib().wipa_logits_greedy_supported(2, V, 384, _lib.WIPA_BF16) == 1  # without rules this shape takes the partials tail
    feats = xa.cuda().to(torch.bfloat16)
    n_init = len(INIT)
    res = greedy_decode_tokens(m, feats, INIT, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, rules=_rules())
    trace, chosen = forced_decode_logits(m, feats, res.tokens, n_init, always, first, EOT, rules=_rules())
    trace = trace.cpu().numpy()
    fired = {k: 0 for k in TR.BRANCHES}
    checked = left_out = 0
    for b in range(2):
        for i in range(STEPS):
            seq = res.tokens[b, n_init:n_init + i].tolist()
            st = TR.apply_rules(trace[b, i], seq, TB, NT, EOT, i == 0, 50, m_first if i == 0 else m_always)
            got = int(res.tokens[b, n_init + i])
            assert int(chosen[b, i]) == got  # the replay makes the choices the free run made
            if i > 0 and seq[-1] == EOT:
                assert got == EOT
                continue
            if st.margin > 1e-3 and st.mass_gap > 1e-3:
                assert got == st.next, (b, i, got, st.next, st.margin, st.mass_gap)
                checked += 1
                for k, f in st.fired.items():
                    fired[k] += int(f)
            else:
                left_out += 1
    print(f"{weights} d=384: {checked} steps checked, {left_out} left out; branches on the path's own history {fired}; oracle counts {ref.counts}")
    assert left_out <= 0.1 * 2 * STEPS
    if weights == "bf16":
        assert all(n >= 1 for n in fired.values()), fired
    # the bf16 path differs from the f32 oracle by its logit error only: report how far the free run followed it
    same = (res.tokens == ref.tokens).mean()
    print(f"token match with the f32 oracle loop: {same:.3f}")


# ---------------------------------------------------------------- the pipeline
def test_transcribe_batches_with_timestamps_equals_serial_decode(micro_refs):
    import whisper_ipa_amd as wipa

    W, xa, _ = micro_refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, fp16=False, sample_len=STEPS)
    batches = [xa.clone(), torch.flip(xa, dims=[0]).contiguous()]
    want = [wipa.decode(m, b.cuda(), opts) for b in batches]
    got = list(wipa.transcribe_batches(m, batches, opts, passes_in_flight=2, check_every=3))
    assert [r.index for r in got] == [0, 1]
    with torch.no_grad():
        cpu = torch.softmax(R.decoder_forward(W, MICRO, torch.full((2, 1), SP.sot, dtype=torch.long), xa)[:, 0].float(), dim=-1)[:, SP.no_speech]
    cpu_rows = [cpu.numpy(), cpu.numpy()[::-1]]
    tb = TB
    for r, w, ns in zip(got, want, cpu_rows):
        assert len(r.results) == len(w) == 2
        for j, (x, y) in enumerate(zip(r.results, w)):
            assert x.tokens == y.tokens and x.text == y.text and x.language == y.language
            assert abs(x.avg_logprob - y.avg_logprob) < 1e-4
            assert any(t >= tb for t in x.tokens) and x.tokens[0] >= tb  # the timestamp tokens stay in; the first sampled one is one
            for v in (x.no_speech_prob, y.no_speech_prob):
                assert np.isfinite(v) and abs(v - float(ns[j])) < 1e-3, (v, float(ns[j]))
    # the without_timestamps=True path stays as it was: NaN
    plain = wipa.decode(m, batches[0].cuda(), wipa.DecodingOptions(language="en", without_timestamps=True, fp16=False, sample_len=4))
    assert all(np.isnan(p.no_speech_prob) for p in plain)


# ---------------------------------------------------------------- transcribe() through the model
def test_transcribe_end_to_end_first_windows_match_decode_and_long_files_walk(micro_refs):
    """whisper_ipa_amd.transcribe on a 40 s and a 5 s clip through the package's own log-mel, encoder and timestamp decode: the
    segments of every file's first window are the splitter's cut of what ``decode(without_timestamps=False)`` gives for that
    window, the short file is done after one window, the long file goes on from the seek the splitter returned."""
    import warnings

    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.transcribe import SEGMENT_KEYS, split_segments

    W, _, _ = micro_refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        out = wipa.transcribe(m, [long, short], language="en", sample_len=STEPS, fp16=False)
    win = np.zeros((2, 480000), dtype=np.float32)
    win[0], win[1, : len(short)] = long[:480000], short
    mel = wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80)
    want = wipa.decode(m, mel, wipa.DecodingOptions(language="en", without_timestamps=False, sample_len=STEPS, fp16=False))
    advances = []
    for i, clip in enumerate((long, short)):
        assert out[i]["language"] == "en"
        segs, adv = split_segments(want[i].tokens, TB, 0.0, min(3000, len(clip) // 160))
        advances.append(adv)
        first = [s for s in out[i]["segments"] if s["seek"] == 0]
        assert [(s["start"], s["end"]) for s in first] == [(x["start"], x["end"]) for x in segs]
        for s, x in zip(first, segs):
            assert set(SEGMENT_KEYS) <= set(s) and np.isfinite(s["no_speech_prob"]) and s["temperature"] == 0.0
            assert s["tokens"] in (x["tokens"], [])  # a segment without text, or of zero length, is emptied as upstream does
            assert abs(s["avg_logprob"] - want[i].avg_logprob) < 1e-5
    assert [s["id"] for s in out[0]["segments"]] == list(range(len(out[0]["segments"])))
    assert all(s["seek"] == 0 for s in out[1]["segments"])  # 5 s: one window (segment ends are the model's timestamps, not clamped)
    seeks = sorted({s["seek"] for s in out[0]["segments"]})
    assert seeks[0] == 0 and len(seeks) >= 2 and seeks[1] == advances[0] and seeks[-1] < 4000
