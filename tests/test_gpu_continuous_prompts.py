"""GPU: continuous batching with a PROMPT PER CLIP (include/wipa.h: wipa_decoder_seek, wipa_decoder_admit_rows_prompted,
wipa_decoder_run_ex with wipa_decode_call.prompted and the PROMPTED tails; whisper_ipa_amd.continuous.decode_continuous(prompts=)) against the CPU
restatement with every clip decoded ALONE, batch of one, on its own unpadded ``[sot_prev] + history + sot_sequence`` -- slots, the
prompt room, admission columns, the prompt pass and shifts do not exist there.  ``pytest -m gpu`` on an MI355X.

Fixtures: the weight sets of tests/prompt_ref.py (MICRO, seed 7, "lively" and "scripted" with the walking script: what the model wants
next names the position it is at, so a wrong position offset behind a prompt picks a wrong token at once), the eight mixed clips and
limits of tests/test_gpu_continuous_rules.py, and the histories of tests/prompt_ref.py assigned so that every per-clip loop decides each
token by more than the f32 logit error (asserted first)."""
import numpy as np
import pytest
import torch

import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP = PR.MICRO, PR.W384, PR.SP
V, TB, NT, EOT = 51865, SP.timestamp_begin, SP.no_timestamps, SP.eot
INIT = list(PR.SOT_SEQUENCE)
LENS = [5, 27, 12, 19, 1, 22, 23, 26]
HIST = [3, 4, 2, 1, 4, 2, 3, 0]          # PR.histories()[j]: 70, 223, 17, 1, 223, 17, 70 and 0 tokens
HIST_BF16 = [3, 4, 1, 2, 0, 2]           # 70, 223, 1, 17, 0 and 17 tokens
ROOM = 224                               # the longest prompt + 1


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def mixed_features(xa: torch.Tensor, n: int) -> torch.Tensor:
    """n different feature tensors from the two fixture clips: clip i is (1 - i / (n - 1)) xa[0] + i / (n - 1) xa[1]"""
    w = torch.linspace(0.0, 1.0, n)[:, None, None]
    return ((1 - w) * xa[0:1] + w * xa[1:2]).contiguous()


def _cut(row):
    row = [int(t) for t in row]
    return row[: row.index(EOT)] if EOT in row else row


def _rules(max_init=50):
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(TB, NT, max_init)


def _options(**kw):
    from whisper_ipa_amd.decoding import DecodingOptions

    return DecodingOptions(language="en", without_timestamps=False, fp16=False, **kw)


def _sum(r):
    return r.avg_logprob * (len(r.tokens) + 1)


def _prompted(history):
    return ([SP.sot_prev] + list(history) if history else []) + INIT


def cpu_no_speech(W, dims, feats, rows):
    """softmax(decoder_forward(row up to its <|startoftranscript|>))[no_speech] per clip"""
    out = []
    with torch.no_grad():
        for i, row in enumerate(rows):
            k = len(row) - len(INIT)
            sot = R.decoder_forward(W, dims, torch.tensor([row[: k + 1]], dtype=torch.long), feats[i: i + 1])[0, -1].float()
            out.append(float(torch.softmax(sot, dim=-1)[SP.no_speech]))
    return out


@pytest.fixture(scope="module")
def refs():
    """per weight set: (W, features [8, 1500, 128], histories, per clip (ids, sum_logprobs), no-speech probabilities), computed once"""
    hist = PR.histories()
    assert [len(hist[j]) for j in HIST] == [70, 223, 17, 1, 223, 17, 70, 0]
    always, first = R.suppress_lists(SP)
    out = {}
    for name, scripted in (("lively", False), ("scripted", True)):
        W = PR.weights(MICRO, 7, scripted)
        with torch.no_grad():
            xa = R.encoder_forward(W, MICRO, PR.clip_mels())
        feats = mixed_features(xa, len(LENS))
        histories = [hist[j] for j in HIST]
        rows = []
        for i, n in enumerate(LENS):
            init = _prompted(histories[i])
            g = TR.greedy_with_rules(R, W, MICRO, feats[i: i + 1], init, always, first, EOT, TB, NT, n)
            ids, margin, gap = _cut(g.tokens[0, len(init):]), float(g.margins.min()), float(g.mass_gaps.min())
            print(f"{name} clip {i}: history {len(histories[i])}, {len(ids)} ids, sum_logprobs {float(g.sum_logprobs[0]):.5f}, "
                  f"min top-2 margin {margin:.4f}, min mass gap {gap:.4f}")
            # before any GPU result is compared: the reference decides every token by more than the f32 logit error can move
            assert margin > 5e-3 and gap > 5e-3, (name, i, margin, gap)
            rows.append((ids, float(g.sum_logprobs[0])))
        out[name] = (W, feats, histories, rows, cpu_no_speech(W, MICRO, feats, [_prompted(h) for h in histories]))
    return out


@pytest.fixture(scope="module")
def runs(refs):
    """the prompted continuous decodes the f32 tests share, per weight set: (a) 3 slots, (b) 3 slots with column_limit = 270 (the span
    bound is prompt_room 224 + 3 + 27 + 7 = 261), (c) 8 slots (no refill)"""
    from whisper_ipa_amd.continuous import decode_continuous

    out = {}
    for name, (W, feats, histories, _, _) in refs.items():
        m = _model(MICRO, W, torch.float32)
        dev = feats.cuda()
        got = {}
        for run, kw in (("slots3", dict(slots=3)), ("shifted", dict(slots=3, column_limit=270)), ("slots8", dict(slots=8))):
            stats = []
            res = decode_continuous(m, dev, _options(), sample_lens=LENS, check_every=4, stats_out=stats, prompts=histories, **kw)
            got[run] = (res, stats[0])
        out[name] = (m, dev, got)
    return out


@pytest.mark.parametrize("weights", ["lively", "scripted"])
def test_f32_prompted_refill_equals_the_per_clip_cpu_loop(refs, runs, weights):
    """8 clips with histories of 0 .. 223 tokens, 3 slots, check_every = 4, rules on: every clip's ids equal the CPU loop on its own
    unpadded [sot_prev] + history + sot_sequence, exactly; sum_logprobs within 1e-2, no-speech within 1e-3 absolute and 1e-2 relative
    (the bounds of the continuous tests without prompts)"""
    _, _, histories, rows, want_ns = refs[weights]
    for run in ("slots3", "shifted", "slots8"):
        res, stats = runs[weights][2][run]
        assert len(res) == len(LENS) and [clip for _, clip, _ in stats.admissions] == list(range(8))
        assert all(col >= ROOM for _, _, col in stats.admissions)
        for i, (r, (ids, slp)) in enumerate(zip(res, rows)):
            print(f"{weights} {run} clip {i}: sum_logprobs {_sum(r):.5f} vs {slp:.5f}; no_speech {r.no_speech_prob:.3e} vs {want_ns[i]:.3e}; ids {r.tokens}")
            assert r.tokens == ids, (run, i, r.tokens, ids)
            assert abs(_sum(r) - slp) < 1e-2
            assert np.isfinite(r.no_speech_prob) and abs(r.no_speech_prob - want_ns[i]) < 1e-3, (run, i, r.no_speech_prob, want_ns[i])
            assert abs(r.no_speech_prob / want_ns[i] - 1.0) < 1e-2, (run, i, r.no_speech_prob, want_ns[i])
    res, stats = runs[weights][2]["slots3"]
    assert stats.shifts == [] and any(col > ROOM for _, _, col in stats.admissions)  # refills above the prompt room


@pytest.mark.parametrize("weights", ["lively", "scripted"])
def test_forced_shifts_and_the_slot_count_change_nothing(runs, weights):
    """column_limit = 270 forces at least one shift, none of which takes the position below the prompt room; 8 slots admit every clip at
    the prompt room.  The three runs give the same ids, and the shifted run is bit-equal to the plain one in sum_logprobs too"""
    plain, _ = runs[weights][2]["slots3"]
    shifted, stats = runs[weights][2]["shifted"]
    many, stats8 = runs[weights][2]["slots8"]
    print(f"{weights}: shifts {stats.shifts}; admissions {stats.admissions}")
    assert stats.shifts and all(x > 0 for x in stats.shifts)
    assert all(ROOM <= col <= 270 for _, _, col in stats.admissions)
    assert all(col == ROOM for _, _, col in stats8.admissions)
    for i, (x, y, z) in enumerate(zip(plain, shifted, many)):
        assert x.tokens == y.tokens == z.tokens, (i, x.tokens, y.tokens, z.tokens)
        assert x.avg_logprob == y.avg_logprob, (i, x.avg_logprob, y.avg_logprob)


def test_sampling_draws_on_the_prompted_rows_own_positions(refs, runs):
    """temperature 0.6, seed 1, 3 slots, rules on, lively set: every clip's ids equal the CPU restatement's draw on the clip's own prompted
    row with stream (clip, 0) -- the counter's position word is the position in the row's unpadded sequence, prompt included.  With a
    temperature per clip (0, 0.6, 0, ...) the greedy clips equal the greedy run and the others the single-temperature run."""
    from whisper_ipa_amd.continuous import decode_continuous

    W, feats, histories, _, _ = refs["lively"]
    m, dev, got = runs["lively"]
    res = decode_continuous(m, dev, _options(temperature=0.6, seed=1), slots=3, sample_lens=LENS, check_every=4, prompts=histories)
    for i in range(len(LENS)):
        init = _prompted(histories[i])
        loop = PR.sample_row_loop(W, MICRO, feats[i: i + 1], init, LENS[i], 1, 0.6, (i, 0), with_rules=True)
        print(f"clip {i}: min key margin of the restatement {loop.key_margins.min():.4f}; ids {res[i].tokens}")
        assert loop.key_margins.min() > 5e-3
        assert res[i].tokens == _cut(loop.tokens[len(init):]), (i, res[i].tokens, _cut(loop.tokens[len(init):]))
        assert abs(_sum(res[i]) - loop.sum_logprob) < 1e-2
    greedy, _ = got["slots3"]
    assert any(x.tokens != y.tokens for x, y in zip(res, greedy))
    temps = [0.0 if i % 2 == 0 else 0.6 for i in range(len(LENS))]
    mixed = decode_continuous(m, dev, _options(seed=1), slots=3, sample_lens=LENS, check_every=4, prompts=histories, temperatures=temps)
    for i, t in enumerate(temps):
        assert mixed[i].tokens == (greedy[i].tokens if t == 0.0 else res[i].tokens), (i, t, mixed[i].tokens)


@pytest.mark.parametrize("absorbed", [True, False])
def test_bf16_d384_prompted_follows_the_rules_on_its_own_logits(absorbed):
    """W384, bf16, scripted table, weight seed 1, 6 clips with histories of 70, 223, 1, 17, 0 and 17 tokens through 2 slots, in the
    absorbed and in the cached cross form: the method and thresholds of test_bf16_d384_follows_the_rules_on_its_own_logits.  Every clip's
    own sequence, prompt included, is replayed through forced_decode_logits; wherever the top-2 margin and the mass gap both exceed 1e-3
    the restatement on those logits picks the id the device picked, and at most 10 % of the steps are left out.  A run with a forced
    shift is bit-equal to the run without."""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import forced_decode_logits

    W = PR.weights(W384, 1, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, W384, PR.clip_mels())
    n = len(HIST_BF16)
    feats = mixed_features(xa, n)
    hist = PR.histories()
    histories = [hist[j] for j in HIST_BF16]
    lens = [20] * n
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    m = _model(W384, W, torch.bfloat16)
    m.cross_attention = "absorbed" if absorbed else "cached"
    assert m.use_absorbed() == absorbed
    dev = feats.cuda().to(torch.bfloat16)
    stats, stats_shifted = [], []
    res = decode_continuous(m, dev, _options(), slots=2, sample_lens=lens, check_every=4, stats_out=stats, prompts=histories)
    assert len(stats[0].admissions) == n and stats[0].admissions[2][2] > ROOM and stats[0].shifts == []
    shifted = decode_continuous(m, dev, _options(), slots=2, sample_lens=lens, check_every=4, stats_out=stats_shifted, prompts=histories,
                                column_limit=ROOM + 3 + 20 + 7 + 4)
    assert stats_shifted[0].shifts, stats_shifted[0]
    for i, (x, y) in enumerate(zip(res, shifted)):
        assert x.tokens == y.tokens and x.avg_logprob == y.avg_logprob, (i, x.tokens, y.tokens, x.avg_logprob, y.avg_logprob)
    checked = left_out = total = 0
    for i in range(n):
        init = _prompted(histories[i])
        ids = res[i].tokens
        row = ids + [EOT] * (lens[i] - len(ids))  # the device's row up to the clip's limit
        # the replay opens a state with at most four tokens: the row's first three are its initial tokens there and everything behind
        # them -- the rest of the prompt, the sot sequence, the generated ids -- is the forced history; step off + k predicts generated id k
        off = len(init) - 3
        trace, _ = forced_decode_logits(m, dev[i: i + 1], np.array([init + row], dtype=np.int64), 3, always, first, EOT, rules=_rules())
        trace = trace[:, off:].cpu().numpy()
        for k in range(lens[i]):
            seq = row[:k]
            if k > 0 and seq[-1] == EOT:
                continue
            total += 1
            st = TR.apply_rules(trace[0, k], seq, TB, NT, EOT, k == 0, 50, m_first if k == 0 else m_always)
            if st.margin > 1e-3 and st.mass_gap > 1e-3:
                assert row[k] == st.next, (i, k, row[k], st.next, st.margin, st.mass_gap)
                checked += 1
            else:
                left_out += 1
    print(f"bf16 d=384 absorbed={absorbed}: {checked} steps checked, {left_out} of {total} left out; ids {[r.tokens for r in res]}")
    assert left_out <= 0.1 * total


def test_seek_admit_run_and_shift_through_the_c_abi(refs):
    """A prompted DeviceStepper with rules, 3 slots, prompt room 80: seek, one prompted and one plain clip, steps, a prompted clip over a
    finished row, an admission that has no room (left out on the device), a shift and more steps.  The token columns equal the per-clip
    loops, and the [3][B] array holds the window starts, limits and prompt lengths before and after the shift."""
    from whisper_ipa_amd.continuous import DeviceStepper
    from whisper_ipa_amd.runtime import on_stream

    W, feats, histories, rows, want_ns = refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    always, first = R.suppress_lists(SP)
    B, n_init, room = 3, len(INIT), 80
    prompts = [[SP.sot_prev] + h if h else [] for h in histories]
    L0, L2 = len(prompts[0]), len(prompts[2])
    assert (L0, L2, len(prompts[7])) == (71, 18, 0)
    with on_stream() as s:
        st = DeviceStepper(m, B, lambda clip: dev[clip], lambda clip: INIT, n_init, LENS, EOT, always, first, None, s, rules=_rules(),
                           no_speech_token=SP.no_speech, prompts=lambda clip: prompts[clip], prompt_room=room)
        assert st.pos == room and st.st.pos.cpu().item() == room and st.starts.numel() == 3 * B
        st.admit([(0, 0), (2, 7)])   # clip 0 (history 70, 5 tokens) and clip 7 (no history, 26 tokens) at column 80
        assert st.starts.cpu().tolist() == [room - L0, 0, room, LENS[0], 0, LENS[7], L0, 0, 0]
        assert st.st.tokens[0, room - L0:room + n_init].cpu().tolist() == prompts[0] + INIT
        st.run(9)                    # column 89: clip 0 has its 5 tokens (columns 83 .. 87) and has taken eot
        assert _cut(st.st.tokens[0, 83:88].cpu().tolist()) == rows[0][0]
        st.admit([(0, 2)])           # clip 2 (history 17, 12 tokens) over clip 0's row, at column 89
        before = st.st.tokens[1].cpu().tolist()
        st.admit([(1, 3, LENS[3], None, [SP.sot_prev] + [1000] * 99)])  # a prompt of 100 columns at column 89: not carried out
        assert st.st.tokens[1].cpu().tolist() == before
        assert st.starts.cpu().tolist() == [89 - L2, 0, room, LENS[2], 0, LENS[7], L2, 0, 0]
        st.run(4)                    # column 93
        st.shift(9)                  # the live windows start at 71 and 80; the position returns to 84
        assert st.pos == 84 and st.st.pos.cpu().item() == 84
        assert st.starts.cpu().tolist() == [80 - L2, 0, room - 9, LENS[2], 0, LENS[7], L2, 0, 0]
        st.run(24)                   # column 108: clip 2 has columns 83 .. 94, clip 7 columns 74 .. 99
        assert st.st.pos.cpu().item() == 108
        assert _cut(st.st.tokens[0, 83:83 + LENS[2]].cpu().tolist()) == rows[2][0]
        assert _cut(st.st.tokens[2, 74:74 + LENS[7]].cpu().tolist()) == rows[7][0]
        assert abs(st.st.sum_logprobs[0].item() - rows[2][1]) < 1e-2 and abs(st.st.sum_logprobs[2].item() - rows[7][1]) < 1e-2
        ns = st.no_speech.cpu().numpy()
        assert abs(ns[0] - want_ns[2]) < 1e-3 and abs(ns[2] - want_ns[7]) < 1e-3


class _Spy:
    """the library with every function that is looked up recorded by name, and the wipa_decode_call of every wipa_decoder_run_ex call
    recorded as (continuous, rules, prompted, rows of the starts array it was built for)"""

    def __init__(self, lib, seen, run_calls):
        self._lib, self._seen, self._run_calls = lib, seen, run_calls

    def __getattr__(self, name):
        self._seen.append(name)
        fn = getattr(self._lib, name)
        if name != "wipa_decoder_run_ex":
            return fn

        def recorded(*a):
            k = a[5]._obj  # the DecodeCall behind C.byref
            self._run_calls.append((bool(k.continuous), bool(k.rules), bool(k.prompted), bool(k.starts_dev)))
            return fn(*a)

        return recorded


NEW_ENTRY_POINTS = ("wipa_decoder_seek", "wipa_decoder_admit_rows_prompted", "wipa_decoder_admit_prompted_workspace_bytes")
UNPROMPTED, PROMPTED = (True, True, False, True), (True, True, True, True)  # continuous with rules on a starts array, without / with .prompted


def test_without_prompts_nothing_else_moved(refs, monkeypatch):
    """decode_continuous and transcribe(schedule="continuous") without prompts call none of the new entry points and no seek, every
    run call they make is continuous with rules and NOT prompted, and their admissions start at column 0; with prompts the same spy sees
    the new entry points and prompted run calls only (so it would have seen them)"""
    import warnings

    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd import continuous as CT

    W, feats, histories, _, _ = refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    real, seen, run_calls = _lib.lib(), [], []
    monkeypatch.setattr(CT._lib, "lib", lambda: _Spy(real, seen, run_calls))
    stats = []
    CT.decode_continuous(m, dev, _options(), slots=3, sample_lens=LENS, check_every=4, stats_out=stats)
    assert "wipa_decoder_admit_rows" in seen and run_calls and set(run_calls) == {UNPROMPTED}, run_calls
    assert not [name for name in seen if name in NEW_ENTRY_POINTS], seen
    assert stats[0].admissions[0][2] == 0 and min(col for _, _, col in stats[0].admissions) == 0
    del seen[:], run_calls[:]
    tstats = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        wipa.transcribe(m, _files(), language="en", sample_len=20, fp16=False, schedule="continuous", slots=2, check_every=8, stats_out=tstats)
    assert "wipa_decoder_admit_rows" in seen and run_calls and set(run_calls) == {UNPROMPTED}, run_calls
    assert not [name for name in seen if name in NEW_ENTRY_POINTS], seen
    assert tstats[0].prompt_budget is None and tstats[0].prompts == []
    assert tstats[0].schedule.admissions[0][2] == 0 and min(col for _, _, col in tstats[0].schedule.admissions) == 0
    del seen[:], run_calls[:]
    CT.decode_continuous(m, dev, _options(), slots=3, sample_lens=LENS, check_every=4, prompts=histories)
    assert all(name in seen for name in NEW_ENTRY_POINTS), seen
    assert "wipa_decoder_admit_rows" not in seen and run_calls and set(run_calls) == {PROMPTED}, run_calls


# ---------------------------------------------------------------- transcribe(): conditioning on both schedules
def _files():
    """the files of tests/test_gpu_continuous_rules.py::test_transcribe_continuous_equals_rounds: 40 s, 5 s, 65 s and 12 s"""
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]
    longer = np.concatenate([R.synthetic_clip(3, 30.0), R.synthetic_clip(4, 30.0), R.synthetic_clip(5, 30.0)[: 5 * 16000]])
    mid = R.synthetic_clip(6, 30.0)[: 12 * 16000]
    return [long, short, longer, mid]


INITIAL_PROMPT = "the quick brown fox jumps over the lazy dog and then it walks all the way home again, slowly, through the rain"


@pytest.mark.parametrize("more", [dict(), dict(seed=5), dict(prompt_budget=20)], ids=["greedy", "fallback", "budget20"])
def test_transcribe_conditioned_continuous_equals_rounds(more):
    """condition_on_previous_text=True with an initial_prompt, f32, slots = 2, sample_len = 20: schedule="continuous" gives the segments,
    tokens and temperatures of schedule="rounds" -- greedy, with the temperature fallback (seed; logprob_threshold is the midpoint of the
    two middle window avg_logprob values of a first rounds run without a threshold, so about half the windows retry, as in
    test_transcribe_with_a_seed_continuous_equals_rounds), and with prompt_budget = 20 on both"""
    import warnings

    import whisper_ipa_amd as wipa

    m = _model(MICRO, PR.weights(MICRO, 7, True), torch.float32)  # the walking script: its text ids decode to text, so histories grow
    files = _files()
    kw = dict(language="en", sample_len=20, fp16=False, condition_on_previous_text=True, initial_prompt=INITIAL_PROMPT, **more)
    stats = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        if "seed" in more:
            probe = wipa.transcribe(m, files, **{**kw, "seed": None, "logprob_threshold": None})
            per_window = sorted({(i, s["seek"]): s["avg_logprob"] for i, r in enumerate(probe) for s in r["segments"]}.values())
            assert len(per_window) >= 4
            mid = len(per_window) // 2
            kw["logprob_threshold"] = 0.5 * (per_window[mid - 1] + per_window[mid])
            print(f"{len(per_window)} windows, avg_logprob {per_window[0]:.4f} .. {per_window[-1]:.4f}; logprob_threshold {kw['logprob_threshold']:.4f}")
        rounds = wipa.transcribe(m, files, **kw)
        cont = wipa.transcribe(m, files, schedule="continuous", slots=2, check_every=8, stats_out=stats, **kw)
    st = stats[0]
    print(f"{more}: prompt budget {st.prompt_budget}; prompts (file, seek, history, kept) {st.prompts}; retries {st.retries}; "
          f"shifts {st.schedule.shifts}")
    assert any(kept > 0 for _, _, _, kept in st.prompts)
    n_initial = min(history for _, _, history, _ in st.prompts)  # every file's first window carries the initial prompt alone
    assert any(history > n_initial for _, _, history, _ in st.prompts), "no window was conditioned on previous text"
    assert st.prompt_budget == more.get("prompt_budget", 223)
    if "prompt_budget" in more:
        assert any(kept < history for _, _, history, kept in st.prompts) and all(kept <= 20 for _, _, _, kept in st.prompts)
    if "seed" in more:
        assert st.retries and any(s["temperature"] > 0.0 for r in cont for s in r["segments"])
        assert not any(s.get("needs_fallback") for r in cont for s in r["segments"])
    assert all(col >= st.prompt_budget + 1 for _, _, col in st.schedule.admissions)
    for i, (x, y) in enumerate(zip(cont, rounds)):
        assert x["text"] == y["text"] and x["language"] == y["language"], (i, x["text"], y["text"])
        assert len(x["segments"]) == len(y["segments"]) >= 1, (i, len(x["segments"]), len(y["segments"]))
        for s, t in zip(x["segments"], y["segments"]):
            for k in ("seek", "start", "end", "tokens", "text", "id", "temperature"):
                assert s[k] == t[k], (i, k, s[k], t[k])
            assert abs(s["avg_logprob"] - t["avg_logprob"]) * 21 < 1e-2  # sample_len = 20: len + 1 <= 21
            assert abs(s["no_speech_prob"] - t["no_speech_prob"]) < 1e-3
    assert len({s["seek"] for s in cont[0]["segments"]}) >= 2 and len({s["seek"] for s in cont[2]["segments"]}) >= 2  # the long files walk
