"""GPU: continuous batching under the timestamp rules (include/wipa.h: wipa_decode_call.continuous with .rules and the CONTINUOUS tails with
rules; whisper_ipa_amd.continuous.decode_continuous(without_timestamps=False), run_stream; transcribe(schedule="continuous")) against
the CPU restatement of tests/timestamp_ref.py with every clip decoded ALONE, batch of one, to its own limit -- slots, refill, admission
columns and shifts do not exist there.  ``pytest -m gpu`` on an MI355X.

Fixtures: the two weight sets of tests/test_gpu_timestamps.py (MICRO, seed 7, "lively" and "scripted") and the clips of
tests/test_gpu_continuous.py (eight mixes of the two fixture clips, limits 5, 27, 12, 19, 1, 22, 23, 26, 3 slots, a check every 4
steps).  A slot's next clip is admitted at a column above 0 over a row that ended in timestamp tokens: rules that scanned the row from
a common first column would read those as the new clip's history."""
import warnings

import numpy as np
import pytest
import torch

import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP = PR.MICRO, PR.W384, PR.SP
V, TB, NT, EOT = 51865, SP.timestamp_begin, SP.no_timestamps, SP.eot
INIT = [SP.sot, SP.lang_first, SP.transcribe]  # tok.sot_sequence
LENS = [5, 27, 12, 19, 1, 22, 23, 26]
LENS_BF16 = [3, 20, 1, 9, 20, 11]


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def _weights(dims, seed, scripted):
    W = R.synthetic_weights(dims, seed=seed)
    if scripted:
        W["decoder.positional_embedding"] = TR.scripted_positional_table(W, TR.timestamp_script(dims.n_text_ctx, TB, EOT, seed=3))
    return W


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


def cpu_no_speech(W, dims, feats):
    """softmax(decoder_forward(SOT))[no_speech] per clip: upstream's logits[:, sot_index]"""
    with torch.no_grad():
        sot = torch.full((feats.shape[0], 1), SP.sot, dtype=torch.long)
        return torch.softmax(R.decoder_forward(W, dims, sot, feats)[:, 0].float(), dim=-1)[:, SP.no_speech].numpy()


def cpu_rows(W, dims, feats, lens):
    """every clip alone through the CPU loop with rules, to its own limit: (ids before EOT, sum_logprobs, min margin, min mass gap), and
    the branch counts over all clips"""
    always, first = R.suppress_lists(SP)
    counts = {k: 0 for k in TR.BRANCHES}
    out = []
    for i, n in enumerate(lens):
        g = TR.greedy_with_rules(R, W, dims, feats[i: i + 1], INIT, always, first, EOT, TB, NT, n)
        for k, v in g.counts.items():
            counts[k] += v
        out.append((_cut(g.tokens[0, len(INIT):]), float(g.sum_logprobs[0]), float(g.margins.min()), float(g.mass_gaps.min())))
    return out, counts


@pytest.fixture(scope="module")
def refs():
    """per weight set: (W, features [8, 1500, 128], the per-clip CPU loop, branch counts, no-speech probabilities), computed once"""
    out = {}
    for name, scripted in (("lively", False), ("scripted", True)):
        W = _weights(MICRO, 7, scripted)
        with torch.no_grad():
            xa = R.encoder_forward(W, MICRO, PR.clip_mels())
        feats = mixed_features(xa, len(LENS))
        rows, counts = cpu_rows(W, MICRO, feats, LENS)
        for i, (ids, slp, margin, gap) in enumerate(rows):
            print(f"{name} clip {i}: {len(ids)} ids, sum_logprobs {slp:.5f}, min top-2 margin {margin:.4f}, min mass gap {gap:.4f}")
            # before any GPU result is compared: the reference decides every token by more than the f32 logit error (3e-5 .. 2.1e-4,
            # README) can move, the bound tests/test_gpu_continuous.py asks of its reference
            assert margin > 5e-3 and gap > 5e-3, (name, i, margin, gap)
        out[name] = (W, feats, rows, counts, cpu_no_speech(W, MICRO, feats))
    return out


@pytest.fixture(scope="module")
def runs(refs):
    """the continuous decodes the f32 tests share, per weight set: 3 slots, 3 slots with column_limit = 40, 8 slots (no refill)"""
    from whisper_ipa_amd.continuous import decode_continuous

    out = {}
    for name, (W, feats, _, _, _) in refs.items():
        m = _model(MICRO, W, torch.float32)
        dev = feats.cuda()
        got = {}
        for run, kw in (("slots3", dict(slots=3)), ("shifted", dict(slots=3, column_limit=40)), ("slots8", dict(slots=8))):
            stats = []
            res = decode_continuous(m, dev, _options(), sample_lens=LENS, check_every=4, stats_out=stats, **kw)
            got[run] = (res, stats[0])
        out[name] = (m, dev, got)
    return out


def _ends_in_timestamp(ids):
    return bool(ids) and ids[-1] >= TB


@pytest.mark.parametrize("weights", ["lively", "scripted"])
def test_f32_refill_equals_the_per_clip_cpu_loop(refs, runs, weights):
    """8 clips, 3 slots, check_every = 4: every clip's ids equal the CPU loop with rules on that clip alone, exactly; sum_logprobs within
    the 1e-2 the rules and continuous tests allow against that loop.  Every branch of the rules fires in the reference, and at least one
    clip starts above column 0 in a slot whose previous clip ended in timestamp tokens."""
    _, _, rows, counts, _ = refs[weights]
    res, stats = runs[weights][2]["slots3"]
    assert all(n >= 1 for n in counts.values()), counts
    assert len(res) == len(LENS) and stats.shifts == []
    assert [clip for _, clip, _ in stats.admissions] == list(range(8))
    over_timestamps = []
    last_in_slot = {}
    for slot, clip, col in stats.admissions:
        if col > 0 and slot in last_in_slot and _ends_in_timestamp(rows[last_in_slot[slot]][0]):
            over_timestamps.append((slot, last_in_slot[slot], clip, col))
        last_in_slot[slot] = clip
    print(f"{weights}: branch counts {counts}; admissions over a row that ended in timestamps (slot, previous, clip, column): {over_timestamps}")
    assert over_timestamps
    for i, (r, (ids, slp, _, _)) in enumerate(zip(res, rows)):
        print(f"clip {i}: sum_logprobs {_sum(r):.5f} vs {slp:.5f}; ids {r.tokens}")
        assert r.tokens == ids, (i, r.tokens, ids)
        assert abs(_sum(r) - slp) < 1e-2
    assert any(any(t >= TB for t in r.tokens) for r in res)


@pytest.mark.parametrize("weights", ["lively", "scripted"])
def test_forced_shifts_and_the_slot_count_change_no_id(runs, weights):
    """column_limit = 40 forces a shift in both runs (with three initial tokens the live rows stand at columns 20, 24 and 32 when the
    column counter reaches 40, on either weight set); 8 slots refill nothing"""
    plain, _ = runs[weights][2]["slots3"]
    shifted, stats = runs[weights][2]["shifted"]
    many, stats8 = runs[weights][2]["slots8"]
    assert stats.shifts and stats.shifts[0] == 20 and all(x > 0 for x in stats.shifts)
    assert all(0 <= col <= 40 for _, _, col in stats.admissions)
    assert all(col == 0 for _, _, col in stats8.admissions)
    for i, (x, y, z) in enumerate(zip(plain, shifted, many)):
        assert x.tokens == y.tokens, (i, x.tokens, y.tokens)
        assert x.tokens == z.tokens, (i, x.tokens, z.tokens)


@pytest.mark.parametrize("weights", ["lively", "scripted"])
def test_no_speech_prob_from_the_tail(refs, runs, weights):
    """no_speech_prob of every clip is within 1e-3 (the bound of test_transcribe_batches_with_timestamps_equals_serial_decode) of the CPU
    restatement's softmax(decoder_forward(SOT))[no_speech] -- for clips admitted at column 0, mid-table, and in a run with shifts"""
    want = refs[weights][4]
    for run in ("slots3", "shifted", "slots8"):
        res, stats = runs[weights][2][run]
        assert any(col > 0 for _, _, col in stats.admissions) or run == "slots8"
        for i, r in enumerate(res):
            print(f"{weights} {run} clip {i}: no_speech_prob {r.no_speech_prob:.6f} vs {float(want[i]):.6f}")
            assert np.isfinite(r.no_speech_prob) and abs(r.no_speech_prob - float(want[i])) < 1e-3, (run, i, r.no_speech_prob, float(want[i]))
            # these models put 1e-6 .. 1e-11 on <|nospeech|>, so the absolute bound alone would pass a zero: an f32 logit error of
            # 2.1e-4 (README) moves a log-probability by at most twice that, a relative error below 1e-3; 1e-2 is asked
            assert abs(r.no_speech_prob / float(want[i]) - 1.0) < 1e-2, (run, i, r.no_speech_prob, float(want[i]))


def test_sampling_with_rules_draws_on_the_clips_own_sequence(refs, runs):
    """temperature 0.6, seed 1, 3 slots, with rules: every clip's ids equal the CPU restatement's draw on that clip alone with stream
    (clip, 0).  The restatement's smallest key margin is checked first: a draw decided by less than the f32 logit error can move is no
    reference (5e-3, the bound tests/test_gpu_continuous.py asks)."""
    from whisper_ipa_amd.continuous import decode_continuous

    W, feats, _, _, _ = refs["lively"]
    m, dev, got = runs["lively"]
    res = decode_continuous(m, dev, _options(temperature=0.6, seed=1), slots=3, sample_lens=LENS, check_every=4)
    for i in range(len(LENS)):
        loop = PR.sample_row_loop(W, MICRO, feats[i: i + 1], INIT, LENS[i], 1, 0.6, (i, 0), with_rules=True)
        print(f"clip {i}: min key margin of the restatement {loop.key_margins.min():.4f}; ids {res[i].tokens}")
        assert loop.key_margins.min() > 5e-3
        assert res[i].tokens == _cut(loop.tokens[len(INIT):]), (i, res[i].tokens, _cut(loop.tokens[len(INIT):]))
        assert abs(_sum(res[i]) - loop.sum_logprob) < 1e-2
    greedy, _ = got["slots3"]
    assert any(x.tokens != y.tokens for x, y in zip(res, greedy))


def test_bf16_d384_follows_the_rules_on_its_own_logits():
    """W384, bf16 (the absorbed form; without rules this shape takes the partials tail), scripted table, weight seed 1, 6 clips through 2
    slots.  Every clip's own history is replayed through forced_decode_logits; wherever the top-2 margin and the mass gap both exceed
    1e-3 the restatement on those logits picks the id the device picked, and at most 10 % of the steps are left out: the cap, the
    weights and the form of test_decode_with_rules_bf16_d384_follows_the_rules_on_its_own_logits (there the oracle's minimum margin is
    0.068 and its minimum mass gap 2.49)."""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import forced_decode_logits

    W = _weights(W384, 1, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, W384, PR.clip_mels())
    feats = mixed_features(xa, len(LENS_BF16))
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    m = _model(W384, W, torch.bfloat16)
    assert m.use_absorbed()
    dev = feats.cuda().to(torch.bfloat16)
    stats = []
    res = decode_continuous(m, dev, _options(), slots=2, sample_lens=LENS_BF16, check_every=4, stats_out=stats)
    assert len(stats[0].admissions) == 6 and stats[0].admissions[2][2] > 0
    n_init = len(INIT)
    checked = left_out = total = 0
    for i, n in enumerate(LENS_BF16):
        ids = res[i].tokens
        row = ids + [EOT] * (n - len(ids))  # the device's row up to the clip's limit
        hist = np.array([INIT + row], dtype=np.int64)
        trace, chosen = forced_decode_logits(m, dev[i: i + 1], hist, n_init, always, first, EOT, rules=_rules())
        trace = trace.cpu().numpy()
        for k in range(n):
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
    print(f"bf16 d=384: {checked} steps checked, {left_out} of {total} left out")
    assert left_out <= 0.1 * total


def test_admit_run_and_shift_through_the_c_abi(refs):
    """DeviceStepper with rules drives admit, steps, a second admission at a later column, a shift and more steps through
    continuous wipa_decoder_run_ex calls with rules, 3 slots: the token columns of each row equal the same clip decoded alone"""
    from whisper_ipa_amd.continuous import DeviceStepper
    from whisper_ipa_amd.runtime import on_stream

    W, feats, rows, _, want_ns = refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    always, first = R.suppress_lists(SP)
    B, n_init = 3, len(INIT)
    with on_stream() as s:
        st = DeviceStepper(m, B, lambda clip: dev[clip], lambda clip: INIT, n_init, LENS, EOT, always, first, None, s, rules=_rules(),
                           no_speech_token=SP.no_speech)
        st.admit([(0, 2), (2, 0)])   # clips 2 (12 tokens) and 0 (5 tokens) at column 0
        st.run(9)                    # column 9: clip 0 has its 5 tokens (columns 3 .. 7) and has taken eot twice
        assert _cut(st.st.tokens[2, 3:8].cpu().tolist()) == rows[0][0]
        st.admit([(2, 3), (1, 5)])   # clip 3 over clip 0's row, which ended in what the rules gave it; clip 5 into the idle slot
        st.run(4)                    # column 13
        assert st.starts.cpu().tolist() == [0, 9, 9, LENS[2], LENS[5], LENS[3]]
        st.run(2)                    # column 15: clip 2 has its 12 tokens (columns 3 .. 14)
        assert _cut(st.st.tokens[0, 3:15].cpu().tolist()) == rows[2][0]
        st.shift(9)                  # the live rows start at 9
        assert st.pos == 6 and st.st.pos.cpu().item() == 6
        assert st.starts.cpu().tolist() == [0, 0, 0, 0, LENS[5], LENS[3]]
        st.run(24)                   # clips 5 (22 tokens) and 3 (19 tokens) from column 3 on
        assert _cut(st.st.tokens[1, 3:3 + LENS[5]].cpu().tolist()) == rows[5][0]
        assert _cut(st.st.tokens[2, 3:3 + LENS[3]].cpu().tolist()) == rows[3][0]
        assert abs(st.st.sum_logprobs[1].item() - rows[5][1]) < 1e-2 and abs(st.st.sum_logprobs[2].item() - rows[3][1]) < 1e-2
        ns = st.no_speech.cpu().numpy()
        assert abs(ns[1] - want_ns[5]) < 1e-3 and abs(ns[2] - want_ns[3]) < 1e-3 and abs(ns[0] - want_ns[2]) < 1e-3


# ---------------------------------------------------------------- transcribe() on both schedules
def _files():
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])          # 40 s
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]                                                        # 5 s
    longer = np.concatenate([R.synthetic_clip(3, 30.0), R.synthetic_clip(4, 30.0), R.synthetic_clip(5, 30.0)[: 5 * 16000]])  # 65 s
    mid = R.synthetic_clip(6, 30.0)[: 12 * 16000]                                                        # 12 s
    return [long, short, longer, mid]


@pytest.fixture(scope="module")
def transcripts(refs):
    import whisper_ipa_amd as wipa

    W = refs["scripted"][0]
    m = _model(MICRO, W, torch.float32)
    files = _files()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        for language in ("en", None):
            stats = []
            rounds = wipa.transcribe(m, files, language=language, sample_len=20, fp16=False)
            cont = wipa.transcribe(m, files, language=language, sample_len=20, fp16=False, schedule="continuous", slots=2, check_every=8,
                                   stats_out=stats)
            out[language] = (rounds, cont, stats[0])
    return out


@pytest.mark.parametrize("language", ["en", None])
def test_transcribe_continuous_equals_rounds(transcripts, language):
    """a 40 s, a 5 s, a 65 s and a 12 s file, slots = 2, sample_len = 20, f32: the same segments per file on both schedules"""
    rounds, cont, stats = transcripts[language]
    assert len(rounds) == len(cont) == 4
    for i, (x, y) in enumerate(zip(cont, rounds)):
        assert x["text"] == y["text"] and x["language"] == y["language"], (i, x["text"], y["text"])
        assert len(x["segments"]) == len(y["segments"]) >= 1, (i, len(x["segments"]), len(y["segments"]))
        for s, t in zip(x["segments"], y["segments"]):
            for k in ("seek", "start", "end", "tokens", "text", "id"):
                assert s[k] == t[k], (i, k, s[k], t[k])
            n = len(s["tokens"])
            print(f"file {i} seek {s['seek']}: avg_logprob {s['avg_logprob']:.6f} vs {t['avg_logprob']:.6f}, "
                  f"no_speech_prob {s['no_speech_prob']:.6f} vs {t['no_speech_prob']:.6f}")
            assert abs(s["no_speech_prob"] - t["no_speech_prob"]) < 1e-3
            assert s.get("needs_fallback", False) == t.get("needs_fallback", False)
    # avg_logprob x (len + 1), per window: the window's tokens are its segments' decoded tokens, of which a segment dict may hold fewer
    # (emptied segments), so the factor is taken from the rounds schedule's result of the same window
    for i, (x, y) in enumerate(zip(cont, rounds)):
        for seek in sorted({s["seek"] for s in x["segments"]}):
            a = [s for s in x["segments"] if s["seek"] == seek][0]
            b = [s for s in y["segments"] if s["seek"] == seek][0]
            assert abs(a["avg_logprob"] - b["avg_logprob"]) * 21 < 1e-2  # sample_len = 20: at most 20 tokens, len + 1 <= 21
    assert len({s["seek"] for s in cont[0]["segments"]}) >= 2 and len({s["seek"] for s in cont[2]["segments"]}) >= 2  # the long files walk


def test_transcribe_continuous_files_wait_for_a_slot_and_detect_once(transcripts):
    _, _, stats = transcripts["en"]
    assert stats.rows == 2 and stats.waited == [2, 3]  # files 2 and 3 waited for a slot
    assert stats.groups[0] == [(0, 0), (1, 0)] and stats.detected == []
    first_of = {}
    for slot, (f, seek), col in stats.schedule.admissions:
        first_of.setdefault(f, col)
    assert first_of[0] == first_of[1] == 0 and first_of[2] > 0 and first_of[3] > 0
    assert sum(stats.schedule.groups) == sum(len(g) for g in stats.groups) == len(stats.schedule.retired)
    _, cont, stats = transcripts[None]
    looked = [clip for call in stats.detected for clip in call]
    assert sorted(looked) == [(0, 0), (1, 0), (2, 0), (3, 0)]  # language=None: detected on each file's first window only
    assert all(r["language"] is not None for r in cont)
