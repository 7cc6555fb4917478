"""CPU: the timestamp rules' numpy restatement against a fixture recorded from transformers' WhisperTimeStampLogitsProcessor,
the segment splitter's known answers, the ``transcribe()`` window loop on scripted decodes, and the option refusals.
Reference: mlx_whisper.transcribe as scripts/evaluate_model.py:112-119 of the reference calls it (openai-whisper's decoding.py /
transcribe.py state the algorithm; mlx_whisper 0.4.3's port is [UPSTREAM-UNVERIFIED])."""
import json
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import timestamp_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "timestamp_rules.json")


def test_restatement_matches_the_recorded_processor():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    doc = json.load(open(GOLDEN))
    v, cases = doc["vocab"], doc["cases"]
    assert len(cases) >= 40
    fired = {k: 0 for k in TR.BRANCHES}
    lens, last_col_wins, uncapped = set(), 0, 0
    for c in cases:
        logits = TR.case_logits(c["seed"], c["scale"], c["boosts"], v["n_vocab"], v["timestamp_begin"])
        seq = c["history"][c["begin_index"]:]
        cap = c["max_initial_timestamp_index"]
        st = TR.apply_rules(logits, seq, v["timestamp_begin"], v["no_timestamps"], v["eot"], len(seq) == 0, -1 if cap is None else cap)
        e = c["expected"]
        assert st.next == e["argmax"], (c["name"], st.next, e)
        assert int(np.isfinite(st.row).sum()) == e["n_finite"], (c["name"], int(np.isfinite(st.row).sum()), e)
        # the processor's row is float32, the restatement float64: 1e-4 is ~100 x the f32 rounding of a log-sum over 51 865 terms
        assert abs(st.logprob - e["logprob"]) < 1e-4, (c["name"], st.logprob, e)
        for k, f in st.fired.items():
            fired[k] += int(f)
        lens.add(min(len(seq), 2))
        last_col_wins += e["argmax"] == v["n_vocab"] - 1
        uncapped += cap is None
    # the fixture covers what the issue names: every branch, len(seq) of 0, 1 and 2, a non-monotone history, no cap, the last column
    assert all(n >= 1 for n in fired.values()), fired
    assert lens == {0, 1, 2} and last_col_wins >= 1 and uncapped >= 1
    assert any("non_monotone" in c["name"] for c in cases)


def test_the_last_timestamp_in_order_rules_not_the_maximum():
    tb, nt, eot, V = 100, 99, 50, 140
    l = np.zeros(V)
    seq = [tb + 30, tb + 30, 7, tb + 5, tb + 5, 8]  # forced: decreasing
    st = TR.apply_rules(l, seq, tb, nt, eot, False)
    assert np.isfinite(st.row[tb + 6]) and not np.isfinite(st.row[tb + 5])  # cut below t + 1 with t = tb + 5, not tb + 30


# ---------------------------------------------------------------- the splitter
T = 50364
a, b, c, d = 1000, 1001, 1002, 1003


def _spans(segs):
    return [(round(s["start"], 2), round(s["end"], 2)) for s in segs]


def test_splitter_known_answers():
    from whisper_ipa_amd.transcribe import split_segments

    segs, adv = split_segments([T + 0, a, b, T + 100, T + 100, c, T + 250, T + 250, d, T + 400], T, 0.0, 3000)
    assert _spans(segs) == [(0.0, 2.0), (2.0, 5.0), (5.0, 8.0)] and adv == 3000
    assert [s["tokens"] for s in segs] == [[T + 0, a, b, T + 100], [T + 100, c, T + 250], [T + 250, d, T + 400]]
    segs, adv = split_segments([T + 0, a, T + 100, T + 100, b, c], T, 0.0, 3000)
    assert _spans(segs) == [(0.0, 2.0)] and adv == 200  # the tail b, c is dropped: decoded again from the next seek
    segs, adv = split_segments([T + 0, a, b], T, 0.0, 3000)
    assert _spans(segs) == [(0.0, 30.0)] and adv == 3000
    segs, adv = split_segments([T + 0, a, T + 150], T, 0.0, 3000)
    assert _spans(segs) == [(0.0, 3.0)] and adv == 3000
    # a time offset shifts both ends; a short last window spans its own content only
    segs, adv = split_segments([T + 0, a, b], T, 60.0, 1500)
    assert _spans(segs) == [(60.0, 75.0)] and adv == 1500
    segs, adv = split_segments([T + 0, a, T + 100, T + 100, b, c], T, 30.0, 3000)
    assert _spans(segs) == [(30.0, 32.0)] and adv == 200


# ---------------------------------------------------------------- the window loop
class _Tok:
    """what transcribe() needs of a tokenizer: ids 1000.. render as letters"""
    timestamp_begin, eot = T, 50257

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)


def _res(tokens, avg_logprob=-0.3, no_speech_prob=0.1, compression_ratio=1.2):
    return SimpleNamespace(tokens=tokens, avg_logprob=avg_logprob, no_speech_prob=no_speech_prob, compression_ratio=compression_ratio,
                           temperature=0.0, language="en")


def test_transcribe_loop_seeks_offsets_skip_and_fallback():
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(75 * 16000, dtype=np.float32)
    audio[::16000] = np.arange(75, dtype=np.float32)  # sample s * 16000 holds s: a window's first sample tells its start
    script = [
        _res([T + 0, a, T + 100, T + 100, b, c]),                     # seek 0: one segment, advance 200 frames (2.00 s)
        _res([T + 0, b, c, T + 500], compression_ratio=3.0),          # seek 200: single ending, whole window; too repetitive
        _res([T + 0, d], avg_logprob=-1.5, no_speech_prob=0.9),       # seek 3200: silent and unsure -> skipped
        _res([T + 0, d, T + 200, T + 200], avg_logprob=-0.2, no_speech_prob=0.9),  # seek 6200: no-speech overridden by the log-prob
        _res([T + 0, a, b]),                                          # seek 6600: the last 9 s, one segment spanning them
    ]
    calls = []

    def decode_fn(windows, languages):
        assert windows.shape == (1, 480000) and windows.dtype == np.float32
        calls.append((float(windows[0, 0]), int(np.flatnonzero(windows[0])[-1]) if windows[0].any() else 0, languages[0]))
        return [script[len(calls) - 1]]

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = transcribe(None, audio, decode_fn=decode_fn, tokenizer=_Tok())
    assert len(calls) == 5
    assert [c0[0] for c0 in calls] == [0.0, 2.0, 32.0, 62.0, 66.0]  # the windows start at seek / 100 seconds
    assert calls[-1][1] == 8 * 16000  # the last window holds 9 s of content (its last non-zero sample is second 74), zero-padded after
    assert [c0[2] for c0 in calls] == [None, "en", "en", "en", "en"]  # language detected on the first window, kept afterwards
    segs = out["segments"]
    assert [s["seek"] for s in segs] == [0, 200, 6200, 6600]
    assert _spans(segs) == [(0.0, 2.0), (2.0, 12.0), (62.0, 66.0), (66.0, 75.0)]
    assert [s["id"] for s in segs] == [0, 1, 2, 3]
    assert [s.get("needs_fallback", False) for s in segs] == [False, True, False, False]
    assert len([x for x in w if "needs_fallback" in str(x.message)]) == 1
    assert [s["text"] for s in segs] == ["a", "bc", "d", "ab"] and out["text"] == "abcdab" and out["language"] == "en"
    for s in segs:
        assert set(s) - {"needs_fallback"} == {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob",
                                               "compression_ratio", "no_speech_prob"}


def test_transcribe_batches_the_next_windows_of_all_files():
    from whisper_ipa_amd.transcribe import transcribe

    long, short = np.zeros(40 * 16000, dtype=np.float32), np.zeros(10 * 16000, dtype=np.float32)
    rounds = []

    def decode_fn(windows, languages):
        rounds.append(len(windows))
        return [_res([T + 0, a, b]) for _ in range(len(windows))]

    out = transcribe(None, [long, short], language="en", decode_fn=decode_fn, tokenizer=_Tok())
    assert rounds == [2, 1]  # round 1: both files' first windows in one batch; round 2: the long file's second window
    assert _spans(out[0]["segments"]) == [(0.0, 30.0), (30.0, 40.0)] and _spans(out[1]["segments"]) == [(0.0, 10.0)]


@pytest.mark.parametrize("kw,name", [
    (dict(condition_on_previous_text=True), "condition_on_previous_text"),
    (dict(initial_prompt="hello"), "initial_prompt"),
    (dict(word_timestamps=True), "word_timestamps"),
    (dict(clip_timestamps="0,10"), "clip_timestamps"),
    (dict(hallucination_silence_threshold=2.0), "hallucination_silence_threshold"),
    (dict(temperature=0.2), "temperature"),
    (dict(temperature=(0.2, 0.4)), "temperature"),
    (dict(beam_size=5), "beam_size"),
    (dict(best_of=5), "best_of"),
])
def test_transcribe_refuses_what_it_does_not_serve(kw, name):
    from whisper_ipa_amd.transcribe import transcribe

    with pytest.raises(NotImplementedError, match=name):
        transcribe(None, np.zeros(16000, dtype=np.float32), decode_fn=lambda w, l: [], tokenizer=_Tok(), **kw)


def test_decode_refuses_sampling_beams_and_prompts():
    from whisper_ipa_amd.decoding import DecodingOptions, _refuse_unsupported, timestamp_rules

    for kw in (dict(temperature=0.2), dict(beam_size=5), dict(best_of=5)):
        with pytest.raises(NotImplementedError):
            _refuse_unsupported(DecodingOptions(**kw))
    with pytest.raises(NotImplementedError, match="prompt"):
        _refuse_unsupported(DecodingOptions(prompt="x", without_timestamps=False))
    _refuse_unsupported(DecodingOptions(without_timestamps=False))  # the timestamp path itself is served
    tok = SimpleNamespace(timestamp_begin=50364, no_timestamps=50363)
    assert timestamp_rules(tok).max_initial_timestamp_index == 50 and timestamp_rules(tok, None).max_initial_timestamp_index == -1
    assert timestamp_rules(tok, 0.0).max_initial_timestamp_index == 0 and timestamp_rules(tok).timestamp_begin == 50364


def test_decode_with_timestamps_renders_the_tokens():
    from whisper_ipa_amd.tokenizer import get_tokenizer

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, language="en", task="transcribe")
    tb = tok.timestamp_begin
    ids = tok.encode("hi")
    assert tok.decode_with_timestamps([tb, *ids, tb + 617]) == "<|0.00|>hi<|12.34|>"
    assert tok.decode([tb, *ids, tb + 617]) == "hi"
