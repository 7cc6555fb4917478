"""CPU: the streaming scheduler of the continuous decode (whisper_ipa_amd.continuous.run_stream) against a fake stepper and a source of
files whose windows exist one at a time; the keyword that lets ``refuse_unserved`` pass ``without_timestamps=False``; what
``transcribe(schedule="continuous")`` refuses; the window bookkeeping both schedules of ``transcribe`` share, through a fake continuous
decoder at the ``stream_fn`` seam; and the refusals of a continuous wipa_decoder_run_ex call with rules.  No GPU."""
import warnings
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

N_INIT, EOT, N_CTX = 3, 9, 128


class FakeStepper:
    """slots x N_CTX token table.  A clip is (file, window); its k-th generated token is 1000 * (file + 1) + 10 * window + k, and it says
    EOT after ``lengths[clip]`` tokens or at its limit, as the CONTINUOUS tails do on the device.  Sums and no-speech values are functions
    of the clip, so a value read from the wrong row, or after the slot was given away, shows."""

    def __init__(self, slots, lengths):
        self.slots, self.lengths = slots, lengths
        self.tokens = np.full((slots, N_CTX), EOT, dtype=np.int64)
        self.start, self.clip, self.limit = [0] * slots, [None] * slots, [0] * slots
        self.pos = 0
        self.snapshots = 0
        self.log = []

    def admit(self, triples):
        self.log.append(("admit", [(slot, clip) for slot, clip, _ in triples], self.pos))
        for slot, clip, limit in triples:
            assert self.pos + N_INIT < N_CTX
            self.clip[slot], self.start[slot], self.limit[slot] = clip, self.pos, limit
            self.tokens[slot, self.pos:self.pos + N_INIT] = [1, 2, 3]

    def run(self, n):
        for _ in range(n):
            p = self.pos
            assert p + 1 < N_CTX, "a step past the table"
            for slot in range(self.slots):
                clip = self.clip[slot]
                if clip is None:
                    continue
                own = self.start[slot] + N_INIT
                if p + 1 < own:
                    continue
                k = p + 1 - own
                if self.tokens[slot, p] == EOT or k >= self.limit[slot] or k >= self.lengths[clip]:
                    self.tokens[slot, p + 1] = EOT
                else:
                    self.tokens[slot, p + 1] = 1000 * (clip[0] + 1) + 10 * clip[1] + k
            self.pos += 1

    def snapshot(self):
        self.snapshots += 1
        sums = np.array([-1.0 if c is None else -(c[0] + 0.1 * c[1]) for c in self.clip], dtype=np.float32)
        nsp = np.array([0.0 if c is None else 0.01 * (10 * c[0] + c[1]) for c in self.clip], dtype=np.float32)
        return self.tokens[:, : self.pos + 1].copy(), sums, nsp

    def shift(self, shift):
        assert 0 < shift <= self.pos
        n = self.pos + 1 - shift
        self.tokens[:, :n] = self.tokens[:, shift:shift + n].copy()
        self.pos -= shift
        self.start = [max(s - shift, 0) for s in self.start]
        self.log.append(("shift", shift, self.pos))


class FileSource:
    """files of ``windows[f]`` windows each, at most one window of a file in flight, at most ``places`` files in progress"""

    def __init__(self, windows, places, limit):
        self.windows, self.places, self.limit = windows, places, limit
        self.waiting = list(range(len(windows)))
        self.active, self.ready = [], []
        self.next = [0] * len(windows)
        self.in_flight = set()
        self.out = {}
        self.events = []

    def pending(self):
        while self.waiting and len(self.active) < self.places:
            f = self.waiting.pop(0)
            self.active.append(f)
            self.ready.append(f)
        out = []
        for f in self.ready:
            assert f not in self.in_flight, "two windows of one file are live"
            self.in_flight.add(f)
            out.append(((f, self.next[f]), self.limit))
            self.events.append(("pending", (f, self.next[f])))
        self.ready = []
        return out

    def retired(self, clip, tokens, sum_logprob, no_speech):
        f, w = clip
        assert clip not in self.out and f in self.in_flight and w == self.next[f]
        self.in_flight.discard(f)
        self.out[clip] = (list(tokens), sum_logprob, no_speech)
        self.events.append(("retired", clip))
        self.next[f] += 1
        if self.next[f] < self.windows[f]:
            self.ready.append(f)
        else:
            self.active.remove(f)


WINDOWS = [3, 1, 4, 2, 1]  # 5 files, 1 - 4 windows each
LENGTHS = {(f, w): 1 + (5 * f + 3 * w) % 11 for f, n in enumerate(WINDOWS) for w in range(n)}  # 1 .. 11 tokens, scripted
LENGTHS[(2, 1)] = 50  # one window runs into its limit


def _stream(column_limit=None, slots=2, check_every=4, limit=12):
    from whisper_ipa_amd.continuous import run_stream

    st = FakeStepper(slots, LENGTHS)
    src = FileSource(WINDOWS, slots, limit)
    stats = run_stream(st, src, slots, N_INIT, EOT, N_CTX, check_every, column_limit)
    return st, src, stats


def _want(clip, limit=12):
    f, w = clip
    return [1000 * (f + 1) + 10 * w + k for k in range(min(LENGTHS[clip], limit))]


def test_run_stream_files_of_windows_through_two_slots():
    st, src, stats = _stream()
    clips = [(f, w) for f, n in enumerate(WINDOWS) for w in range(n)]
    # every window is retired exactly once, with its own tokens and the values of its own row
    assert sorted(src.out) == clips and sorted(stats.retired) == clips and len(stats.retired) == len(clips)
    for clip in clips:
        tokens, slp, nsp = src.out[clip]
        assert tokens == _want(clip), (clip, tokens)
        assert slp == pytest.approx(-(clip[0] + 0.1 * clip[1])) and nsp == pytest.approx(0.01 * (10 * clip[0] + clip[1]))
    # files are admitted in input order, a file's windows in order (FileSource asserts that no file has two windows live)
    admitted = [clip for _, clip, _ in stats.admissions]
    assert len(admitted) == len(clips)
    firsts = [f for f, w in admitted if w == 0]
    assert firsts == sorted(firsts) == list(range(5))
    for f, n in enumerate(WINDOWS):
        assert [w for g, w in admitted if g == f] == list(range(n))
    # a window is admitted only after its predecessor has retired
    for clip in clips:
        if clip[1] > 0:
            assert src.events.index(("retired", (clip[0], clip[1] - 1))) < src.events.index(("pending", clip))
    # two slots, never more than two files in progress; groups add up to the admissions; one snapshot per check
    assert all(slot in (0, 1) for slot, _, _ in stats.admissions)
    assert sum(stats.groups) == len(clips) and stats.groups[0] == 2
    assert st.snapshots == stats.steps // 4
    assert st.clip.count(None) == 0 and stats.shifts == []


def test_run_stream_shifts_change_no_result():
    _, plain, ps = _stream()
    st, shifted, ss = _stream(column_limit=32)  # n_init + limit + 2 * check_every - 1 = 22 is the smallest a limit of 12 takes
    assert ss.shifts and all(x > 0 for x in ss.shifts)
    assert [e[1] for e in st.log if e[0] == "shift"] == ss.shifts
    assert shifted.out == plain.out
    assert ss.steps == ps.steps and [a[:2] for a in ss.admissions] == [a[:2] for a in ps.admissions]
    assert all(0 <= col <= 32 for _, _, col in ss.admissions)
    from whisper_ipa_amd.continuous import run_stream

    with pytest.raises(ValueError, match="limit"):  # a clip whose limit does not fit the column window is refused when it is admitted
        run_stream(FakeStepper(2, LENGTHS), FileSource(WINDOWS, 2, 12), 2, N_INIT, EOT, N_CTX, 4, 21)


def test_run_stream_ends_on_an_empty_source_and_with_more_slots_than_files():
    from whisper_ipa_amd.continuous import run_stream

    st = FakeStepper(4, LENGTHS)
    stats = run_stream(st, FileSource([], 4, 12), 4, N_INIT, EOT, N_CTX, 4)
    assert stats.steps == 0 and stats.admissions == [] and st.log == []
    st, src, stats = _stream(slots=8)
    assert sorted(src.out) == sorted(LENGTHS) and stats.groups[0] == 5
    assert all(src.out[c][0] == _want(c) for c in src.out)


def test_run_schedule_keeps_its_stats():
    """the existing scheduler's results are what they were (tests/test_continuous_host.py derives them): 64 steps, shifts 20 and 12"""
    from test_continuous_host import _run

    _, stats = _run([None] * 8, [5, 27, 12, 19, 1, 22, 23, 26], slots=3, column_limit=40)
    assert stats.steps == 64 and stats.shifts == [20, 12] and stats.groups == []


def test_refuse_unserved_keeps_the_refusal_and_gains_a_keyword():
    from whisper_ipa_amd.continuous import refuse_unserved
    from whisper_ipa_amd.decoding import DecodingOptions

    class M:
        _fp8 = {}

    timed = DecodingOptions(without_timestamps=False)
    with pytest.raises(NotImplementedError, match="without_timestamps=False"):
        refuse_unserved(M(), timed)
    refuse_unserved(M(), timed, timestamps=True)
    refuse_unserved(M(), DecodingOptions(without_timestamps=False, temperature=0.6, seed=1), timestamps=True)
    with pytest.raises(NotImplementedError, match="best_of"):  # the keyword opens nothing else
        refuse_unserved(M(), DecodingOptions(without_timestamps=False, best_of=3, temperature=0.5, seed=1), timestamps=True)


# ---------------------------------------------------------------- transcribe(schedule="continuous")
T = 50364
a, b, c, d = 1000, 1001, 1002, 1003


class _Tok:
    """what transcribe() needs of a tokenizer: ids 1000.. render as letters"""
    timestamp_begin, eot = T, 50257

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)


def _never_decode(windows, languages):
    raise AssertionError("something was decoded")  # and a decoder that returned nothing would leave the window loop standing still


@pytest.mark.parametrize("kw,name", [
    (dict(seed=1), "seed"),
    (dict(word_timestamps=True), "word_timestamps"),
    (dict(condition_on_previous_text=True), "condition_on_previous_text"),
    (dict(initial_prompt="hello"), "initial_prompt"),
    (dict(best_of=3), "best_of"),
    (dict(decode_fn=_never_decode), "decode_fn"),
])
def test_transcribe_continuous_refuses_by_name_before_anything_is_decoded(kw, name):
    from whisper_ipa_amd.transcribe import transcribe

    def never(source, slots, check_every):
        raise AssertionError("something was decoded")

    with pytest.raises(NotImplementedError, match=name):
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_Tok(), **kw)


def test_transcribe_continuous_refuses_fp8_models_and_unknown_schedules():
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(16000, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="fp8"):
        transcribe(SimpleNamespace(_fp8={"x": 1}), audio, schedule="continuous", stream_fn=lambda *x, **k: None, tokenizer=_Tok())
    with pytest.raises(ValueError, match="schedule"):
        transcribe(None, audio, schedule="lockstep", decode_fn=_never_decode, tokenizer=_Tok())


def _scripted(first_sample: float):
    """a window's result as a function of the window's own first sample (which tells its file and its start): tokens, log-probability
    sum and no-speech probability"""
    k = int(round(first_sample))
    f, sec = k // 1000, k % 1000
    table = {
        0: ([T + 0, a, T + 100, T + 100, b, c], -1.2, 0.1),       # advance 2.00 s
        2: ([T + 0, b, c, c, c, T + 500], -2.0, 0.2),              # single ending: the whole window
        32: ([T + 0, d], -4.5, 0.9),                               # silent and unsure: skipped
        62: ([T + 0, d, T + 200, T + 200], -0.5, 0.9),             # no-speech overridden by the log-probability
        66: ([T + 0, a, b], -0.9, 0.1),
    }
    tokens, slp, nsp = table.get(sec, ([T + 0, a + f % 4, T + 150, T + 150], -0.4 - 0.1 * f, 0.05))
    if f == 3:
        slp = -9.0  # file 3 fails the log-probability threshold: needs_fallback and the one warning
    return tokens, slp, nsp


def _files():
    """four files of 75, 5, 31 and 12 s; sample s * 16000 of file f holds 1000 * f + s"""
    out = []
    for f, secs in enumerate((75, 5, 31, 12)):
        x = np.zeros(secs * 16000, dtype=np.float32)
        x[::16000] = 1000.0 * f + np.arange(secs, dtype=np.float32)
        out.append(x)
    return out


def test_transcribe_both_schedules_share_the_window_bookkeeping():
    """the same scripted per-window tokens through ``schedule="rounds"`` (a fake decode_fn) and ``schedule="continuous"`` (a fake stream
    at the ``stream_fn`` seam, which retires one window per call in an order of its own): equal results, segment for segment"""
    from whisper_ipa_amd.transcribe import transcribe

    tok = _Tok()

    def decode_fn(windows, languages):
        out = []
        for w, lang in zip(windows, languages):
            tokens, slp, nsp = _scripted(w[0])
            text = tok.decode([t for t in tokens if t < T]).strip()
            comp = len(text.encode()) / len(zlib.compress(text.encode())) if text else float("nan")
            out.append(SimpleNamespace(tokens=tokens, avg_logprob=slp / (len(tokens) + 1), no_speech_prob=nsp, compression_ratio=comp,
                                       temperature=0.0, language=lang or "en"))
        return out

    seen = []

    def stream_fn(source, slots, check_every):
        assert slots == 2 and check_every == 8
        live = []
        while True:
            new = source.pending()
            if new:
                clips = [clip for clip, _ in new]
                windows, languages = source.group(clips)
                assert windows.shape == (len(clips), 480000) and windows.dtype == np.float32
                unknown = [j for j, lang in enumerate(languages) if lang is None]
                if unknown:
                    source.detected([clips[j] for j in unknown], ["en"] * len(unknown))
                live += [(clip, w[0]) for clip, w in zip(clips, windows)]
                seen.append(clips)
            if not live:
                return "stats"
            assert len(live) <= slots and len({clip[0] for clip, _ in live}) == len(live)  # one window per file, two files at most
            clip, first = live.pop()  # the newest first: retirement order is not admission order
            tokens, slp, nsp = _scripted(first)
            source.retired(clip, tokens, slp, nsp)

    with warnings.catch_warnings(record=True) as w_rounds:
        warnings.simplefilter("always")
        rounds = transcribe(None, _files(), decode_fn=decode_fn, tokenizer=tok)
    stats = []
    with warnings.catch_warnings(record=True) as w_cont:
        warnings.simplefilter("always")
        cont = transcribe(None, _files(), schedule="continuous", slots=2, stream_fn=stream_fn, tokenizer=tok, stats_out=stats)
    assert cont == rounds
    assert [s["seek"] for s in cont[0]["segments"]] == [0, 200, 6200, 6600] and cont[0]["text"] == "abcccdab"
    assert all(s.get("needs_fallback") for s in cont[3]["segments"]) and not any(s.get("needs_fallback") for s in cont[1]["segments"])
    for w in (w_rounds, w_cont):
        assert len([x for x in w if "needs_fallback" in str(x.message)]) == 1
    st = stats[0]
    assert st.schedule == "stats" and st.rows == 2 and st.waited == [2, 3]
    assert st.groups == seen and st.groups[0] == [(0, 0), (1, 0)]
    assert st.detected == [[(0, 0), (1, 0)], [(2, 0)], [(3, 0)]]  # language=None: every file's first window, nothing else
    decoded = [clip for g in st.groups for clip in g]
    assert len(decoded) == len(set(decoded))  # every window once
    assert set(decoded) == {(i, s["seek"]) for i in range(4) for s in cont[i]["segments"]} | {(0, 3200)}  # the skipped window was decoded too


# ---------------------------------------------------------------- the C ABI
def test_abi_has_the_entry_point():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    assert "wipa_decoder_run_ex" in _lib.SIGNATURES and hasattr(_lib.lib(), "wipa_decoder_run_ex")
    assert {"continuous", "rules", "no_speech_dev", "no_speech_token"} <= {f for f, _ in _lib.DecodeCall._fields_}


def test_run_continuous_rules_refuses_by_name_before_any_launch():
    """With rules on a continuous call: fp8 tables, candidate groups, a missing starts array, a no-speech column outside the vocabulary,
    a no-speech array without rules and a wrong count of initial tokens are refused with a message that names the entry point and the
    field; the pointers are never dereferenced"""
    import __graft_entry__ as g

    g.build()
    from decode_call_util import FAKE, fp8_cfg, refusal, small_cfg
    from whisper_ipa_amd import _lib

    cfg = small_cfg(_lib)
    on = dict(rules=True, continuous=1, starts_dev=FAKE, no_speech_dev=FAKE, no_speech_token=50362)
    assert "call.continuous needs call.starts_dev" in refusal(_lib, "run", cfg, **{**on, "starts_dev": None})
    assert "fp8" in refusal(_lib, "run", fp8_cfg(_lib), **on)
    assert "candidate groups" in refusal(_lib, "run", small_cfg(_lib, dec_n_group=2), **on)
    assert "call.no_speech_token=51865" in refusal(_lib, "run", cfg, **{**on, "no_speech_token": 51865})
    assert "call.no_speech_token=-1" in refusal(_lib, "run", cfg, **{**on, "no_speech_token": -1})
    assert "call.no_speech_dev needs call.rules" in refusal(_lib, "run", cfg, **{**on, "rules": False})
    assert "initial tokens" in refusal(_lib, "run", cfg, **{**on, "no_speech_dev": None, "n_init": 5})
