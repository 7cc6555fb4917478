"""CPU: the temperature fallback on the continuous schedule.  ``run_stream`` with draws (a source that hands a clip out again with a
temperature, an attempt and a stream of its own) against a scripted stepper; ``transcribe(seed=S)`` on both schedules with scripted
decodes -- a fake ``decode_fn`` + ``fallback_fn`` on the rounds side, a fake ``stream_fn`` that declares ``retries`` on the continuous
side; what stays refused; the host image of the sampling record with a row part; and the refusals of
wipa_decoder_run_ex with wipa_decode_call.sample_rows.  No GPU."""
import ctypes as C
import struct
import warnings
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from test_continuous_rules_host import EOT, LENGTHS, N_CTX, N_INIT, WINDOWS, FakeStepper, FileSource, _Tok, _want

T = 50364
a, b, c, d = 1000, 1001, 1002, 1003


# ---------------------------------------------------------------- run_stream with draws
class DrawStepper(FakeStepper):
    """FakeStepper that takes (slot, clip, limit, draw) and remembers what it was given, with the column"""

    def __init__(self, slots, lengths):
        super().__init__(slots, lengths)
        self.given = []

    def admit(self, entries):
        assert all(len(e) == 4 for e in entries)
        self.given += [(slot, clip, draw, self.pos) for slot, clip, _, draw in entries]
        super().admit([e[:3] for e in entries])


class RetrySource:
    """clips 0 .. n-1, each needing ``tries[clip]`` attempts: a clip whose attempt is not its last is handed out AGAIN, with the draw
    (0.2 * attempt, attempt, (clip, 7)); attempt 0 comes with draw None"""

    def __init__(self, tries, limit):
        self.tries, self.limit = tries, limit
        self.ready = [(clip, 0) for clip in range(len(tries))]
        self.attempt = {clip: 0 for clip in range(len(tries))}
        self.out, self.events = {}, []

    def pending(self):
        out = [((clip, 0), self.limit, (0.2 * k, k, (clip, 7)) if k else None) for clip, k in self.ready]
        self.events += [("pending", clip, k) for clip, k in self.ready]
        self.ready = []
        return out

    def retired(self, clip, tokens, sum_logprob, no_speech):
        f = clip[0]
        k = self.attempt[f]
        self.events.append(("retired", f, k))
        if k + 1 < self.tries[f]:
            self.attempt[f] = k + 1
            self.ready.append((f, k + 1))
        else:
            self.out[f] = (list(tokens), k)


def test_run_stream_hands_draws_to_admit_and_readmits_at_the_same_check():
    from whisper_ipa_amd.continuous import run_stream

    tries = [1, 3, 2, 1]
    lengths = {(f, 0): 2 + 3 * f for f in range(4)}  # 2, 5, 8, 11 tokens
    st = DrawStepper(4, lengths)  # a slot per clip, as transcribe gives every active file a row: a retry finds the slot it left
    src = RetrySource(tries, 12)
    stats = run_stream(st, src, 4, N_INIT, EOT, N_CTX, 4)
    # every attempt of every clip reached admit once, with the draw its source gave
    want = sorted((f, k) for f, n in enumerate(tries) for k in range(n))
    assert sorted((clip[0], draw[1] if draw else 0) for _, clip, draw, _ in st.given) == want
    for _, clip, draw, _ in st.given:
        assert draw is None or draw == (0.2 * draw[1], draw[1], (clip[0], 7))
    assert sum(1 for g in st.given if g[2] is not None) == sum(n - 1 for n in tries) == 3
    # a clip handed out again is admitted at the check that retired it: at the column the stepper stood at, into a slot that was free
    column_of = {}
    for e in st.log:
        if e[0] == "admit":
            for _, clip in e[1]:
                column_of.setdefault(clip[0], []).append(e[2])
    for f, n in enumerate(tries):
        cols = column_of[f]
        assert len(cols) == n
        for k in range(1, n):
            own = cols[k - 1] + N_INIT
            generated = lengths[(f, 0)] + 1  # its tokens and the eot behind them
            first_check = next(p for p in range(4, N_CTX, 4) if p - own + 1 >= generated)  # the first check that sees the row's eot
            assert cols[k] == first_check, (f, k, cols, first_check)
    assert stats.shifts == [] and sum(stats.groups) == len(st.given) == 7
    # the tokens of a clip are those of its LAST attempt's occupancy (the fake's tokens do not depend on the attempt)
    for f in range(4):
        assert src.out[f] == ([1000 * (f + 1) + k for k in range(lengths[(f, 0)])], tries[f] - 1)
    # pending -> retired -> pending again, in this order, for every retry
    for f, n in enumerate(tries):
        for k in range(1, n):
            assert src.events.index(("retired", f, k - 1)) < src.events.index(("pending", f, k)) < src.events.index(("retired", f, k))


def test_run_stream_takes_pairs_as_before():
    """a source of (clip, limit) pairs reaches a stepper that unpacks triples, as tests/test_continuous_rules_host.py runs it"""
    from whisper_ipa_amd.continuous import run_stream

    st = FakeStepper(2, LENGTHS)  # its admit unpacks (slot, clip, limit): a fourth element would raise
    src = FileSource(WINDOWS, 2, 12)
    stats = run_stream(st, src, 2, N_INIT, EOT, N_CTX, 4)
    assert sorted(src.out) == sorted(LENGTHS) and all(src.out[clip][0] == _want(clip) for clip in src.out)
    assert stats.steps > 0 and sum(stats.groups) == len(LENGTHS)
    # mixed: a triple with draw None is a 4-tuple for admit
    st2 = DrawStepper(1, {(0, 0): 2})
    src2 = RetrySource([1], 4)
    run_stream(st2, src2, 1, N_INIT, EOT, N_CTX, 4)
    assert st2.given == [(0, (0, 0), None, 0)]


# ---------------------------------------------------------------- transcribe(seed=S) on both schedules
TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def _scripted(first_sample: float, attempt: int):
    """a window's result as a function of its own first sample (file and start) and the attempt: tokens, log-probability sum, no-speech
    probability.  Windows end in a single timestamp, so each consumes all its frames."""
    k = int(round(first_sample))
    passing = ([T + 0, a + attempt % 4, b, T + 500], -1.0, 0.1)          # avg -0.2
    failing = ([T + 0, c, d, a + attempt % 3, T + 400], -9.0 - attempt, 0.1)  # avg <= -1.5
    if k == 0:       # file 0, first window: passes at temperature 0
        return passing
    if k == 30:      # file 0, second window: passes at its second retry
        return passing if attempt >= 2 else failing
    if k == 1000:    # file 1: fails to the end of the schedule
        return failing
    if k == 2000:    # file 2: silent and unsure -- the silence exception: no retry, and the window is skipped
        return ([T + 0, d, T + 300], -9.0, 0.9)
    if k == 3000:    # file 3, first window: passes at its first retry
        return passing if attempt >= 1 else failing
    return passing   # file 3, second window (k = 3030)


def _files():
    """four files of 40, 5, 12 and 31 s; sample s * 16000 of file f holds 1000 * f + s"""
    out = []
    for f, secs in enumerate((40, 5, 12, 31)):
        x = np.zeros(secs * 16000, dtype=np.float32)
        x[::16000] = 1000.0 * f + np.arange(secs, dtype=np.float32)
        out.append(x)
    return out


def _result(tok, first, attempt, language):
    tokens, slp, nsp = _scripted(first, attempt)
    text = tok.decode([t for t in tokens if t < T]).strip()
    comp = len(text.encode()) / max(len(zlib.compress(text.encode())), 1) if text else float("nan")
    return SimpleNamespace(tokens=tokens, avg_logprob=slp / (len(tokens) + 1), no_speech_prob=nsp, compression_ratio=comp,
                           temperature=TEMPS[attempt], language=language or "en", first=first)


def test_transcribe_with_a_seed_both_schedules_retry_the_same_windows():
    from whisper_ipa_amd.transcribe import transcribe

    tok = _Tok()
    drawn_rounds, drawn_cont = [], []

    def decode_fn(windows, languages):
        return [_result(tok, w[0], 0, lang) for w, lang in zip(windows, languages)]

    def fallback_fn(results, languages, *, temperature, attempt, streams, seed):
        assert seed == 5
        drawn_rounds.extend((float(temperature), int(attempt), tuple(s)) for s in streams)
        return [_result(tok, r.first, attempt, lang) for r, lang in zip(results, languages)]

    seen = []

    def stream_fn(source, slots, check_every):
        first, live = {}, []
        while True:
            new = source.pending()
            assert all(len(e) == 3 for e in new)  # with a seed: (clip, limit, draw)
            fresh = [clip for clip, _, draw in new if draw is None]
            if fresh:
                windows, languages = source.group(fresh)
                unknown = [j for j, lang in enumerate(languages) if lang is None]
                if unknown:
                    source.detected([fresh[j] for j in unknown], ["en"] * len(unknown))
                for clip, w in zip(fresh, windows):
                    assert clip not in first, "a window was encoded twice"
                    first[clip] = w[0]
                seen.append(fresh)
            for clip, _, draw in new:
                if draw is not None:
                    assert clip in first, "a retry of a window that was never admitted"
                    drawn_cont.append((float(draw[0]), int(draw[1]), tuple(draw[2])))
                live.append((clip, draw))
            if not live:
                return "stats"
            assert len(live) <= slots and len({clip[0] for clip, _ in live}) == len(live)  # one window per file in flight
            clip, draw = live.pop()
            tokens, slp, nsp = _scripted(first[clip], draw[1] if draw else 0)
            source.retired(clip, tokens, slp, nsp)

    stream_fn.retries = True
    with warnings.catch_warnings(record=True) as w_rounds:
        warnings.simplefilter("always")
        rounds = transcribe(None, _files(), decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=tok, seed=5)
    stats = []
    with warnings.catch_warnings(record=True) as w_cont:
        warnings.simplefilter("always")
        cont = transcribe(None, _files(), schedule="continuous", slots=2, stream_fn=stream_fn, tokenizer=tok, seed=5, stats_out=stats)
    assert cont == rounds  # segment for segment: seek, start, end, tokens, text, temperature, avg_logprob, ...
    # the temperatures that produced the segments; no needs_fallback where a retry ran (nor anywhere: every failing window was retried)
    assert [s["temperature"] for s in cont[0]["segments"]] == [0.0, 0.4] and [s["seek"] for s in cont[0]["segments"]] == [0, 3000]
    assert [s["temperature"] for s in cont[1]["segments"]] == [1.0]      # failed to the end: the last attempt is kept
    assert cont[2]["segments"] == []                                      # the silence exception: not retried, then skipped
    assert [s["temperature"] for s in cont[3]["segments"]] == [0.2, 0.0]
    for res in (rounds, cont):
        assert not any(s.get("needs_fallback") for r in res for s in r["segments"])
    for w in (w_rounds, w_cont):
        assert not [x for x in w if "needs_fallback" in str(x.message)]
    # the retries' (temperature, attempt, stream) are the same on both sides; stream = (seek, file index)
    want = [(TEMPS[k], k, (3000, 0)) for k in (1, 2)] + [(TEMPS[k], k, (0, 1)) for k in (1, 2, 3, 4, 5)] + [(TEMPS[1], 1, (0, 3))]
    assert sorted(drawn_rounds) == sorted(drawn_cont) == sorted(want)
    st = stats[0]
    assert st.schedule == "stats" and st.rows == 2 and st.waited == [2, 3]
    windows = [(0, 0), (0, 3000), (1, 0), (2, 0), (3, 0), (3, 3000)]
    assert st.groups == seen and sorted(clip for g in st.groups for clip in g) == windows  # every window once: fresh windows only
    assert sorted(st.retries) == sorted((stream[1], stream[0], k) for _, k, stream in want)
    for f in (0, 1, 3):  # a window's attempts come in order
        ks = [k for g, _, k in st.retries if g == f]
        assert ks == list(range(1, len(ks) + 1))
    assert st.detected == [[(0, 0), (1, 0)], [(2, 0)], [(3, 0)]]  # language=None: every file's first window, no retry among them


def test_transcribe_without_a_seed_keeps_the_flag_on_the_continuous_schedule():
    """seed=None: pending() returns pairs, nothing is retried, the failing windows carry needs_fallback and one warning is printed"""
    from whisper_ipa_amd.transcribe import transcribe

    tok = _Tok()

    def stream_fn(source, slots, check_every):
        while True:
            new = source.pending()
            if not new:
                return None
            assert all(len(e) == 2 for e in new)
            windows, _ = source.group([clip for clip, _ in new])
            source.detected([clip for clip, _ in new], ["en"] * len(new))
            for (clip, _), w in zip(new, windows):
                source.retired(clip, *_scripted(w[0], 0))

    stats = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = transcribe(None, _files(), schedule="continuous", slots=2, stream_fn=stream_fn, tokenizer=tok, stats_out=stats)
    assert stats[0].retries == []
    assert all(s.get("needs_fallback") for s in out[1]["segments"]) and all(s["temperature"] == 0.0 for r in out for s in r["segments"])
    assert len([x for x in caught if "needs_fallback" in str(x.message)]) == 1


def _never_stream(source, slots, check_every):
    raise AssertionError("something was decoded")


def _never_decode(windows, languages):
    raise AssertionError("something was decoded")


def test_seed_is_refused_for_a_stream_fn_that_does_not_declare_retries():
    from whisper_ipa_amd.transcribe import transcribe

    with pytest.raises(NotImplementedError, match="seed"):
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=_never_stream, tokenizer=_Tok(), seed=1)


@pytest.mark.parametrize("kw,name", [
    (dict(word_timestamps=True), "word_timestamps"),
    (dict(condition_on_previous_text=True), "condition_on_previous_text"),
    (dict(initial_prompt="hello"), "initial_prompt"),
    (dict(best_of=3), "best_of"),
    (dict(decode_fn=_never_decode), "decode_fn"),
])
def test_the_other_options_stay_refused_with_a_seed(kw, name):
    from whisper_ipa_amd.transcribe import transcribe

    def never(source, slots, check_every):
        raise AssertionError("something was decoded")

    never.retries = True
    with pytest.raises(NotImplementedError, match=name):
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_Tok(), seed=1, **kw)
    with pytest.raises(NotImplementedError, match="fp8"):
        transcribe(SimpleNamespace(_fp8={"x": 1}), np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_Tok(),
                   seed=1)


def test_decode_continuous_refuses_temperatures_without_a_seed_or_beside_a_temperature():
    import torch

    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import DecodingOptions

    m = SimpleNamespace(_fp8=None)
    x = torch.zeros(2, 3000, 80)
    with pytest.raises(NotImplementedError, match="seed"):
        decode_continuous(m, x, DecodingOptions(without_timestamps=True), temperatures=[0.0, 0.2])
    with pytest.raises(ValueError, match="temperatures"):
        decode_continuous(m, x, DecodingOptions(without_timestamps=True, temperature=0.4, seed=1), temperatures=[0.0, 0.2])
    with pytest.raises(ValueError, match="temperatures"):
        decode_continuous(m, x, DecodingOptions(without_timestamps=True, seed=1), temperatures=[0.0, -0.2])
    with pytest.raises(ValueError, match="attempts"):
        decode_continuous(m, x, DecodingOptions(without_timestamps=True, seed=1), temperatures=[0.0, 0.2], attempts=[0, 65536])
    with pytest.raises(ValueError, match="attempts"):
        decode_continuous(m, x, DecodingOptions(without_timestamps=True, seed=1), attempts=[0, 1])


# ---------------------------------------------------------------- the record with a row part, on the host
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    return _lib.lib()


def test_rows_record_image_for_a_known_seed(lib):
    B = 3
    n = lib.wipa_sample_rows_bytes(B)
    assert n == 16 + 16 * B and lib.wipa_sample_rows_bytes(0) == 0
    img = np.full(n, 0xAB, dtype=np.uint8)
    assert lib.wipa_sample_rows_fill(img.ctypes.data, n, 0x1122334455667788, B) == 0
    words = img.view(np.uint32)
    assert words[:4].tolist() == [0x55667788, 0x11223344, B, 0]
    for r in range(B):  # every row greedy: stream (row, 0), attempt 0, 1 / T = +0.0
        assert words[4 + 4 * r: 8 + 4 * r].tolist() == [r, 0, 0, 0]
    assert lib.wipa_sample_rows_fill(img.ctypes.data, n - 1, 1, B) != 0 and b"wipa_sample_rows_fill" in lib.wipa_last_error()
    # one row: temperature 0.5 at attempt 3 on stream (7, 9); temperature 0 gives 1 / T = 0.0, the greedy mark
    assert lib.wipa_sample_rows_fill_row(img.ctypes.data, n, B, 1, 7, 9, 3, 0.5) == 0
    assert words[8:11].tolist() == [7, 9, 3] and img[16 + 16 + 12: 16 + 32].tobytes() == struct.pack("<f", 2.0)
    assert lib.wipa_sample_rows_fill_row(img.ctypes.data, n, B, 1, 7, 9, 3, 0.0) == 0
    assert img[16 + 16 + 12: 16 + 32].tobytes() == struct.pack("<f", 0.0)
    assert words[4:8].tolist() == [0, 0, 0, 0] and words[12:16].tolist() == [2, 0, 0, 0]  # the neighbours are untouched


def test_rows_record_refuses_by_the_arguments_name(lib):
    """a negative or non-finite temperature, an attempt of 65536 and a slot of B: by name, on the host image and -- before any launch, the
    device pointer is never dereferenced -- in wipa_sample_rows_set"""
    B = 4
    n = lib.wipa_sample_rows_bytes(B)
    img = np.zeros(n, dtype=np.uint8)
    lib.wipa_sample_rows_fill(img.ctypes.data, n, 1, B)
    before = img.copy()
    fake = C.c_void_p(0x1000)

    def set_one(slot, attempt, temperature):
        return lib.wipa_sample_rows_set(fake, B, 2, (C.c_int32 * 2)(0, slot), (C.c_uint32 * 4)(0, 0, 1, 0), (C.c_int32 * 2)(0, attempt),
                                        (C.c_float * 2)(0.0, temperature), None)

    for slot, attempt, temperature, name in ((1, 0, -0.2, b"temperature"), (1, 0, float("nan"), b"temperature"), (1, 0, float("inf"), b"temperature"),
                                             (1, 65536, 0.2, b"attempt"), (1, -1, 0.2, b"attempt"), (B, 0, 0.2, b"slot"), (-1, 0, 0.2, b"slot")):
        assert lib.wipa_sample_rows_fill_row(img.ctypes.data, n, B, slot, 0, 0, attempt, temperature) != 0
        assert name in lib.wipa_last_error(), (name, lib.wipa_last_error())
        assert set_one(slot, attempt, temperature) != 0
        assert name in lib.wipa_last_error() and b"wipa_sample_rows_set" in lib.wipa_last_error(), (name, lib.wipa_last_error())
    assert (img == before).all()
    assert lib.wipa_sample_rows_set(None, B, 0, None, None, None, None, None) != 0 and b"rows_dev" in lib.wipa_last_error()
    assert lib.wipa_sample_rows_set(fake, B, 0, None, None, None, None, None) == 0  # no rows: nothing to write, nothing launched


# ---------------------------------------------------------------- the C ABI
def test_abi_has_the_entry_points(lib):
    from whisper_ipa_amd import _lib

    assert "sample_rows" in {f for f, _ in _lib.DecodeCall._fields_}
    for name in ("wipa_decoder_run_ex", "wipa_sample_rows_bytes", "wipa_sample_rows_fill", "wipa_sample_rows_fill_row",
                 "wipa_sample_rows_set"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_run_continuous_rows_refuses_by_name_before_any_launch(lib):
    """With a temperature per row: a record beside the single-temperature one, an unaligned record, fp8 tables, candidate groups, a missing
    starts array, a wrong count of initial tokens and a bad no-speech column are refused with a message that names the entry point and the
    field; rules may be NULL; the pointers are never dereferenced"""
    from decode_call_util import FAKE, fp8_cfg, refusal, small_cfg
    from whisper_ipa_amd import _lib

    cfg = small_cfg(_lib)
    for r in (True, False):
        on = dict(rules=r, continuous=1, starts_dev=FAKE, sample_rows=FAKE)
        assert "call.continuous needs call.starts_dev" in refusal(_lib, "run", cfg, **{**on, "starts_dev": None})
        assert "fp8" in refusal(_lib, "run", fp8_cfg(_lib), **on)
        assert "candidate groups" in refusal(_lib, "run", small_cfg(_lib, dec_n_group=2), **on)
        assert "initial tokens" in refusal(_lib, "run", cfg, **{**on, "n_init": 5})
        assert "call.sample_rows takes the place of call.sample" in refusal(_lib, "run", cfg, **{**on, "sample": FAKE})
    on = dict(rules=True, continuous=1, starts_dev=FAKE, sample_rows=FAKE)
    assert "call.no_speech_token=51865" in refusal(_lib, "run", cfg, **on, no_speech_dev=FAKE, no_speech_token=51865)
    assert "call.no_speech_dev needs call.rules" in refusal(_lib, "run", cfg, **{**on, "rules": False}, no_speech_dev=FAKE)
    msg = refusal(_lib, "run", cfg, **{**on, "sample_rows": 0x1004})
    assert "call.sample_rows" in msg and "16-byte aligned" in msg
