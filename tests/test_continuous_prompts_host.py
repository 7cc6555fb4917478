"""CPU: prompts on the continuous schedule.  The scheduler with a prompt room (``run_schedule`` / ``run_stream`` with ``prompt_room = R``)
against a fake stepper that keeps a token table with every clip's prompt IN FRONT of its admission column; ``transcribe``'s window
source with conditioning -- the prompt a window is handed out with, its budget, its reset and its retry -- against the rounds loop
with a scripted ``decode_fn``; what stays refused; the new symbols of the C ABI and their refusals by name.  No GPU."""
import ctypes as C
import warnings
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from test_continuous_host import EOT, N_CTX, N_INIT, FakeStepper, _expected, _text
from test_continuous_rules_host import _Tok

PROMPT = 7000  # prompt column j of clip i holds PROMPT + 10 * i + (j % 10)


class PromptedStepper:
    """slots x N_CTX token table that starts at column R.  Clip i's prompt of ``prompt_lens[i]`` columns goes in front of its admission
    column, its text token at its k-th generated column is 100 * (i + 1) + k and it says EOT after ``ends[i]`` text tokens or at its
    limit.  Asserts what the device relies on: no prompt column below 0, no admission and no shift below R."""

    def __init__(self, slots, ends, limits, prompt_lens, room):
        self.slots, self.ends, self.limits, self.prompt_lens, self.room = slots, ends, limits, prompt_lens, room
        self.tokens = np.full((slots, N_CTX), EOT, dtype=np.int64)
        self.start = [0] * slots   # window starts
        self.own = [0] * slots     # first generated column
        self.clip = [None] * slots
        self.pos = room
        self.out, self.log = {}, []

    def admit(self, pairs):
        self.log.append(("admit", list(pairs), self.pos))
        assert self.pos >= self.room
        for slot, clip in pairs:
            L = self.prompt_lens[clip]
            assert self.pos - L >= 0 and self.pos + N_INIT < N_CTX
            self.clip[slot], self.start[slot], self.own[slot] = clip, self.pos - L, self.pos + N_INIT
            self.tokens[slot, self.pos - L:self.pos] = [PROMPT + 10 * clip + j % 10 for j in range(L)]
            self.tokens[slot, self.pos:self.pos + N_INIT] = [1, 2, 3, 4]

    def run(self, n):
        for _ in range(n):
            p = self.pos
            assert p + 1 < N_CTX, "a step past the table"
            for slot in range(self.slots):
                clip = self.clip[slot]
                if clip is None or p + 1 < self.own[slot]:
                    continue
                k = p + 1 - self.own[slot]
                if self.tokens[slot, p] == EOT or k >= self.limits[clip] or (self.ends[clip] is not None and k >= self.ends[clip]):
                    self.tokens[slot, p + 1] = EOT
                else:
                    self.tokens[slot, p + 1] = 100 * (clip + 1) + k
            self.pos += 1

    def last_tokens(self):
        return self.tokens[:, self.pos].copy()

    def retire(self, slot, clip, first_column, n_columns):
        assert self.clip[slot] == clip and first_column == self.own[slot]
        L = self.prompt_lens[clip]  # the prompt is still in front of the sot sequence, whatever was shifted
        assert self.tokens[slot, self.start[slot]:self.start[slot] + L].tolist() == [PROMPT + 10 * clip + j % 10 for j in range(L)]
        self.out[clip] = self.tokens[slot, first_column:first_column + n_columns].tolist()
        self.clip[slot] = None
        self.log.append(("retire", clip, self.pos))

    def shift(self, shift):
        live = [s for s in range(self.slots) if self.clip[s] is not None]
        assert 0 < shift <= self.pos - self.room, "a shift below the prompt room"
        assert all(self.start[s] - shift >= 0 for s in live), "a live window start below column 0"
        n = self.pos + 1 - shift
        self.tokens[:, :n] = self.tokens[:, shift:shift + n].copy()
        self.pos -= shift
        self.start = [s - shift for s in self.start]
        self.own = [s - shift for s in self.own]
        self.log.append(("shift", shift, self.pos))


LIMITS = [5, 27, 12, 19, 1, 22, 23, 26]
PROMPTS = [7, 30, 0, 2, 30, 17, 7, 0]
ROOM = 30


def _run(column_limit, room=ROOM, slots=3, prompt_lens=PROMPTS, limits=LIMITS):
    from whisper_ipa_amd.continuous import run_schedule

    st = PromptedStepper(slots, [None] * len(limits), limits, prompt_lens, room)
    stats = run_schedule(st, len(limits), slots, N_INIT, limits, EOT, N_CTX, 4, column_limit, prompt_lens=prompt_lens, prompt_room=room)
    return st, stats


def test_admissions_and_shifts_stay_above_the_prompt_room_and_change_no_result():
    """8 clips with prompts of 0 .. 30 columns through 3 slots, R = 30: no admission below column R, every shift leaves the position at
    or above R and every live window start at or above 0 (the fake asserts both), and the results equal the run without shifts"""
    plain, ps = _run(None)
    assert ps.shifts == [] and all(col >= ROOM for _, _, col in ps.admissions) and ps.admissions[0][2] == ROOM
    for i in range(8):
        assert _text(plain.out[i]) == _text(_expected(i, None, LIMITS[i]))
    need = ROOM + N_INIT + max(LIMITS) + 2 * 4 - 1  # 68
    for limit in (need, need + 6):
        shifted, ss = _run(limit)
        assert ss.shifts and all(x > 0 for x in ss.shifts)
        assert shifted.out == plain.out
        assert ss.steps == ps.steps and [a[:2] for a in ss.admissions] == [a[:2] for a in ps.admissions]
        assert all(ROOM <= col <= limit for _, _, col in ss.admissions)
        positions = [e[2] for e in shifted.log if e[0] == "shift"]
        assert positions and all(p >= ROOM for p in positions)


def test_the_shift_is_the_smaller_of_window_start_and_distance_to_the_room():
    """one slot, R = 10, column_limit = 29: the second clip is admitted at column 18 and is live at column 26, where the next interval
    would pass the limit; its window starts at 18 but the position may fall by 16 only"""
    st, stats = _run(29, room=10, slots=1, prompt_lens=[0, 0], limits=[3, 8])
    assert stats.admissions == [(0, 0, 10), (0, 1, 18)] and stats.shifts == [16]
    assert [e for e in st.log if e[0] == "shift"] == [("shift", 16, 10)]
    assert st.out == {0: [100, 101, 102], 1: [200 + k for k in range(8)]}


def test_span_bound_names_column_limit():
    from whisper_ipa_amd.continuous import run_schedule, run_stream

    st = PromptedStepper(3, [None] * 8, LIMITS, PROMPTS, ROOM)
    with pytest.raises(ValueError, match="column_limit"):
        run_schedule(st, 8, 3, N_INIT, LIMITS, EOT, N_CTX, 4, ROOM + N_INIT + max(LIMITS) + 2 * 4 - 2, prompt_lens=PROMPTS, prompt_room=ROOM)
    assert st.log == []

    class Source:
        def __init__(self):
            self.given = False

        def pending(self):
            if self.given:
                return []
            self.given = True
            return [((0, 0), 27, None, [1] * 5)]

        def retired(self, *a):
            raise AssertionError("nothing runs")

    stepper = SimpleNamespace(admit=lambda group: (_ for _ in ()).throw(AssertionError("admitted")))
    with pytest.raises(ValueError, match="column_limit"):  # per clip, at its admission: 30 + 4 + 27 + 7 = 68 > 67
        run_stream(stepper, Source(), 2, N_INIT, EOT, N_CTX, 4, column_limit=67, prompt_room=ROOM)
    with pytest.raises(ValueError, match="prompt_room"):   # a prompt that does not fit the room
        st = PromptedStepper(1, [None], [3], [ROOM + 1], ROOM)
        run_schedule(st, 1, 1, N_INIT, [3], EOT, N_CTX, 4, None, prompt_lens=[ROOM + 1], prompt_room=ROOM)


def test_room_zero_is_the_existing_loop():
    """R = 0 with empty prompts reproduces the stats and the calls of the loop without prompts on the existing fake"""
    from whisper_ipa_amd.continuous import run_schedule

    ends = [None, 11, None, 4, None, None, 2, None]
    for column_limit in (None, 40):
        a = FakeStepper(3, ends, LIMITS)
        sa = run_schedule(a, 8, 3, N_INIT, LIMITS, EOT, N_CTX, 4, column_limit)
        b = FakeStepper(3, ends, LIMITS)
        sb = run_schedule(b, 8, 3, N_INIT, LIMITS, EOT, N_CTX, 4, column_limit, prompt_lens=[0] * 8, prompt_room=0)
        assert sa == sb and a.log == b.log and a.out == b.out
    assert sa.shifts  # column_limit = 40 did shift


# ---------------------------------------------------------------- transcribe: the window source with conditioning
T = 50364
SOT_PREV = 50361


class _PTok(_Tok):
    sot_prev, sot_sequence = SOT_PREV, (50258, 50259, 50359)

    def encode(self, text):
        return [1000 + (ord(ch) - ord("a")) % 26 for ch in text if ch != " "]


def _files():
    """three files of 95, 5 and 40 s; sample s * 16000 of file f holds 1000 * f + s"""
    out = []
    for f, secs in enumerate((95, 5, 40)):
        x = np.zeros(secs * 16000, dtype=np.float32)
        x[::16000] = 1000.0 * f + np.arange(secs, dtype=np.float32)
        out.append(x)
    return out


def _scripted(first_sample, attempt):
    """a window's result from its first sample and the attempt: seven tokens ending in a single timestamp (the window is consumed).  The
    second window of file 0 (k = 30) fails until its fourth attempt, temperature 0.6: its booking resets the prompt"""
    k = int(round(first_sample))
    toks = [T, 1000 + k % 26, 1001 + k % 26, 1002 + k % 26, 1003 + attempt, 1004, T + 500]
    failing = k == 30 and attempt < 3
    return toks, (-20.0 if failing else -1.0), 0.1


TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def _both(**kw):
    """transcribe on both schedules with scripted decodes; returns (rounds, continuous, the prompts each schedule gave per (file, seek,
    attempt), the continuous run's stats)"""
    from whisper_ipa_amd.transcribe import transcribe

    tok = _PTok()
    given_rounds, given_cont = {}, {}
    frames = {}

    def result(first, attempt, language):
        tokens, slp, nsp = _scripted(first, attempt)
        text = tok.decode([t for t in tokens if t < T]).strip()
        comp = len(text.encode()) / max(len(zlib.compress(text.encode())), 1)
        return SimpleNamespace(tokens=tokens, avg_logprob=slp / (len(tokens) + 1), no_speech_prob=nsp, compression_ratio=comp,
                               temperature=TEMPS[attempt], language=language or "en", first=first)

    def decode_fn(windows, languages, prompts=None):
        for w, p in zip(windows, prompts):
            given_rounds[(int(round(w[0])), 0)] = list(p)
        return [result(w[0], 0, lang) for w, lang in zip(windows, languages)]

    def fallback_fn(results, languages, *, temperature, attempt, streams, seed, prompts=None):
        for r, p in zip(results, prompts):
            given_rounds[(int(round(r.first)), attempt)] = list(p)
        return [result(r.first, attempt, lang) for r, lang in zip(results, languages)]

    def stream_fn(source, slots, check_every, prompt_room=None):
        frames["room"] = prompt_room
        first, live = {}, []
        while True:
            new = source.pending()
            assert all(len(e) == 4 for e in new)  # with conditioning: (clip, limit, draw, prompt)
            fresh = [clip for clip, _, draw, _ in new if draw is None]
            if fresh:
                windows, languages = source.group(fresh)
                for clip, w in zip(fresh, windows):
                    first[clip] = w[0]
            for clip, _, draw, prompt in new:
                assert len(prompt) <= prompt_room and (not prompt or prompt[0] == SOT_PREV)
                given_cont[(int(round(first[clip])), draw[1] if draw else 0)] = list(prompt[1:])
                live.append((clip, draw))
            if not live:
                return "stats"
            clip, draw = live.pop(0)
            source.retired(clip, *_scripted(first[clip], draw[1] if draw else 0))

    stream_fn.retries = stream_fn.prompts = True
    stats = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rounds = transcribe(None, _files(), decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=tok, language="en", seed=5, **kw)
        cont = transcribe(None, _files(), schedule="continuous", slots=2, stream_fn=stream_fn, tokenizer=tok, language="en", seed=5,
                          stats_out=stats, **kw)
    return rounds, cont, given_rounds, given_cont, stats[0], frames["room"]


def test_window_source_hands_out_the_prompt_the_rounds_loop_builds():
    """condition_on_previous_text with an initial prompt: window k's prompt is the initial prompt plus the booked tokens of the windows
    before it, reset after the window booked at temperature 0.6, and every retry carries the prompt of its first attempt"""
    rounds, cont, given_rounds, given_cont, st, room = _both(condition_on_previous_text=True, initial_prompt="abc", sample_len=20)
    assert cont == rounds
    assert given_cont == given_rounds and len(given_cont) == 4 + 3 + 1 + 2  # file 0: 4 windows + 3 retries; file 1: 1; file 2: 2
    initial = [1000, 1001, 1002]
    w0 = _scripted(0, 0)[0]
    assert given_cont[(0, 0)] == initial and given_cont[(30, 0)] == initial + w0
    for attempt in (1, 2, 3):
        assert given_cont[(30, attempt)] == given_cont[(30, 0)]  # the retry carries the same prompt
    assert [s["temperature"] for s in cont[0]["segments"]] == [0.0, 0.6, 0.0, 0.0]
    assert given_cont[(60, 0)] == []  # booked above 0.5: the prompt is reset
    assert given_cont[(90, 0)] == _scripted(60, 0)[0]
    assert given_cont[(2030, 0)] == initial + _scripted(2000, 0)[0]
    assert st.prompt_budget == 223 and room == 224  # sample_len 20 leaves upstream's budget
    assert sorted((f, at, kept) for f, at, _, kept in st.prompts) == sorted(
        [(0, 0, 3), (0, 3000, 10), (0, 3000, 10), (0, 3000, 10), (0, 3000, 10), (0, 6000, 0), (0, 9000, 7), (1, 0, 3), (2, 0, 3), (2, 3000, 10)])


def test_prompt_budget_cuts_the_history_on_both_schedules():
    rounds, cont, given_rounds, given_cont, st, room = _both(condition_on_previous_text=True, initial_prompt="abc", sample_len=20,
                                                             prompt_budget=5)
    assert cont == rounds and given_cont == given_rounds
    assert given_cont[(30, 0)] == ([1000, 1001, 1002] + _scripted(0, 0)[0])[-5:] and all(len(p) <= 5 for p in given_cont.values())
    assert st.prompt_budget == 5 and room == 6
    assert any(kept < history for _, _, history, kept in st.prompts)
    # an initial prompt alone (no conditioning): the first window of every file carries it, nothing else does
    rounds, cont, given_rounds, given_cont, st, _ = _both(initial_prompt="abc", sample_len=20)
    assert cont == rounds and given_cont == given_rounds
    assert given_cont[(0, 0)] == [1000, 1001, 1002] and given_cont[(30, 0)] == [] and given_cont[(2030, 0)] == []


def test_the_default_budget_is_what_the_column_window_leaves():
    from whisper_ipa_amd.transcribe import continuous_prompt_budget, transcribe

    assert continuous_prompt_budget(448, 3, 224, 8) == 196  # against upstream's 223
    assert continuous_prompt_budget(448, 3, 197, 8) == 223 and continuous_prompt_budget(448, 3, 198, 8) == 222
    assert continuous_prompt_budget(448, 3, 20, 8) == 223

    def never(source, slots, check_every, prompt_room=None):
        raise AssertionError("something was decoded")

    never.prompts = True
    with pytest.raises(ValueError, match="prompt_budget"):  # more than fits
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_PTok(), language="en",
                   condition_on_previous_text=True, prompt_budget=197)
    with pytest.raises(ValueError, match="prompt_budget"):  # without conditioning
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_PTok(), language="en",
                   prompt_budget=5)


@pytest.mark.parametrize("kw,name", [(dict(condition_on_previous_text=True), "condition_on_previous_text"),
                                     (dict(initial_prompt="hello"), "initial_prompt")])
def test_a_stream_fn_that_does_not_declare_prompts_is_refused_by_name(kw, name):
    from whisper_ipa_amd.transcribe import continuous_prompt_budget, transcribe

    def never(source, slots, check_every):
        raise AssertionError("something was decoded")

    never.retries = True
    with pytest.raises(NotImplementedError, match=name):
        transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=never, tokenizer=_PTok(), **kw)
    # the same call with a stream_fn that declares prompts reaches it, with the prompt room
    called = []

    def stream_fn(source, slots, check_every, prompt_room=None):
        called.append(prompt_room)

    stream_fn.prompts = True
    transcribe(None, np.zeros(16000, dtype=np.float32), schedule="continuous", stream_fn=stream_fn, tokenizer=_PTok(), language="en", **kw)
    assert called == [continuous_prompt_budget(448, 3, 224, 8) + 1] == [197]


def test_decode_continuous_refuses_by_name():
    from whisper_ipa_amd.continuous import decode_continuous, refuse_unserved
    from whisper_ipa_amd.decoding import DecodingOptions

    import torch

    model = SimpleNamespace(_fp8=None)
    x = torch.zeros(2, 1500, 8)
    with pytest.raises(NotImplementedError, match="prompts with best_of"):
        decode_continuous(model, x, DecodingOptions(without_timestamps=True, best_of=3, temperature=0.5, seed=1), prompts=[[], [1]])
    with pytest.raises(NotImplementedError, match="prompts on an fp8"):
        decode_continuous(SimpleNamespace(_fp8={"x": 1}), x, DecodingOptions(without_timestamps=True), prompts=[[], [1]])
    with pytest.raises(ValueError, match="prompt_room comes with prompts"):
        decode_continuous(model, x, DecodingOptions(without_timestamps=True), prompt_room=5)
    for name in ("prompt", "prefix", "prompts"):  # the options stay refused: the keyword is decode_continuous's own
        with pytest.raises(NotImplementedError, match=name):
            refuse_unserved(model, DecodingOptions(without_timestamps=True, **{name: [1, 2]}))


# ---------------------------------------------------------------- the C ABI
NEW = ("wipa_decoder_seek", "wipa_decoder_admit_prompted_workspace_bytes", "wipa_decoder_admit_rows_prompted", "wipa_decoder_run_ex")


def _lib_and_cfg():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    small = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865, n_text_ctx=448, n_text_state=384,
                 n_text_head=6, n_text_layer=2, dtype=_lib.WIPA_BF16, dec_cross_absorbed=1)
    return _lib, _lib.lib(), small


def test_abi_has_the_new_entry_points():
    _lib, lib, small = _lib_and_cfg()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "prompted" in {f for f, _ in _lib.DecodeCall._fields_}
    cfg = _lib.ModelCfg(**small)
    size = lib.wipa_decoder_admit_prompted_workspace_bytes
    assert size(C.byref(cfg), 0, 4) == 0 and size(C.byref(cfg), 2, -1) == 0
    assert 0 < size(C.byref(cfg), 2, 0) < size(C.byref(cfg), 2, 32) < size(C.byref(cfg), 2, 197) < size(C.byref(cfg), 16, 197)


def test_new_entry_points_refuse_by_name_before_any_launch():
    """the pointers are never dereferenced: every refusal comes before anything is enqueued"""
    _lib, lib, small = _lib_and_cfg()
    cfg = _lib.ModelCfg(**small)
    fp8 = _lib.ModelCfg(**{**small, "dec_cross_absorbed": 0, "dec_w_dtype": _lib.WIPA_FP8_E4M3})
    grouped = _lib.ModelCfg(**{**small, "dec_n_group": 2})
    fake = C.c_void_p(0x1000)
    tab = (C.c_void_p * 64)()
    rules = _lib.DecodeRules(50364, 50363, 50)
    err = lib.wipa_last_error

    seek = lib.wipa_decoder_seek
    for column in (-1, 447, 448):
        assert seek(C.byref(cfg), fake, 1 << 40, 4, column, None) != 0 and b"column" in err()
    assert seek(C.byref(cfg), fake, 16, 4, 5, None) != 0  # a state blob that is too small

    from decode_call_util import FAKE, refusal

    on = dict(rules=True, continuous=1, prompted=1, starts_dev=FAKE, no_speech_dev=FAKE, no_speech_token=50362)
    msg = refusal(_lib, "run", cfg, **{**on, "starts_dev": None})
    assert "call.continuous needs call.starts_dev" in msg and "[3][B] with call.prompted" in msg
    assert "call.sample_rows takes the place of call.sample" in refusal(_lib, "run", cfg, **on, sample=FAKE, sample_rows=FAKE)
    assert "call.sample_rows" in refusal(_lib, "run", cfg, **on, sample_rows=0x1008) and b"16-byte aligned" in err()
    assert "call.no_speech_dev needs call.rules" in refusal(_lib, "run", cfg, **{**on, "rules": False})
    assert "call.no_speech_token=51865" in refusal(_lib, "run", cfg, **{**on, "no_speech_token": 51865})
    assert "fp8" in refusal(_lib, "run", fp8, **on)
    assert "candidate groups" in refusal(_lib, "run", grouped, **on)
    assert "initial tokens" in refusal(_lib, "run", cfg, **{**on, "no_speech_dev": None, "n_init": 5})
    assert "call.prompted" in refusal(_lib, "run", cfg, **{**on, "continuous": 0}) and b"need call.continuous" in err()

    admit = lib.wipa_decoder_admit_rows_prompted
    slots = (C.c_int32 * 2)(0, 1)
    feats = (C.c_void_p * 2)(0x1000, 0x1000)
    init = (C.c_int32 * 6)(50258, 50259, 50359, 50258, 50259, 50359)
    lim = (C.c_int32 * 2)(5, 5)
    lens = (C.c_int32 * 2)(2, 0)
    ptok = (C.c_int32 * 4)(50361, 1000, 0, 0)  # [n_rows][W], right-aligned: row 0 holds two columns, row 1 none

    def call(cfg_=cfg, slots_=slots, init_=init, lens_=lens, ptok_=ptok, W=2, starts=fake, ws=fake, ws_bytes=1 << 40, n_init=3):
        return admit(C.byref(cfg_), tab, fake, 1 << 40, 4, 2, slots_, feats, init_, n_init, lim, lens_, ptok_, W, starts, None, None, ws, ws_bytes,
                     None)

    assert call(starts=None) != 0 and b"starts_dev (int32 [3][B]" in err()
    assert call(cfg_=fp8) != 0 and b"fp8" in err()
    assert call(slots_=(C.c_int32 * 2)(0, 4)) != 0 and b"slot" in err()          # what wipa_decoder_admit_rows refuses
    assert call(slots_=(C.c_int32 * 2)(1, 1)) != 0 and b"listed twice" in err()
    assert call(init_=(C.c_int32 * 6)(50258, 50259, 51865, 0, 0, 0)) != 0 and b"initial token" in err()
    assert call(n_init=5) != 0 and b"initial tokens" in err()
    assert call(lens_=(C.c_int32 * 2)(-1, 0)) != 0 and b"prompt length" in err()
    assert call(lens_=(C.c_int32 * 2)(445, 0), W=444) != 0 and b"prompt length" in err()   # L outside 0 .. n_text_ctx - n_init - 1 = 444
    assert call(W=445) != 0 and b"prompt width" in err()
    assert call(lens_=(C.c_int32 * 2)(3, 0)) != 0 and b"exceeds the width" in err()
    assert call(ptok_=(C.c_int32 * 4)(50361, 51865, 0, 0)) != 0 and b"prompt token" in err()
    assert call(ptok_=(C.c_int32 * 4)(50361, 1000, -7, 99999), ws_bytes=16) != 0 and b"workspace too small" in err()  # padding is not looked at
    assert call(ws=None) != 0 and b"workspace too small" in err()
