"""CPU: the scheduler of the continuous-batching decode (whisper_ipa_amd.continuous.run_schedule) against a fake stepper -- a Python
object that keeps a token table and advances every slot by one column per step, each clip producing its prescribed number of text
tokens and then EOT, or EOT at its limit, as the CONTINUOUS tails do on the device.  Admission order, results in input order when
clips finish out of order, the shift amounts and their positivity, queues shorter than the slots, the refusals by name, and the three
new symbols of the C ABI.  No GPU."""
import numpy as np
import pytest

N_INIT, EOT, N_CTX = 4, 9, 128


class FakeStepper:
    """slots x N_CTX token table; clip i's text token at its k-th generated column is 100 * (i + 1) + k, and it says EOT after
    ``ends[i]`` text tokens (None: never) or at its limit"""

    def __init__(self, slots, ends, limits):
        self.slots, self.ends, self.limits = slots, ends, limits
        self.tokens = np.full((slots, N_CTX), EOT, dtype=np.int64)
        self.start = [0] * slots
        self.clip = [None] * slots
        self.pos = 0
        self.out = {}
        self.log = []

    def admit(self, pairs):
        self.log.append(("admit", list(pairs), self.pos))
        for slot, clip in pairs:
            assert self.pos + N_INIT < N_CTX
            self.clip[slot], self.start[slot] = clip, self.pos
            self.tokens[slot, self.pos:self.pos + N_INIT] = [1, 2, 3, 4]

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
                    continue  # prompt
                k = p + 1 - own
                if self.tokens[slot, p] == EOT or k >= self.limits[clip] or (self.ends[clip] is not None and k >= self.ends[clip]):
                    self.tokens[slot, p + 1] = EOT
                else:
                    self.tokens[slot, p + 1] = 100 * (clip + 1) + k
            self.pos += 1

    def last_tokens(self):
        return self.tokens[:, self.pos].copy()

    def retire(self, slot, clip, first_column, n_columns):
        assert self.clip[slot] == clip and first_column == self.start[slot] + N_INIT
        self.out[clip] = self.tokens[slot, first_column:first_column + n_columns].tolist()
        self.log.append(("retire", clip, self.pos))

    def shift(self, shift):
        assert 0 < shift <= self.pos
        n = self.pos + 1 - shift
        self.tokens[:, :n] = self.tokens[:, shift:shift + n].copy()
        self.pos -= shift
        self.start = [max(s - shift, 0) for s in self.start]
        self.log.append(("shift", shift, self.pos))


def _expected(clip, end, limit):
    n = limit if end is None else min(end, limit)
    row = [100 * (clip + 1) + k for k in range(n)]
    return row + [EOT] * (limit - n) if end is not None and end < limit else row


def _run(ends, limits, slots, check_every=4, column_limit=None):
    from whisper_ipa_amd.continuous import run_schedule

    st = FakeStepper(slots, ends, limits)
    stats = run_schedule(st, len(limits), slots, N_INIT, limits, EOT, N_CTX, check_every, column_limit)
    return st, stats


def _text(row):
    return row[: row.index(EOT)] if EOT in row else row


def test_admission_order_and_results_in_input_order():
    """8 clips through 3 slots; clips finish out of order (lengths 5, 17, 2, 9, 1, 12, 3, 6, some by EOT and some by their limit)"""
    limits = [5, 17, 2, 9, 1, 12, 3, 6]
    ends = [None, 11, None, 4, None, None, 2, None]
    st, stats = _run(ends, limits, slots=3)
    assert [clip for _, clip, _ in stats.admissions] == list(range(8))  # input order
    assert [slot for slot, _, _ in stats.admissions[:3]] == [0, 1, 2] and all(col == 0 for _, _, col in stats.admissions[:3])
    assert stats.retired != sorted(stats.retired)  # they did finish out of order
    assert sorted(st.out) == list(range(8))
    for i in range(8):
        want = _text(_expected(i, ends[i], limits[i]))
        assert _text(st.out[i]) == want, (i, st.out[i], want)
        assert len(st.out[i]) <= limits[i]
    # a freed slot takes the next pending clip at the column of the check that freed it
    for slot, clip, col in stats.admissions[3:]:
        assert col % 4 == 0 and col > 0
    # every retirement precedes the admission that reuses its slot's columns
    order = [e[0] for e in st.log]
    assert order[0] == "admit" and "retire" in order


def test_forced_shifts_amounts_and_same_results():
    """lengths under which column_limit = 40 forces two shifts (the whole run of the shorter list above takes 32 steps and never
    reaches column 40): the amounts are the smallest start among the live rows, 20 and then 12, and nothing else changes"""
    limits = [5, 27, 12, 19, 1, 22, 23, 26]
    ends = [None] * 8
    plain, ps = _run(ends, limits, slots=3, column_limit=None)
    assert ps.shifts == []
    shifted, ss = _run(ends, limits, slots=3, column_limit=40)
    assert ss.shifts == [20, 12]
    assert shifted.out == plain.out
    assert ss.steps == ps.steps and [a[:2] for a in ss.admissions] == [a[:2] for a in ps.admissions]
    shifts = [e for e in shifted.log if e[0] == "shift"]
    assert [e[1] for e in shifts] == ss.shifts
    assert all(0 <= col <= 40 for _, _, col in ss.admissions)
    # the smallest limit the scheduler takes for these lengths: n_init + longest + 2 * check_every - 1 = 38
    tight, ts = _run(ends, limits, slots=3, column_limit=38)
    assert tight.out == plain.out and len(ts.shifts) >= 2 and all(x > 0 for x in ts.shifts)


def test_column_limit_too_small_is_refused_before_any_step():
    from whisper_ipa_amd.continuous import run_schedule

    st = FakeStepper(3, [None] * 3, [5, 17, 2])
    with pytest.raises(ValueError, match="column_limit"):
        run_schedule(st, 3, 3, N_INIT, [5, 17, 2], EOT, N_CTX, 4, 27)
    with pytest.raises(ValueError, match="column_limit"):
        run_schedule(st, 3, 3, N_INIT, [5, 17, 2], EOT, N_CTX, 4, N_CTX - N_INIT)
    assert st.log == []


def test_shift_positivity_assertion():
    """rows that outlive what the scheduler sized its window by (limits that iterate as 1 but index as 10**6, on a stepper that never
    says EOT): the oldest live row reaches the limit with its start at column 0, and the scheduler asserts instead of shifting by 0"""
    from whisper_ipa_amd.continuous import run_schedule

    class Stuck(FakeStepper):
        def last_tokens(self):
            return np.full(self.slots, 7)

    class Lying(list):
        def __getitem__(self, i):
            return 10 ** 6

    st = Stuck(2, [None, None], [50, 50])
    with pytest.raises(AssertionError, match="shift would be 0"):
        run_schedule(st, 2, 2, N_INIT, Lying([1, 1]), EOT, N_CTX, 4, 20)
    assert st.pos == 20 and not any(e[0] == "shift" for e in st.log)


def test_queue_shorter_than_slots_and_empty_queue():
    st, stats = _run([None, 3], [6, 6], slots=5)
    assert [a[:2] for a in stats.admissions] == [(0, 0), (1, 1)]
    assert _text(st.out[0]) == [100 + k for k in range(6)] and _text(st.out[1]) == [200, 201, 202]
    assert stats.steps == 12  # 3 prompt steps + 6 tokens = 9 -> three checks of 4
    st, stats = _run([], [], slots=4)
    assert stats.steps == 0 and stats.admissions == [] and st.log == [] and st.out == {}


def test_step_counts_and_the_bound_from_the_lengths():
    from whisper_ipa_amd.continuous import continuous_steps_bound, lockstep_steps

    limits = [5, 17, 2, 9, 1, 12, 3, 6]
    _, stats = _run([None] * 8, limits, slots=3)
    assert lockstep_steps(limits, 3) == 17 + 12 + 6
    bound = continuous_steps_bound(limits, 3, N_INIT, 4)
    assert bound == max(-(-(sum(limits) + 8 * 3) // 3), 17 + 3)
    assert stats.steps >= bound
    assert lockstep_steps([], 4) == 0 and continuous_steps_bound([], 4, N_INIT, 8) == 0


class BothStepper:
    """a scripted stepper that serves both schedulers: slots x n_ctx token table, n_init = 3; clip i's k-th generated token is
    100 * (i + 1) + k, and it says EOT after ``lengths[i]`` tokens or at its limit.  ``admit`` takes ``run_schedule``'s pairs (the limit is
    ``limits[clip]``) and ``run_stream``'s triples; ``last_tokens`` / ``retire`` and ``snapshot`` read the same table."""

    N_INIT = 3

    def __init__(self, slots, lengths, limits, n_ctx):
        self.slots, self.lengths, self.limits, self.n_ctx = slots, lengths, limits, n_ctx
        self.tokens = np.full((slots, n_ctx), EOT, dtype=np.int64)
        self.start, self.clip, self.limit = [0] * slots, [None] * slots, [0] * slots
        self.pos = 0
        self.rows = {}

    def admit(self, entries):
        for slot, clip, *limit in entries:
            assert self.pos + self.N_INIT < self.n_ctx
            self.clip[slot], self.start[slot], self.limit[slot] = clip, self.pos, limit[0] if limit else self.limits[clip]
            self.tokens[slot, self.pos:self.pos + self.N_INIT] = [1, 2, 3]

    def run(self, n):
        for _ in range(n):
            p = self.pos
            assert p + 1 < self.n_ctx, "a step past the table"
            for slot, clip in enumerate(self.clip):
                own = self.start[slot] + self.N_INIT
                if clip is None or p + 1 < own:
                    continue
                k = p + 1 - own
                done = self.tokens[slot, p] == EOT or k >= self.limit[slot] or k >= self.lengths[clip]
                self.tokens[slot, p + 1] = EOT if done else 100 * (clip + 1) + k
            self.pos += 1

    def shift(self, shift):
        assert 0 < shift <= self.pos
        n = self.pos + 1 - shift
        self.tokens[:, :n] = self.tokens[:, shift:shift + n].copy()
        self.pos -= shift
        self.start = [max(s - shift, 0) for s in self.start]

    def last_tokens(self):
        return self.tokens[:, self.pos].copy()

    def retire(self, slot, clip, first_column, n_columns):
        assert self.clip[slot] == clip and first_column == self.start[slot] + self.N_INIT
        self.rows[clip] = _text(self.tokens[slot, first_column:first_column + n_columns].tolist())

    def snapshot(self):
        return self.tokens[:, : self.pos + 1].copy(), np.zeros(self.slots, dtype=np.float32), np.zeros(self.slots, dtype=np.float32)


def test_both_schedulers_make_the_same_schedule():
    """the same 9 clips through 3 slots of a 48-column table, check_every = 4, n_init = 3: ``run_schedule`` and ``run_stream`` (a source
    whose first ``pending()`` gives every clip) take the same steps, shift by the same amounts, admit the same clips into the same slots at
    the same columns, retire them in the same order and hand out the same token rows.  Clips 1, 5 and 8 never say EOT: they end at their
    limits."""
    from whisper_ipa_amd.continuous import run_schedule, run_stream

    n_ctx, slots, check_every = 48, 3, 4
    limits = [12, 25, 16, 18, 9, 22, 15, 19, 20]
    lengths = [10, 99, 16, 17, 2, 99, 14, 18, 99]  # text tokens before EOT; 99: none within the limit
    a = BothStepper(slots, lengths, limits, n_ctx)
    sa = run_schedule(a, len(limits), slots, BothStepper.N_INIT, limits, EOT, n_ctx, check_every)

    class Source:
        def __init__(self):
            self.clips, self.rows = [(i, n) for i, n in enumerate(limits)], {}

        def pending(self):
            out, self.clips = self.clips, []
            return out

        def retired(self, clip, tokens, sum_logprob, no_speech):
            assert clip not in self.rows
            self.rows[clip] = list(tokens)

    b, src = BothStepper(slots, lengths, limits, n_ctx), Source()
    sb = run_stream(b, src, slots, BothStepper.N_INIT, EOT, n_ctx, check_every)
    assert len(sa.shifts) >= 2 and all(x > 0 for x in sa.shifts)
    assert (sa.steps, sa.shifts, sa.admissions, sa.retired) == (sb.steps, sb.shifts, sb.admissions, sb.retired)
    assert sorted(sa.retired) == list(range(9)) and sa.retired != sorted(sa.retired)
    want = {i: [100 * (i + 1) + k for k in range(min(lengths[i], limits[i]))] for i in range(9)}
    assert a.rows == want and src.rows == want
    assert [len(want[i]) == limits[i] for i in range(9)].count(True) >= 1  # a clip that ended by its limit
    assert (a.tokens == b.tokens).all()


def test_refusals_name_the_option():
    from whisper_ipa_amd.continuous import refuse_unserved
    from whisper_ipa_amd.decoding import DecodingOptions

    class M:
        _fp8 = {}

    ok = DecodingOptions(without_timestamps=True)
    refuse_unserved(M(), ok)
    refuse_unserved(M(), DecodingOptions(without_timestamps=True, temperature=0.6, seed=1))
    for kw, name in ((dict(without_timestamps=False), "without_timestamps=False"), (dict(prompt="a b"), "prompt"), (dict(prefix=[5, 6]), "prefix"),
                     (dict(prompts=[[1]]), "prompts"), (dict(best_of=3, temperature=0.5, seed=1), "best_of"), (dict(beam_size=2), "beam_size"),
                     (dict(temperature=0.5), "seed")):
        with pytest.raises(NotImplementedError, match=name):
            refuse_unserved(M(), DecodingOptions(**{**ok.__dict__, **kw}))

    class F:
        _fp8 = {"x": 1}

    with pytest.raises(NotImplementedError, match="fp8"):
        refuse_unserved(F(), ok)


def test_abi_has_the_three_entry_points():
    import __graft_entry__ as g

    g.build()
    import whisper_ipa_amd
    from whisper_ipa_amd import _lib

    lib = _lib.lib()
    for name in ("wipa_decoder_admit_rows", "wipa_decoder_shift_columns", "wipa_decoder_run_ex"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert callable(whisper_ipa_amd.decode_continuous)


def test_entry_points_refuse_by_name_before_any_launch():
    """fp8 tables, candidate groups and a missing starts array are refused with WIPA_ERR_ARG and a message that names the entry point and
    the field; the pointers are never dereferenced"""
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from decode_call_util import FAKE, fp8_cfg, refusal, small_cfg
    from whisper_ipa_amd import _lib

    lib = _lib.lib()
    small = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865, n_text_ctx=448, n_text_state=384,
                 n_text_head=6, n_text_layer=2, dtype=_lib.WIPA_BF16, dec_cross_absorbed=1)
    cfg = _lib.ModelCfg(**small)
    fake = C.c_void_p(0x1000)
    tab = (C.c_void_p * 64)()
    assert "call.continuous needs call.starts_dev" in refusal(_lib, "run", cfg, continuous=1)
    msg = refusal(_lib, "run", fp8_cfg(_lib), continuous=1, starts_dev=FAKE, n_init=4)
    assert "fp8" in msg and "dec_w_dtype" in msg
    assert "candidate groups" in refusal(_lib, "run", small_cfg(_lib, dec_n_group=2), continuous=1, starts_dev=FAKE)
    assert "call.n_init: 1..4 initial tokens" in refusal(_lib, "run", cfg, continuous=1, starts_dev=FAKE, n_init=5)
    # fields that need a continuous call, one by one
    for field in ("sample_rows", "no_speech_dev"):
        assert f"call.{field}" in refusal(_lib, "run", cfg, rules=True, **{field: FAKE}) and "need call.continuous" in lib.wipa_last_error().decode()
    assert "call.prompted" in refusal(_lib, "run", cfg, prompted=1, starts_dev=FAKE) and "need call.continuous" in lib.wipa_last_error().decode()
    grouped = _lib.ModelCfg(**{**small, "dec_n_group": 2})
    rc = lib.wipa_decoder_shift_columns(C.byref(grouped), fake, 1 << 40, 4, fake, 1, None)
    assert rc != 0 and b"candidate groups" in lib.wipa_last_error()
    rc = lib.wipa_decoder_shift_columns(C.byref(cfg), fake, 1 << 40, 4, fake, 0, None)
    assert rc != 0 and b"shift" in lib.wipa_last_error()
    slots = (C.c_int32 * 1)(7)
    feats = (C.c_void_p * 1)(0x2000)
    init = (C.c_int32 * 4)(1, 2, 3, 4)
    lim = (C.c_int32 * 1)(5)
    rc = lib.wipa_decoder_admit_rows(C.byref(cfg), tab, fake, 1 << 40, 4, 1, slots, feats, init, 4, lim, fake, None, None, None)
    assert rc != 0 and b"slot" in lib.wipa_last_error()
