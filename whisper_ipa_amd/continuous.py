"""Continuous-batching decode: the rows of one decode state are SLOTS, and a slot whose clip has finished takes the next clip while the
other rows go on (include/wipa.h: wipa_decoder_admit_rows / wipa_decoder_shift_columns /
wipa_decode_call.continuous).

``decode`` runs a batch in lockstep: every row steps until the last one has reached EOT, and a row that ended early sits EOT-latched
in its slot, its encoder output still streamed through every cross-attention layer of every step.  Here the host looks at the last
token column every ``check_every`` steps, retires the rows that have finished -- their tokens and log-probability sums are copied out in
stream order -- and admits the next pending clips into the freed slots at the column the state stands at.  Every row has its own first
column (``start``), so its position embeddings, attention window, sampling counter and prompt end are its own; when the shared column
counter nears the end of the table, all columns move down by the smallest start among the live rows (a *shift*), which no row can see.

The scheduler (``run_schedule``) is plain Python against a small stepper interface, so it is tested without a GPU; ``DeviceStepper`` is
the stepper on the library.

With ``without_timestamps=False`` the steps end in the CONTINUOUS tails with the timestamp rules (wipa_decode_call.rules;
DESIGN.md section 14): the rules run on every row's own sequence, from its own first column, and the tail leaves the row's no-speech
probability at its <|startoftranscript|> column.  ``run_stream`` is the scheduler for clips that are not all known when the run starts
-- the windows of files, of which ``transcribe(schedule="continuous")`` keeps one per file in flight (``stream_windows``); a check is
one device-to-host copy (``DeviceStepper.snapshot``).

A TEMPERATURE PER ROW: ``decode_continuous(temperatures=, attempts=)`` and ``transcribe(schedule="continuous",
seed=S)`` keep the state's sampling record with a row part (wipa_sample_rows_set: stream, attempt and 1 / temperature per slot, 0 for a
greedy row) and end the steps in the tails that read it (wipa_decode_call.sample_rows), so a window retried at a higher temperature
sits beside greedy first attempts and beside retries of other windows at other temperatures.  ``run_stream``'s source may hand a clip
out again, with its draw; ``_GroupStepper`` admits it from the encoder features its first admission left.

A PROMPT PER ROW: ``decode_continuous(prompts=)`` and ``transcribe(schedule="continuous",
condition_on_previous_text=True)``.  A clip is still admitted at the column the state stands at; its prompt ([sot_prev] + history)
stands IN FRONT of that column and goes through one batched pass over the admitted rows only (wipa_decoder_admit_rows_prompted), and
the steps end in the PROMPTED tails (wipa_decode_call.prompted).  So that a prompt always has room, a prompted run opens its
state at column ``prompt_room`` (wipa_decoder_seek) and the loop never shifts below it.
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .decoding import (DecoderState, DecodingOptions, DecodingResult, Sampling, _bank_of, _mask, _suppress_lists, compression_ratio,
                       decode_call, detect_language, timestamp_rules)
from .runtime import on_stream, ptr, sptr, stream_id
from .tokenizer import get_tokenizer


# ---------------------------------------------------------------- the scheduler (no GPU)
@dataclass
class ScheduleStats:
    steps: int = 0                                   # decoder steps run (every slot steps in each)
    shifts: List[int] = field(default_factory=list)  # the shift amounts, in order
    admissions: List[Tuple[int, int, int]] = field(default_factory=list)  # (slot, clip, column) in admission order
    retired: List[int] = field(default_factory=list)                      # clips in the order they were retired
    groups: List[int] = field(default_factory=list)                       # run_stream: the sizes of the admitted groups, in order
    live_rows: List[int] = field(default_factory=list)                    # the live rows of every interval of check_every steps


def default_column_limit(n_ctx: int, n_init: int, check_every: int) -> int:
    """the last column an interval may end at: ``n_text_ctx - 1 - check_every``, and never so high that an admission at it would leave no
    column to generate (n_init matters for check_every below it only)"""
    return n_ctx - 1 - max(check_every, n_init)


def run_schedule(stepper, n_clips: int, slots: int, n_init: int, limits: Sequence[int], eot: int, n_ctx: int, check_every: int = 8,
                 column_limit: Optional[int] = None, prompt_lens: Optional[Sequence[int]] = None, prompt_room: int = 0) -> ScheduleStats:
    """Decode clips 0 .. n_clips-1 through ``slots`` rows of ``stepper``:

      stepper.admit(pairs)              pairs [(slot, clip)]: the clips start at the current column of their slots
      stepper.run(n)                    n decoder steps of every slot
      stepper.last_tokens() -> [slots]  the token every slot holds at the current column (this is where the host waits)
      stepper.retire(slot, clip, first_column, n_columns)   copy the clip's generated columns and its log-probability sum out, in stream
                                        order -- before anything overwrites them
      stepper.shift(shift)              move every column down by ``shift``

    Clip i may generate ``limits[i]`` tokens.  A row is finished when its last token is ``eot`` or it has generated its limit; clips are
    admitted in input order into the lowest free slot.  The column counter is mirrored on the host (it advances by one per step); the loop
    is ``_run_slots``, which ``run_stream`` shares.
    ``prompt_lens`` / ``prompt_room``: clip i carries ``prompt_lens[i]`` prompt columns IN FRONT of its admission column, and the run keeps
    the column counter at or above ``prompt_room`` (the stepper opens its state there); 0 is the loop without prompts, call for call."""
    if slots < 1 or check_every < 1:
        raise ValueError(f"decode_continuous: slots = {slots} and check_every = {check_every} must be positive")
    if len(limits) != n_clips:
        raise ValueError(f"decode_continuous: {len(limits)} sample_lens for {n_clips} clips")
    if any(int(n) < 1 for n in limits):
        raise ValueError("decode_continuous: every clip generates at least one token (sample_lens >= 1)")
    if column_limit is None:
        column_limit = default_column_limit(n_ctx, n_init, check_every)
    longest = max([int(n) for n in limits], default=0)
    # a live row spans at most n_init + limit columns plus the steps up to the check that retires it; after a shift the oldest live row
    # starts at column 0 and the next interval must still fit
    need = prompt_room + n_init + longest + 2 * check_every - 1
    if not (column_limit + n_init < n_ctx and column_limit >= need):
        room = "prompt_room + " if prompt_room else ""
        raise ValueError(f"decode_continuous: column_limit = {column_limit} outside {need} .. {n_ctx - 1 - n_init} ({room}n_init + longest sample_len + "
                         f"2 * check_every - 1 .. n_text_ctx - 1 - n_init)")
    if prompt_lens is None:
        entries = [(clip, limits[clip]) for clip in range(n_clips)]
    else:
        if len(prompt_lens) != n_clips:
            raise ValueError(f"decode_continuous: {len(prompt_lens)} prompts for {n_clips} clips")
        entries = [(clip, limits[clip], None, range(int(prompt_lens[clip]))) for clip in range(n_clips)]  # the loop wants a prompt's length only
    batches = iter([entries])  # every clip is pending from the start, none later
    return _run_slots(stepper, ScheduleStats(), slots, n_init, eot, check_every, column_limit, lambda: next(batches, []),
                      lambda group: stepper.admit([(slot, clip) for slot, clip, *_ in group]),
                      lambda pos: (stepper.last_tokens(), stepper.retire), prompt_room=prompt_room)


def run_stream(stepper, source, slots: int, n_init: int, eot: int, n_ctx: int, check_every: int = 8,
               column_limit: Optional[int] = None, prompt_room: int = 0) -> ScheduleStats:
    """``run_schedule`` for clips that are not all known when the run starts (the windows of files: a file's next window exists once its
    previous one has retired).  The clips come from ``source`` and their results go back to it:

      source.pending() -> [(clip, limit)]   the clips that are ready now, each returned once, in the order they take slots; asked at the
                                            start and after every check (a retirement may have made more ready).  ``clip`` is any
                                            hashable value; it may generate ``limit`` tokens.  An entry may be (clip, limit, draw) with
                                            ``draw`` = None (greedy) or (temperature, attempt, stream): the row's own temperature, its
                                            index in the fallback schedule and its Philox stream (lo, hi).  A source may hand a clip out
                                            AGAIN after it has retired (a retry): it is admitted at the check that retired it.
                                            With ``prompt_room`` > 0 an entry may be (clip, limit, draw, prompt): ``prompt`` is the clip's
                                            prompt columns ([sot_prev] + history; empty or None: no prompt), which stand in front of
                                            its admission column; the run keeps the column counter at or above ``prompt_room``
      source.retired(clip, tokens, sum_logprob, no_speech)   the clip's generated tokens before its first ``eot`` (a list), its
                                            log-probability sum and its no-speech probability, as host values, at the check that retires it

      stepper.admit(triples)    [(slot, clip, limit)]: ONE call per check for all clips that start at the current column (a group); an
                                entry whose source gave a draw is (slot, clip, limit, draw), one with a prompt (slot, clip, limit, draw, prompt)
      stepper.run(n), stepper.shift(shift)   as for ``run_schedule``
      stepper.snapshot() -> (tokens [slots, >= column + 1], sums [slots], no_speech [slots])   host arrays from ONE device-to-host copy
                                            (this is where the host waits); everything a check retires is read from them

    Clips beyond the free slots wait in a queue, in the order ``pending`` gave them.  The run ends when nothing is live and nothing is
    pending."""
    if slots < 1 or check_every < 1:
        raise ValueError(f"decode_continuous: slots = {slots} and check_every = {check_every} must be positive")
    if column_limit is None:
        column_limit = default_column_limit(n_ctx, n_init, check_every)
    if not column_limit + n_init < n_ctx:
        raise ValueError(f"decode_continuous: column_limit = {column_limit} above {n_ctx - 1 - n_init} (n_text_ctx - 1 - n_init)")
    stats = ScheduleStats()

    def admit(group):
        for _, _, limit, *_ in group:
            # the bound of run_schedule, per clip: after a shift the oldest live row's sot sequence starts at column prompt_room at the
            # latest and the next interval must fit
            need = prompt_room + n_init + limit + 2 * check_every - 1
            if limit < 1 or need > column_limit:
                raise ValueError(f"decode_continuous: a clip's limit of {limit} tokens is outside 1 .. "
                                 f"{column_limit - prompt_room - n_init - 2 * check_every + 1} (column_limit"
                                 f"{' - prompt_room' if prompt_room else ''} - n_init - 2 * check_every + 1)")
        stepper.admit(group)
        stats.groups.append(len(group))

    def check(pos):
        tokens, sums, no_speech = stepper.snapshot()

        def retire(slot, clip, own, n_columns):
            row = [int(t) for t in tokens[slot][own:own + n_columns]]
            if eot in row:
                row = row[: row.index(eot)]
            source.retired(clip, row, float(sums[slot]), float(no_speech[slot]))

        return [row[pos] for row in tokens], retire

    return _run_slots(stepper, stats, slots, n_init, eot, check_every, column_limit, source.pending, admit, check, prompt_room=prompt_room)


def _run_slots(stepper, stats: ScheduleStats, slots: int, n_init: int, eot: int, check_every: int, column_limit: int, pending, admit,
               check, prompt_room: int = 0) -> ScheduleStats:
    """The loop of ``run_schedule`` and ``run_stream``: the column mirror, the shift rule, admission into the lowest free slot, the
    finished test and the stats.  What the two protocols differ in comes as three callables:

      pending() -> [(clip, limit, *draw)]   the clips that join the queue now; asked at the start and after every check
      admit(group)                          group [(slot, clip, limit, *draw)]: the clips that start at the current column, one call
      check(pos) -> (last, retire)          after an interval: ``last[slot]`` is the token a slot holds at column ``pos`` (this is where the
                                            host waits), ``retire(slot, clip, first_column, n_columns)`` takes a finished clip's columns out

    ``prompt_room`` = R > 0 (prompts in front of the admission column): the counter starts at R and no shift takes it below R, so a prompt
    of up to R columns always has room; an entry's fourth element is its prompt, and its row's window starts L = len(prompt) columns
    below its admission column.  R = 0 is the loop without prompts, call for call."""
    queue: deque = deque()
    live: Dict[int, Tuple[object, int, int, int]] = {}  # slot -> (clip, window start, limit, prompt columns)
    pos = int(prompt_room)
    if pos < 0:
        raise ValueError(f"decode_continuous: prompt_room = {prompt_room} must not be negative")

    def admit_pending():
        queue.extend(pending())
        group = []
        for slot in range(slots):
            if not queue:
                break
            if slot not in live:
                clip, limit, *rest = queue.popleft()
                n_prompt = len(rest[1]) if len(rest) > 1 and rest[1] is not None else 0
                if n_prompt > prompt_room:
                    raise ValueError(f"decode_continuous: a prompt of {n_prompt} columns does not fit prompt_room = {prompt_room}")
                live[slot] = (clip, pos - n_prompt, int(limit), n_prompt)
                group.append((slot, clip, int(limit), *rest))
                stats.admissions.append((slot, clip, pos))
        if group:
            admit(group)

    admit_pending()
    while live:
        if pos + check_every > column_limit:  # the next interval would pass the limit
            shift = min(min(start for _, start, _, _ in live.values()), pos - prompt_room)  # never below the prompt room
            assert shift > 0, "decode_continuous: a live row spans the whole column window (the shift would be 0)"
            stepper.shift(shift)
            stats.shifts.append(shift)
            pos -= shift
            live = {slot: (clip, start - shift, limit, n_prompt) for slot, (clip, start, limit, n_prompt) in live.items()}
            assert pos + check_every <= column_limit
        stats.live_rows.append(len(live))
        stepper.run(check_every)
        stats.steps += check_every
        pos += check_every
        last, retire = check(pos)
        for slot in sorted(live):
            clip, start, limit, n_prompt = live[slot]
            own = start + n_prompt + n_init
            generated = pos - own + 1  # columns own .. pos
            if generated >= 1 and (int(last[slot]) == eot or generated >= limit):
                retire(slot, clip, own, min(generated, limit))
                stats.retired.append(clip)
                del live[slot]
        admit_pending()
    return stats


def lockstep_steps(limits: Sequence[int], slots: int) -> int:
    """the generating steps a lockstep decode of the same clips takes: batches of ``slots`` in input order, each run to its longest row"""
    limits = [int(n) for n in limits]
    return sum(max(limits[i:i + slots]) for i in range(0, len(limits), slots))


def continuous_steps_bound(limits: Sequence[int], slots: int, n_init: int, check_every: int) -> int:
    """a lower bound on the steps of a continuous decode, from the lengths alone: every clip occupies a slot for at least the
    n_init - 1 steps of its prompt walk and its ``limit`` generating steps, ``slots`` slots work in parallel, and no schedule ends before
    its longest clip"""
    limits = [int(n) for n in limits]
    if not limits:
        return 0
    work = sum(n + n_init - 1 for n in limits)
    return max(-(-work // slots), max(limits) + n_init - 1)


# ---------------------------------------------------------------- the stepper on the library
class DeviceStepper:
    """``run_schedule``'s stepper on wipa_decoder_*: one decode state of ``slots`` rows, owned by the model per library stream."""

    def __init__(self, model, slots: int, features, initial, n_init: int, limits: Sequence[int], eot: int,
                 suppress_always: Sequence[int], suppress_first: Sequence[int], sample: Optional[Sampling], s, use_graph: bool = True,
                 rules: Optional["_lib.DecodeRules"] = None, no_speech_token: Optional[int] = None, row_seed: Optional[int] = None,
                 draws=None, prompts=None, prompt_room: Optional[int] = None, row_ids=None):
        """``rules``: the timestamp rules (wipa_decode_call.rules; None: the plain continuous tails).  With them and
        ``no_speech_token`` the step's tail leaves every row's no-speech probability in ``self.no_speech``.
        ``row_seed``: a TEMPERATURE PER ROW (wipa_decode_call.sample_rows; ``sample`` is then None): the state's sampling record
        with a row part is filled with this seed, and every admission writes the admitted clips' entries -- ``draws(clip)`` or the
        fourth element of an admitted tuple, (temperature, attempt, (stream_lo, stream_hi)); None is a greedy row.
        ``prompt_room`` (None: no prompts, the calls and the [2][B] starts buffer of the unprompted stepper): a PROMPTED stepper -- the
        state is opened at that column (wipa_decoder_seek), admissions go through wipa_decoder_admit_rows_prompted with the clips' prompt
        columns (``prompts(clip)`` or the fifth element of an admitted tuple: [sot_prev] + history, empty for none), the steps end in
        the prompted tails (wipa_decode_call.prompted), on a [3][B] starts buffer of its own.
        ``row_ids`` (clip -> an id of the model's adapter bank, -1 for none): the steps carry the bank (wipa_decode_call.bank); an admission
        writes the slot's id with a plain device copy and adds the clip's cross K / V terms (wipa_decoder_adapt_cross) before the slot's
        first step; a prompted admission does all of that itself (wipa_decoder_admit_rows_prompted_bank) and runs the prompt pass of the
        admitted rows under their adapters."""
        self.L = _lib.lib()
        self.model, self.B, self.s, self.eot, self.use_graph = model, int(slots), s, int(eot), use_graph
        self.features = features  # clip -> device tensor [n_audio_ctx, d] in the model's dtype, contiguous
        self.initial, self.n_init = initial, int(n_init)  # clip -> its n_init initial tokens, asked for when the clip is admitted
        if not 1 <= self.n_init <= 4:
            raise ValueError("decode_continuous: every clip takes the same number (1..4) of initial tokens")
        self.limits = [int(n) for n in limits]
        self.sample = sample
        if row_seed is not None and sample is not None:
            raise ValueError("decode_continuous: a temperature per row takes the place of the single-temperature sampling record")
        self.row_seed, self.draws = row_seed, draws
        self.row_ids = row_ids
        self.prompts, self.prompt_room = prompts, (int(prompt_room) if prompt_room is not None else None)
        if self.prompt_room is not None and not 0 <= self.prompt_room < model.dims.n_text_ctx - 1:
            raise ValueError(f"decode_continuous: prompt_room = {prompt_room} outside 0 .. n_text_ctx - 2")
        self.pk = pk = model.packed(absorbed=model.use_absorbed())  # the absorbed form where it applies, else the cached one
        states = model.__dict__.setdefault("_continuous_states", {})
        key = (stream_id(), self.B, int(pk["cfg"].dec_cross_absorbed))
        st = states.get(key)
        if st is not None and (st.blob.device != model.device or st.layout_key != _layout_key(pk, self.B)):
            s.synchronize()
            st.release()
            st = None
        if st is None:
            st = states[key] = DecoderState(model, self.B, pk)
        self.st = st
        if getattr(st, "_cont_starts", None) is None:  # ONE buffer per state: its address is part of the step graph's key
            st._cont_starts = torch.zeros(2 * self.B, dtype=torch.int32, device=model.device)
        self.starts = st._cont_starts
        if self.prompt_room is not None:  # a buffer of its own: the unprompted stepper's stays [2][B]
            if getattr(st, "_cont_starts_prompted", None) is None:
                st._cont_starts_prompted = torch.zeros(3 * self.B, dtype=torch.int32, device=model.device)
            self.starts = st._cont_starts_prompted
        self.rules = rules
        self.no_speech = None
        if rules is not None and no_speech_token is not None:
            if getattr(st, "_cont_no_speech", None) is None:  # ONE buffer per state, like the starts
                st._cont_no_speech = torch.zeros(self.B, dtype=torch.float32, device=model.device)
            self.no_speech = st._cont_no_speech
        self.rows = None
        if row_seed is not None:  # ONE buffer per state, like the starts: its address is part of the step graph's key
            nbytes = int(self.L.wipa_sample_rows_bytes(self.B))
            if getattr(st, "_cont_rows", None) is None:
                st._cont_rows = torch.zeros(nbytes, dtype=torch.uint8, device=model.device)
            self.rows = st._cont_rows
        self.no_speech_token = int(no_speech_token) if no_speech_token is not None else 0
        self.m_always = _mask(model, suppress_always)
        self.m_first = _mask(model, list(suppress_always) + list(suppress_first))
        n = len(self.limits)
        self.width = max(self.limits, default=1)
        self.out_tokens = torch.full((max(n, 1), self.width), self.eot, dtype=torch.int32, device=model.device)
        self.out_sums = torch.zeros(max(n, 1), dtype=torch.float32, device=model.device)
        self.out_no_speech = torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device=model.device)
        self.pos = 0
        self._keep = []  # what enqueued work reads
        self.bank = _bank_of(model, st, [-1] * self.B) if row_ids is not None else None  # every slot on the base until a clip is admitted
        self._begin()
        # every run of this stepper makes the same call: its buffers are one per state
        self.call = decode_call(self.n_init, self.eot, self.m_first, self.m_always, rules, self.rec, self.starts, continuous=True,
                                prompted=self.prompt_room is not None, sample_rows=self.rows, no_speech=self.no_speech,
                                no_speech_token=self.no_speech_token, bank=self.bank)

    def _begin(self):
        L, pk, st = self.L, self.pk, self.st
        init = (C.c_int32 * self.n_init)(*([0] * self.n_init))  # every slot is finished until a clip is admitted: start 0, limit 0
        _lib.check(L.wipa_decoder_begin(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), self.B, init, self.n_init, sptr(self.s)),
                   "wipa_decoder_begin")
        self.starts.zero_()
        if self.prompt_room is not None:  # open the prompt room: the idle state's position, once
            _lib.check(L.wipa_decoder_seek(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), self.B, self.prompt_room, sptr(self.s)),
                       "wipa_decoder_seek")
            self.pos = self.prompt_room
        if self.no_speech is not None:
            self.no_speech.fill_(float("nan"))
        if self.rows is not None:  # the header, and every row greedy until a clip is admitted
            host = np.zeros(self.rows.numel(), dtype=np.uint8)
            _lib.check(L.wipa_sample_rows_fill(host.ctypes.data, host.size, int(self.row_seed) & 0xFFFFFFFFFFFFFFFF, self.B), "wipa_sample_rows_fill")
            self.rows.copy_(torch.from_numpy(host))  # on the caller's library stream
        self.rec = None
        if self.sample is not None:  # seed, attempt and temperature; the streams are written per admission
            self.rec = st.sample_record(Sampling(self.sample.seed, self.sample.temperature, None, self.sample.attempt))

    def admit(self, pairs):
        """pairs [(slot, clip)] of ``run_schedule`` (the clip's limit is ``limits[clip]``), or triples [(slot, clip, limit)] of ``run_stream``,
        which may carry a fourth element: the clip's draw (temperature, attempt, stream) or None, and a fifth: its prompt columns"""
        limits = [int(t[2]) if len(t) > 2 else self.limits[t[1]] for t in pairs]
        given = [t[3] if len(t) > 3 else (self.draws(t[1]) if self.draws is not None else None) for t in pairs]
        prompt_rows = [list(t[4] or []) if len(t) > 4 else (list(self.prompts(t[1]) or []) if self.prompts is not None else []) for t in pairs]
        pairs = [(t[0], t[1]) for t in pairs]
        n = len(pairs)
        slots = (C.c_int32 * n)(*[slot for slot, _ in pairs])
        feats = [self.features(clip) for _, clip in pairs]
        self._keep.extend(feats)
        fptr = (C.c_void_p * n)(*[ptr(f) for f in feats])
        rows = [[int(t) for t in self.initial(clip)] for _, clip in pairs]
        assert all(len(r) == self.n_init for r in rows)
        init = (C.c_int32 * (n * self.n_init))(*[t for r in rows for t in r])
        lim = (C.c_int32 * n)(*limits)
        streams = None
        if self.sample is not None:
            own = self.sample.streams
            flat = [int(v) & 0xFFFFFFFF for _, clip in pairs for v in (own[clip] if own is not None else (clip, 0))]
            streams = (C.c_uint32 * (2 * n))(*flat)
        pk, st = self.pk, self.st
        ids = None
        if self.bank is not None:
            ids = [int(self.row_ids(clip)) for _, clip in pairs]
            if any(not -1 <= i < self.bank.n for i in ids):
                raise _lib.WipaError(f"row_adapters: ids {ids} outside -1 .. {self.bank.n - 1}")
        if self.prompt_room is not None:
            W = max(len(r) for r in prompt_rows)
            lens = (C.c_int32 * n)(*[len(r) for r in prompt_rows])
            flat = (C.c_int32 * max(n * W, 1))(*[int(t) for r in prompt_rows for t in [0] * (W - len(r)) + r])  # right-aligned
            nbytes = int(self.L.wipa_decoder_admit_prompted_workspace_bytes(C.byref(pk["cfg"]), n, W))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.model.device)
            self._keep.append(ws)
            args = (C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, n, slots, fptr, init, self.n_init, lim, lens, flat, W,
                    ptr(self.starts), ptr(self.rec) if self.rec is not None else None, streams, ptr(ws), nbytes)
            if self.bank is None:
                _lib.check(self.L.wipa_decoder_admit_rows_prompted(*args, sptr(self.s)), "wipa_decoder_admit_rows_prompted")
            else:  # the slots' ids, the clips' cross K / V terms and the prompt pass under the adapters: one call
                _lib.check(self.L.wipa_decoder_admit_rows_prompted_bank(*args, C.byref(self.bank), (C.c_int32 * n)(*ids), sptr(self.s)),
                           "wipa_decoder_admit_rows_prompted_bank")
        else:
            if any(prompt_rows):
                raise ValueError("decode_continuous: a clip came with a prompt, but the stepper was not built for prompts (prompt_room)")
            _lib.check(self.L.wipa_decoder_admit_rows(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, n, slots, fptr,
                                                      init, self.n_init, lim, ptr(self.starts), ptr(self.rec) if self.rec is not None else None,
                                                      streams, sptr(self.s)), "wipa_decoder_admit_rows")
        if self.bank is not None and self.prompt_room is None:  # the slots' ids, then the clips' cross K / V terms behind the projection
            st._bank_ids[torch.tensor([slot for slot, _ in pairs], device=st._bank_ids.device)] = torch.tensor(ids, dtype=torch.int32, device=st._bank_ids.device)
            for (slot, _), f in zip(pairs, feats):
                one = (C.c_int32 * 1)(slot)
                _lib.check(self.L.wipa_decoder_adapt_cross(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, ptr(f), 1, one,
                                                           C.byref(self.bank), sptr(self.s)), "wipa_decoder_adapt_cross")
        if self.rows is not None:  # the admitted slots' entries of the row record, in stream order behind the admission
            draws = [d if d is not None else (0.0, 0, (slot, 0)) for d, (slot, _) in zip(given, pairs)]
            flat = (C.c_uint32 * (2 * n))(*[int(v) & 0xFFFFFFFF for _, _, stream in draws for v in stream])
            attempts = (C.c_int32 * n)(*[int(a) for _, a, _ in draws])
            temps = (C.c_float * n)(*[float(t) for t, _, _ in draws])
            _lib.check(self.L.wipa_sample_rows_set(ptr(self.rows), self.B, n, slots, flat, attempts, temps, sptr(self.s)), "wipa_sample_rows_set")
        elif any(d is not None for d in given):
            raise ValueError("decode_continuous: a clip came with a draw, but the stepper was not built for a temperature per row (row_seed)")

    def run(self, n: int):
        pk, st = self.pk, self.st
        _lib.check(self.L.wipa_decoder_run_ex(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, C.byref(self.call), n,
                                              int(self.use_graph), sptr(self.s)), "wipa_decoder_run_ex")
        self.pos += n

    def last_tokens(self) -> np.ndarray:
        last = self.st.tokens[:, self.pos].cpu().numpy()  # synchronises the library stream
        if self.prompt_room is not None:
            self._keep.clear()  # every admission's prompt pass is done: its workspace is not held to the end of the run
        return last

    def retire(self, slot: int, clip: int, first_column: int, n_columns: int):
        self.out_tokens[clip, :n_columns].copy_(self.st.tokens[slot, first_column:first_column + n_columns])
        self.out_sums[clip].copy_(self.st.sum_logprobs[slot])
        if self.no_speech is not None:
            self.out_no_speech[clip].copy_(self.no_speech[slot])

    def snapshot(self):
        """``run_stream``'s check: (tokens [slots, column + 1], sums [slots], no_speech [slots]) on the host from ONE device-to-host copy
        (the three are packed into one int32 buffer on the device first); synchronises the library stream"""
        B, n = self.B, self.pos + 1
        nsp = self.no_speech if self.no_speech is not None else torch.full((B,), float("nan"), dtype=torch.float32, device=self.model.device)
        host = torch.cat([self.st.tokens[:, :n].reshape(-1), self.st.sum_logprobs.view(torch.int32), nsp.view(torch.int32)]).cpu().numpy()
        return host[: B * n].reshape(B, n), host[B * n: B * n + B].view(np.float32), host[B * n + B:].view(np.float32)

    def shift(self, shift: int):
        pk, st = self.pk, self.st
        _lib.check(self.L.wipa_decoder_shift_columns(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), self.B, ptr(self.starts), int(shift),
                                                     sptr(self.s)), "wipa_decoder_shift_columns")
        self.pos -= shift

    def results(self):
        """(tokens [clips, longest limit] int64 with eot behind a row's end, sum_logprobs [clips]) on the host; waits for the stream"""
        toks = self.out_tokens.cpu().numpy().astype(np.int64)
        sums = self.out_sums.cpu().numpy().copy()
        self._keep.clear()
        return toks, sums


def _layout_key(pk, B: int) -> tuple:
    lay = _lib.DecLayout()
    _lib.check(_lib.lib().wipa_decoder_layout(C.byref(pk["cfg"]), B, C.byref(lay)), "wipa_decoder_layout")
    return tuple(getattr(lay, f) for f, _ in lay._fields_)


# ---------------------------------------------------------------- the public entry point
def refuse_unserved(model, options: DecodingOptions, timestamps: bool = False) -> None:
    """what a continuous decode does not serve, each refused by the option's name.  ``timestamps``: the caller serves
    ``without_timestamps=False`` (``decode_continuous`` does, with wipa_decode_call.rules)"""
    if not options.without_timestamps and not timestamps:
        raise NotImplementedError("decode_continuous: without_timestamps=False is not implemented (the timestamp rules scan a row from a "
                                  "common first column); pass without_timestamps=True")
    for name in ("prompt", "prefix", "prompts"):
        value = getattr(options, name)
        if value is not None and len(value):
            raise NotImplementedError(f"decode_continuous: {name} is not implemented (prompt conditioning is served by decode())")
    if options.best_of is not None and options.best_of > 1:
        raise NotImplementedError("decode_continuous: best_of is not implemented (candidate groups are served by decode())")
    if options.beam_size:
        raise NotImplementedError("decode_continuous: beam_size is not implemented")
    if options.temperature < 0.0:
        raise ValueError(f"temperature must be >= 0, got {options.temperature}")
    if options.temperature != 0.0 and options.seed is None:
        raise NotImplementedError("decode_continuous: temperature above 0 needs DecodingOptions.seed (sampling is opt-in and reproducible)")
    if getattr(model, "_fp8", None):
        raise NotImplementedError("decode_continuous: an fp8-quantised model is not implemented (the continuous step runs on bf16 / f32 "
                                  "decoder tables)")


class _Features:
    """clip -> its encoder output, encoding mels in chunks of ``chunk`` clips ahead of need (the chunk a clip lies in and the one after
    it), and detecting the language and no-speech probability of a chunk when it is encoded"""

    def __init__(self, model, x: torch.Tensor, chunk: int, options: DecodingOptions, tok):
        d = model.dims
        self.model, self.x, self.chunk, self.options, self.tok = model, x, max(int(chunk), 1), options, tok
        self.encoded = model.is_features(x)  # by the effective N (model.audio_ctx)
        self.n = x.shape[0]
        self.chunks: Dict[int, torch.Tensor] = {}
        self.lang_token: Dict[int, int] = {}
        self.lang_probs: Dict[int, Optional[dict]] = {}
        self.no_speech: Dict[int, float] = {}

    def ensure(self, k: int):
        if k in self.chunks or k * self.chunk >= self.n:
            return
        lo, hi = k * self.chunk, min((k + 1) * self.chunk, self.n)
        part = self.x[lo:hi]
        feats = part if self.encoded else self.model.embed_audio(part)
        if self.options.fp16 and self.model.dtype == torch.float32:  # DecodingOptions.fp16: as decode() rounds the features
            with on_stream():
                feats = feats.to(torch.float16).to(torch.float32)
        with on_stream():
            feats = feats.to(device=self.model.device, dtype=self.model.dtype).contiguous()
        self.chunks[k] = feats
        if self.options.language is None:
            from .tokenizer import LANGUAGES

            lang_tokens, probs, nsp = detect_language(self.model, feats, self.tok, with_no_speech=True)
            for j in range(hi - lo):
                self.lang_token[lo + j] = int(lang_tokens[j])
                self.lang_probs[lo + j] = dict(zip(LANGUAGES[: self.tok.num_languages], probs[j].tolist()))
                self.no_speech[lo + j] = float(nsp[j])

    def __call__(self, clip: int) -> torch.Tensor:
        k = clip // self.chunk
        self.ensure(k)
        self.ensure(k + 1)
        for old in [c for c in self.chunks if c < k - 1]:  # consumed: every clip of it has been admitted, in input order
            del self.chunks[old]
        return self.chunks[k][clip - k * self.chunk]


class _GroupStepper(DeviceStepper):
    """``run_stream``'s stepper for ``transcribe(schedule="continuous")``: an admitted group's windows go through ONE log-mel call, ONE
    encoder call and ONE detect_language call (the windows of files whose language is still unknown), then ONE admission.
    ``seed``: the temperature fallback (a temperature per row).  A window's encoder features and initial tokens are HELD from its first
    admission until the source says the window is booked (``release``; the source calls it through its ``on_booked`` attribute): a
    window the source hands out again -- a retry -- is admitted from them, with no second log-mel, encoder or language detection, and
    ``source.group`` is asked for fresh windows only.  A file has one window in flight, so at most one feature tensor per active file."""

    def __init__(self, model, slots: int, source, options: DecodingOptions, tok, base, always, first, rules, s, seed: Optional[int] = None,
                 prompt_room: Optional[int] = None):
        self.source, self.options, self.tok, self.base = source, options, tok, list(base)
        self._held: Dict[object, Tuple[torch.Tensor, List[int]]] = {}
        source.on_booked = self.release
        super().__init__(model, slots, lambda clip: self._held[clip][0], lambda clip: self._held[clip][1], len(base), [], tok.eot, always, first,
                         None, s, rules=rules, no_speech_token=tok.no_speech, row_seed=seed, prompt_room=prompt_room)

    def release(self, clip):
        """the window is booked: nothing will ask for its features again"""
        self._held.pop(clip, None)

    def admit(self, triples):
        fresh = [t[1] for t in triples if t[1] not in self._held]
        if fresh:
            self._encode(fresh)
        super().admit(triples)

    def _encode(self, clips):
        from . import audio as A
        from .tokenizer import LANGUAGES

        windows, languages = self.source.group(clips)
        model = self.model
        dev_audio = torch.from_numpy(np.ascontiguousarray(windows)).to(model.device)
        feats = model.embed_audio(A.log_mel_spectrogram(dev_audio, n_mels=model.dims.n_mels))
        if self.options.fp16 and model.dtype == torch.float32:  # DecodingOptions.fp16: as decode() rounds the features
            feats = feats.to(torch.float16).to(torch.float32)
        feats = feats.to(device=model.device, dtype=model.dtype).contiguous()
        unknown = [j for j, lang in enumerate(languages) if lang is None]
        if unknown:
            lang_tokens, _ = detect_language(model, feats[unknown] if len(unknown) != len(clips) else feats, self.tok)
            found = [LANGUAGES[int(t) - self.tok.sot - 1] for t in lang_tokens]
            self.source.detected([clips[j] for j in unknown], found)
            for j, lang in zip(unknown, found):
                languages[j] = lang
        for j, clip in enumerate(clips):
            row = list(self.base)
            row[1] = self.tok.to_language_token(languages[j])
            self._held[clip] = (feats[j], row)

    def snapshot(self):
        out = super().snapshot()
        self._keep.clear()  # the stream has been waited for: every admission's copy of its features is done
        return out


def stream_windows(model, source, decode_options: dict, slots: int, check_every: int = 8,
                   column_limit: Optional[int] = None, seed: Optional[int] = None, prompt_room: Optional[int] = None) -> ScheduleStats:
    """The model's continuous decoder for ``transcribe(schedule="continuous")``: ``run_stream`` over ``source`` (transcribe._WindowSource:
    ``pending`` / ``retired`` of ``run_stream``, plus ``group(clips)`` -> (samples [n, 480000], languages) and ``detected(clips, languages)``)
    on ``slots`` rows, with timestamps.  Without ``seed`` every row is at temperature 0; with it the source's entries carry their draws
    (a retried window's temperature, attempt and stream) and the steps end in the tails with a temperature per row.  ``prompt_room``
    (None: no prompts): the source's entries carry their prompt columns as a fourth element, which stand in front of a window's admission
    column; the state is opened at that column and never shifted below it"""
    options = DecodingOptions(**{**decode_options, "without_timestamps": False, "temperature": 0.0})
    refuse_unserved(model, options, timestamps=True)
    tok = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=options.language or "en", task=options.task)
    always, first = _suppress_lists(options, tok)
    rules = timestamp_rules(tok, options.max_initial_timestamp)
    base = list(tok.sot_sequence)
    with on_stream() as s:
        stepper = _GroupStepper(model, slots, source, options, tok, base, always, first, rules, s, seed=seed, prompt_room=prompt_room)
        stats = run_stream(stepper, source, slots, len(base), tok.eot, model.dims.n_text_ctx, check_every, column_limit,
                           prompt_room=int(prompt_room) if prompt_room is not None else 0)
        stepper._keep.clear()
    return stats


def decode_continuous(model, mels_or_features: torch.Tensor, options: DecodingOptions = DecodingOptions(without_timestamps=True),
                      slots: int = 64, sample_lens: Optional[Sequence[int]] = None, check_every: int = 8,
                      column_limit: Optional[int] = None, stats_out: Optional[list] = None, temperatures: Optional[Sequence[float]] = None,
                      attempts: Optional[Sequence[int]] = None, prompts: Optional[Sequence[Sequence[int]]] = None,
                      prompt_room: Optional[int] = None, row_adapters: Optional[Sequence[Optional[str]]] = None) -> List[DecodingResult]:
    """``decode`` for a stream of clips through ``slots`` rows with refill: mels [N, 3000, n_mels] or encoded features [N, 1500, d];
    results in input order.  ``sample_lens``: the tokens clip i may generate (default ``options.sample_len`` or n_text_ctx // 2 for
    every clip).  Served: greedy, and ``temperature > 0`` with ``seed`` -- clip i draws from ``options.sample_streams[i]`` or from
    stream (i, 0), whichever slot it lands in and whenever it is admitted.  ``language=None`` detects the language (and fills
    ``no_speech_prob``) per encoded chunk of ``slots`` clips.  ``stats_out``: a list that receives the run's ``ScheduleStats``.
    ``without_timestamps=False``: the initial tokens are ``sot_sequence``, the timestamp rules of ``decode()`` run on every row's own
    sequence, and ``no_speech_prob`` is what the step's tail left at the row's <|startoftranscript|> column.
    ``temperatures``: a temperature >= 0 PER CLIP (0: a greedy clip), with ``attempts`` (default 0 for every clip) the clip's index in a
    fallback schedule; needs ``options.seed`` and ``options.temperature == 0``.  Clip i draws what ``decode`` draws for it at that
    temperature and attempt on its stream; the steps end in the tails with a temperature per row (wipa_decode_call.sample_rows).
    ``prompts``: the previous-text token ids PER CLIP, without ``sot_prev`` ([]: no prompt) -- clip i is decoded as ``decode`` decodes a row
    whose initial tokens are ``[sot_prev] + prompts[i] + sot_sequence`` (the last ``n_text_ctx // 2 - 1`` ids of a longer history, as
    there): its prompt stands in front of its admission column and goes through one batched pass when the clip is admitted (DESIGN.md
    section 16).  ``prompt_room`` (default: the longest prompt + 1) is the column the state is opened at and never shifted below; every
    prompt with its ``sot_prev`` must fit it.  The room comes out of the column window: ``prompt_room + n_init + the longest sample_len +
    2 * check_every - 1`` must not exceed ``column_limit`` (default ``n_text_ctx - 1 - check_every`` = 439), or ``ValueError`` names
    ``column_limit``.  So a full 223-token history (room 224) leaves 197 tokens to generate at ``check_every`` 8, not the default
    ``sample_len`` of 224: pass ``sample_lens`` / ``options.sample_len`` of at most 197, or shorter histories (196 tokens fit beside 224;
    ``transcribe``'s ``prompt_budget`` makes that cut).  Works with ``temperatures=`` / ``attempts=``; refused with ``best_of`` and on
    an fp8-quantised model.
    ``row_adapters``: an adapter name of the model's bank (``Whisper.set_adapter_bank``), or None, PER CLIP: the clip decodes under it
    in whichever slot it lands (the admission writes the slot's id and adds the clip's cross K / V terms); with ``prompts`` the
    clip's prompt pass runs under its adapter too."""
    row_ids = None
    if row_adapters is not None or options.row_adapters is not None:
        bank = getattr(model, "_bank", None)
        if bank is None:
            raise _lib.WipaError("row_adapters needs an adapter bank on the model: Whisper.set_adapter_bank(lora.AdapterBank(...))")
        names = list(row_adapters if row_adapters is not None else options.row_adapters)
        if len(names) != mels_or_features.shape[0]:
            raise ValueError(f"row_adapters: {len(names)} names for {mels_or_features.shape[0]} clips")
        row_ids = bank.ids(names)
    if prompts is not None:
        if options.best_of is not None and options.best_of > 1:
            raise NotImplementedError("decode_continuous: prompts with best_of is not implemented (candidate groups are served by decode())")
        if getattr(model, "_fp8", None):
            raise NotImplementedError("decode_continuous: prompts on an fp8-quantised model is not implemented (the prompt pass and the "
                                      "continuous step run on bf16 / f32 decoder tables)")
    elif prompt_room is not None:
        raise ValueError("decode_continuous: prompt_room comes with prompts")
    refuse_unserved(model, options, timestamps=True)
    if temperatures is None and attempts is not None:
        raise ValueError("decode_continuous: attempts comes with temperatures (a temperature and an attempt per clip)")
    if temperatures is not None:
        if options.seed is None:
            raise NotImplementedError("decode_continuous: temperatures needs DecodingOptions.seed (sampling is opt-in and reproducible)")
        if options.temperature != 0.0:
            raise ValueError("decode_continuous: temperatures (a temperature per clip) cannot be combined with options.temperature != 0")
        temperatures = [float(t) for t in temperatures]
        attempts = [int(a) for a in attempts] if attempts is not None else [0] * len(temperatures)
        if len(temperatures) != mels_or_features.shape[0] or len(attempts) != len(temperatures):
            raise ValueError(f"decode_continuous: {len(temperatures)} temperatures and {len(attempts)} attempts for {mels_or_features.shape[0]} clips")
        if any(not (t >= 0.0 and t < float("inf")) for t in temperatures):
            raise ValueError(f"decode_continuous: temperatures must be >= 0 and finite, got {temperatures}")
        if any(not 0 <= a < 65536 for a in attempts):
            raise ValueError(f"decode_continuous: attempts outside 0..65535: {attempts}")
    x = mels_or_features
    if x.dim() != 3:
        raise ValueError("decode_continuous: mels [N, 3000, n_mels] or features [N, n_audio_ctx, d]")
    d = model.dims
    N = x.shape[0]
    tok = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=options.language or "en", task=options.task)
    default_len = options.sample_len or d.n_text_ctx // 2
    limits = [int(n) for n in sample_lens] if sample_lens is not None else [int(default_len)] * N
    if len(limits) != N:
        raise ValueError(f"decode_continuous: {len(limits)} sample_lens for {N} clips")
    if N == 0:
        if stats_out is not None:
            stats_out.append(ScheduleStats())
        return []
    always, first = _suppress_lists(options, tok)
    timed = not options.without_timestamps
    rules = timestamp_rules(tok, options.max_initial_timestamp) if timed else None
    base = list(tok.sot_sequence) if timed else list(tok.sot_sequence_including_notimestamps)
    sample = None
    if options.temperature != 0.0:
        streams = [(int(a), int(b)) for a, b in options.sample_streams] if options.sample_streams is not None else [(i, 0) for i in range(N)]
        if len(streams) != N:
            raise ValueError(f"sample_streams: {len(streams)} streams for {N} clips")
        sample = Sampling(int(options.seed), float(options.temperature), streams, int(options.sample_attempt))
    draws = None
    if temperatures is not None and N:
        row_streams = [(int(a), int(b)) for a, b in options.sample_streams] if options.sample_streams is not None else [(i, 0) for i in range(N)]
        if len(row_streams) != N:
            raise ValueError(f"sample_streams: {len(row_streams)} streams for {N} clips")

        def draws(clip: int):
            return temperatures[clip], attempts[clip], row_streams[clip]

    prompt_rows = None
    if prompts is not None:
        if len(prompts) != N:
            raise ValueError(f"decode_continuous: {len(prompts)} prompts for {N} clips")
        # upstream's _get_initial_tokens, as decode(prompts=) builds a row: [sot_prev] + the last n_text_ctx // 2 - 1 tokens of the history
        keep = d.n_text_ctx // 2 - 1
        prompt_rows = [([int(tok.sot_prev)] + [int(t) for t in list(ids)[-keep:]]) if len(ids) else [] for ids in prompts]
        longest = max(len(r) for r in prompt_rows)
        room = longest if prompt_room is None else int(prompt_room)
        if not longest <= room <= d.n_text_ctx - len(base) - 1:
            raise ValueError(f"decode_continuous: prompt_room = {room} outside {longest} .. {d.n_text_ctx - len(base) - 1} (the longest prompt + 1 "
                             f".. n_text_ctx - n_init - 1)")
    feats = _Features(model, x, slots, options, tok)

    def initial(clip: int) -> List[int]:  # with language=None the chunk's detection has run when the clip is admitted
        row = list(base)
        if options.language is None:
            feats(clip)
            row[1] = feats.lang_token[clip]
        return row

    with on_stream() as s:
        stepper = DeviceStepper(model, slots, feats, initial, len(base), limits, tok.eot, always, first, sample, s, rules=rules,
                                no_speech_token=tok.no_speech if timed else None, row_seed=int(options.seed) if draws is not None else None,
                                draws=draws, prompts=(lambda clip: prompt_rows[clip]) if prompt_rows is not None else None,
                                prompt_room=room if prompt_rows is not None else None,
                                row_ids=(lambda clip: row_ids[clip]) if row_ids is not None else None)
        if prompt_rows is None:
            stats = run_schedule(stepper, N, slots, len(base), limits, tok.eot, d.n_text_ctx, check_every, column_limit)
        else:
            stats = run_schedule(stepper, N, slots, len(base), limits, tok.eot, d.n_text_ctx, check_every, column_limit,
                                 prompt_lens=[len(r) for r in prompt_rows], prompt_room=room)
        tail_no_speech = stepper.out_no_speech.cpu().numpy() if timed else None
        toks, sums = stepper.results()
    if stats_out is not None:
        stats_out.append(stats)
    from .tokenizer import LANGUAGES

    results = []
    for i in range(N):
        row = toks[i, : limits[i]].tolist()
        if tok.eot in row:
            row = row[: row.index(tok.eot)]
        text = tok.decode([t for t in row if t < tok.timestamp_begin]).strip()
        comp = compression_ratio(text)
        lang = options.language or "en"
        if options.language is None:
            lang = LANGUAGES[feats.lang_token[i] - tok.sot - 1]
        # the features the caller gave; those encoded here are dropped chunk by chunk once their clips are admitted
        results.append(DecodingResult(audio_features=x[i] if feats.encoded else None, language=lang, language_probs=feats.lang_probs.get(i), tokens=row, text=text,
                                      avg_logprob=float(sums[i]) / (len(row) + 1),
                                      temperature=temperatures[i] if temperatures is not None else options.temperature, compression_ratio=comp,
                                      no_speech_prob=float(tail_no_speech[i]) if timed else feats.no_speech.get(i, float("nan"))))
    return results
