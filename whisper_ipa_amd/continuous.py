"""Continuous-batching decode: the rows of one decode state are SLOTS, and a slot whose clip has finished takes the next clip while the
other rows go on (include/wipa.h: wipa_decoder_admit_rows / wipa_decoder_shift_columns /
wipa_decoder_run_continuous).

``decode`` runs a batch in lockstep: every row steps until the last one has reached EOT, and a row that ended early sits EOT-latched
in its slot, its encoder output still streamed through every cross-attention layer of every step.  Here the host looks at the last
token column every ``check_every`` steps, retires the rows that have finished -- their tokens and log-probability sums are copied out in
stream order -- and admits the next pending clips into the freed slots at the column the state stands at.  Every row has its own first
column (``start``), so its position embeddings, attention window, sampling counter and prompt end are its own; when the shared column
counter nears the end of the table, all columns move down by the smallest start among the live rows (a *shift*), which no row can see.

The scheduler (``run_schedule``) is plain Python against a small stepper interface, so it is tested without a GPU; ``DeviceStepper`` is
the stepper on the library.
"""
from __future__ import annotations

import ctypes as C
import zlib
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .decoding import (DecoderState, DecodingOptions, DecodingResult, Sampling, _mask, _suppress_lists, detect_language)
from .runtime import on_stream, ptr, sptr, stream_id
from .tokenizer import get_tokenizer


# ---------------------------------------------------------------- the scheduler (no GPU)
@dataclass
class ScheduleStats:
    steps: int = 0                                   # decoder steps run (every slot steps in each)
    shifts: List[int] = field(default_factory=list)  # the shift amounts, in order
    admissions: List[Tuple[int, int, int]] = field(default_factory=list)  # (slot, clip, column) in admission order
    retired: List[int] = field(default_factory=list)                      # clips in the order they were retired


def default_column_limit(n_ctx: int, n_init: int, check_every: int) -> int:
    """the last column an interval may end at: ``n_text_ctx - 1 - check_every``, and never so high that an admission at it would leave no
    column to generate (n_init matters for check_every below it only)"""
    return n_ctx - 1 - max(check_every, n_init)


def run_schedule(stepper, n_clips: int, slots: int, n_init: int, limits: Sequence[int], eot: int, n_ctx: int, check_every: int = 8,
                 column_limit: Optional[int] = None) -> ScheduleStats:
    """Decode clips 0 .. n_clips-1 through ``slots`` rows of ``stepper``:

      stepper.admit(pairs)              pairs [(slot, clip)]: the clips start at the current column of their slots
      stepper.run(n)                    n decoder steps of every slot
      stepper.last_tokens() -> [slots]  the token every slot holds at the current column (this is where the host waits)
      stepper.retire(slot, clip, first_column, n_columns)   copy the clip's generated columns and its log-probability sum out, in stream
                                        order -- before anything overwrites them
      stepper.shift(shift)              move every column down by ``shift``

    Clip i may generate ``limits[i]`` tokens.  A row is finished when its last token is ``eot`` or it has generated its limit; clips are
    admitted in input order into the lowest free slot.  The column counter is mirrored here (it advances by one per step)."""
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
    need = n_init + longest + 2 * check_every - 1
    if not (column_limit + n_init < n_ctx and column_limit >= need):
        raise ValueError(f"decode_continuous: column_limit = {column_limit} outside {need} .. {n_ctx - 1 - n_init} (n_init + longest sample_len + "
                         f"2 * check_every - 1 .. n_text_ctx - 1 - n_init)")
    stats = ScheduleStats()
    queue = deque(range(n_clips))
    live: Dict[int, Tuple[int, int]] = {}  # slot -> (clip, start)
    pos = 0

    def admit_pending():
        pairs = []
        for slot in range(slots):
            if not queue:
                break
            if slot not in live:
                clip = queue.popleft()
                live[slot] = (clip, pos)
                pairs.append((slot, clip))
                stats.admissions.append((slot, clip, pos))
        if pairs:
            stepper.admit(pairs)

    admit_pending()
    while live:
        if pos + check_every > column_limit:  # the next interval would pass the limit
            shift = min(start for _, start in live.values())
            assert shift > 0, "decode_continuous: a live row spans the whole column window (the shift would be 0)"
            stepper.shift(shift)
            stats.shifts.append(shift)
            pos -= shift
            live = {slot: (clip, start - shift) for slot, (clip, start) in live.items()}
            assert pos + check_every <= column_limit
        stepper.run(check_every)
        stats.steps += check_every
        pos += check_every
        last = stepper.last_tokens()
        for slot in sorted(live):
            clip, start = live[slot]
            generated = pos - (start + n_init) + 1  # columns start + n_init .. pos
            if generated >= 1 and (int(last[slot]) == eot or generated >= int(limits[clip])):
                stepper.retire(slot, clip, start + n_init, min(generated, int(limits[clip])))
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
                 suppress_always: Sequence[int], suppress_first: Sequence[int], sample: Optional[Sampling], s, use_graph: bool = True):
        self.L = _lib.lib()
        self.model, self.B, self.s, self.eot, self.use_graph = model, int(slots), s, int(eot), use_graph
        self.features = features  # clip -> device tensor [n_audio_ctx, d] in the model's dtype, contiguous
        self.initial, self.n_init = initial, int(n_init)  # clip -> its n_init initial tokens, asked for when the clip is admitted
        if not 1 <= self.n_init <= 4:
            raise ValueError("decode_continuous: every clip takes the same number (1..4) of initial tokens")
        self.limits = [int(n) for n in limits]
        self.sample = sample
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
        self.m_always = _mask(model, suppress_always)
        self.m_first = _mask(model, list(suppress_always) + list(suppress_first))
        n = len(self.limits)
        self.width = max(self.limits, default=1)
        self.out_tokens = torch.full((max(n, 1), self.width), self.eot, dtype=torch.int32, device=model.device)
        self.out_sums = torch.zeros(max(n, 1), dtype=torch.float32, device=model.device)
        self.pos = 0
        self._keep = []  # what enqueued work reads
        self._begin()

    def _begin(self):
        L, pk, st = self.L, self.pk, self.st
        init = (C.c_int32 * self.n_init)(*([0] * self.n_init))  # every slot is finished until a clip is admitted: start 0, limit 0
        _lib.check(L.wipa_decoder_begin(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), self.B, init, self.n_init, sptr(self.s)),
                   "wipa_decoder_begin")
        self.starts.zero_()
        self.rec = None
        if self.sample is not None:  # seed, attempt and temperature; the streams are written per admission
            self.rec = st.sample_record(Sampling(self.sample.seed, self.sample.temperature, None, self.sample.attempt))

    def admit(self, pairs):
        n = len(pairs)
        slots = (C.c_int32 * n)(*[slot for slot, _ in pairs])
        feats = [self.features(clip) for _, clip in pairs]
        self._keep.extend(feats)
        fptr = (C.c_void_p * n)(*[ptr(f) for f in feats])
        rows = [[int(t) for t in self.initial(clip)] for _, clip in pairs]
        assert all(len(r) == self.n_init for r in rows)
        init = (C.c_int32 * (n * self.n_init))(*[t for r in rows for t in r])
        lim = (C.c_int32 * n)(*[self.limits[clip] for _, clip in pairs])
        streams = None
        if self.sample is not None:
            own = self.sample.streams
            flat = [int(v) & 0xFFFFFFFF for _, clip in pairs for v in (own[clip] if own is not None else (clip, 0))]
            streams = (C.c_uint32 * (2 * n))(*flat)
        pk, st = self.pk, self.st
        _lib.check(self.L.wipa_decoder_admit_rows(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, n, slots, fptr, init,
                                                  self.n_init, lim, ptr(self.starts), ptr(self.rec) if self.rec is not None else None, streams,
                                                  sptr(self.s)), "wipa_decoder_admit_rows")

    def run(self, n: int):
        pk, st = self.pk, self.st
        _lib.check(self.L.wipa_decoder_run_continuous(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), self.B, self.n_init,
                                                      self.eot, ptr(self.m_first), ptr(self.m_always), n, int(self.use_graph), None,
                                                      ptr(self.rec) if self.rec is not None else None, ptr(self.starts), sptr(self.s)),
                   "wipa_decoder_run_continuous")
        self.pos += n

    def last_tokens(self) -> np.ndarray:
        return self.st.tokens[:, self.pos].cpu().numpy()  # synchronises the library stream

    def retire(self, slot: int, clip: int, first_column: int, n_columns: int):
        self.out_tokens[clip, :n_columns].copy_(self.st.tokens[slot, first_column:first_column + n_columns])
        self.out_sums[clip].copy_(self.st.sum_logprobs[slot])

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
def refuse_unserved(model, options: DecodingOptions) -> None:
    """what ``decode_continuous`` does not serve, each refused by the option's name"""
    if not options.without_timestamps:
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
        self.encoded = tuple(x.shape[-2:]) == (d.n_audio_ctx, d.n_audio_state)
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


def decode_continuous(model, mels_or_features: torch.Tensor, options: DecodingOptions = DecodingOptions(without_timestamps=True),
                      slots: int = 64, sample_lens: Optional[Sequence[int]] = None, check_every: int = 8,
                      column_limit: Optional[int] = None, stats_out: Optional[list] = None) -> List[DecodingResult]:
    """``decode`` for a stream of clips through ``slots`` rows with refill: mels [N, 3000, n_mels] or encoded features [N, 1500, d];
    results in input order.  ``sample_lens``: the tokens clip i may generate (default ``options.sample_len`` or n_text_ctx // 2 for
    every clip).  Served: greedy, and ``temperature > 0`` with ``seed`` -- clip i draws from ``options.sample_streams[i]`` or from
    stream (i, 0), whichever slot it lands in and whenever it is admitted.  ``language=None`` detects the language (and fills
    ``no_speech_prob``) per encoded chunk of ``slots`` clips.  ``stats_out``: a list that receives the run's ``ScheduleStats``."""
    refuse_unserved(model, options)
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
    base = list(tok.sot_sequence_including_notimestamps)
    sample = None
    if options.temperature != 0.0:
        streams = [(int(a), int(b)) for a, b in options.sample_streams] if options.sample_streams is not None else [(i, 0) for i in range(N)]
        if len(streams) != N:
            raise ValueError(f"sample_streams: {len(streams)} streams for {N} clips")
        sample = Sampling(int(options.seed), float(options.temperature), streams, int(options.sample_attempt))
    feats = _Features(model, x, slots, options, tok)

    def initial(clip: int) -> List[int]:  # with language=None the chunk's detection has run when the clip is admitted
        row = list(base)
        if options.language is None:
            feats(clip)
            row[1] = feats.lang_token[clip]
        return row

    with on_stream() as s:
        stepper = DeviceStepper(model, slots, feats, initial, len(base), limits, tok.eot, always, first, sample, s)
        stats = run_schedule(stepper, N, slots, len(base), limits, tok.eot, d.n_text_ctx, check_every, column_limit)
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
        comp = len(text.encode("utf-8")) / max(len(zlib.compress(text.encode("utf-8"))), 1) if text else float("nan")
        lang = options.language or "en"
        if options.language is None:
            lang = LANGUAGES[feats.lang_token[i] - tok.sot - 1]
        # the features the caller gave; those encoded here are dropped chunk by chunk once their clips are admitted
        results.append(DecodingResult(audio_features=x[i] if feats.encoded else None, language=lang, language_probs=feats.lang_probs.get(i), tokens=row, text=text,
                                      avg_logprob=float(sums[i]) / (len(row) + 1), temperature=options.temperature, compression_ratio=comp,
                                      no_speech_prob=feats.no_speech.get(i, float("nan"))))
    return results
