"""``transcribe(model, audio, ...)``: mlx_whisper.transcribe as the reference's base-model leg calls it
(scripts/evaluate_model.py:112-119: ``mlx_whisper.transcribe(audio_path, path_or_hf_repo=..., language=..., word_timestamps=False)``)
-- decode with timestamps on, cut the result into segments at consecutive timestamp pairs, skip silent windows, and walk files
longer than 30 s window by window.  The window loop is openai-whisper's transcribe.py (mlx_whisper 0.4.3 ports it;
[UPSTREAM-UNVERIFIED] where the port cannot be inspected): ``seek`` advances in mel frames, to the last closed timestamp pair
unless the window ends in a single timestamp.

What differs from upstream, on purpose:
  * the next windows of ALL files still in progress go through log-mel, encoder and decode as one batch per round (rows of one
    batch belong to different files at different seeks); upstream transcribes one file at a time;
  * each window's log-mel is computed from the window's own samples (``pad_or_trim`` + the existing kernel), so the 8 dB floor
    under the maximum is per window; upstream computes one log-mel of the whole file.  A single-window file is unaffected;
  * the temperature fallback is keyed on ``seed``.  With ``seed=None`` only temperature 0 runs: where
    ``compression_ratio_threshold`` / ``logprob_threshold`` would have made upstream retry at a higher temperature, the window's
    segments carry ``needs_fallback=True`` and one warning is printed per call.  With a seed the failing windows of a round are
    decoded again, as ONE sub-batch per temperature of the schedule, from the encoder features the first decode left (no second
    log-mel, no second encoder pass), until they pass or the schedule ends (the last attempt is kept, as upstream does).  The draw
    is a function of (seed, (seek, file index), index in the schedule, position, column): a window samples the same tokens
    whichever rows it is retried with.  Upstream draws from a global generator instead.  ``best_of=N`` (with a seed) is dropped at
    temperature 0, as upstream's decode_with_fallback drops it, and passed to every retry: the window is then decoded as N candidates
    that share its encoder output, candidate k on stream (seek, file index + (k << 24)), and the retry's result is the candidate
    with the highest length-normalised log-probability (decoding.py).  A custom ``fallback_fn`` receives ``best_of=N``; a custom
    ``decode_fn`` without a ``fallback_fn`` cannot serve it and is refused;
  * ``word_timestamps=True``: after a round's decode and fallback, the windows that were not skipped go through ONE
    ``timing.find_alignment`` call from the encoder features their decode left (no second log-mel, no second encoder pass), and
    every segment gains ``"words"``.  Upstream's word-duration heuristics, its snapping of segment bounds to the words and of
    ``seek`` to the last word are left out (timing.py says why), so segments and seeks are those of ``word_timestamps=False``.
    An fp8-quantised model is refused before anything is decoded;
  * ``condition_on_previous_text`` defaults to False.  With True -- or with an ``initial_prompt`` -- every file keeps upstream's
    bookkeeping (``all_tokens``, ``prompt_reset_since``; a window decoded above temperature 0.5 resets the prompt, a skipped window
    changes nothing) and the rows of a round carry their OWN prompts, of different lengths, through ``decode(prompts=...)``: the
    ragged decode of decoding.py.  One deviation comes with batching (decoding.py's docstring): ``sample_len`` is clamped to
    ``n_text_ctx`` minus the round's common prompt width, so a window next to one with a full 223-token history generates at most
    221 tokens, not 224;
  * ``schedule="continuous"`` (the default is ``"rounds"``, everything above): the windows go through ``min(slots, files)`` rows of ONE
    decode state with refill (continuous.py) instead of one lockstep batch per round.  A file is a stream of
    windows with at most one in flight; files take places in input order and wait beyond ``slots``; the windows that become ready at
    the same check share one log-mel, one encoder, one language-detection and one admission call.  The per-window bookkeeping
    (``_Books.window``) is the rounds schedule's.  With ``seed`` the temperature fallback runs on this schedule too: a window that
    fails the thresholds is not booked, its file keeps its place, and the SAME window becomes pending again at the next temperature
    of the schedule, with the stream (seek, file index), the attempt index and the seed of the rounds schedule's retry -- so both
    schedules draw the same tokens.  It is admitted at the check that retired the failed attempt, from the encoder features its first
    admission left (no second log-mel, encoder or language detection), into a row that sits beside greedy first attempts and beside
    retries of other windows at other temperatures: the decode state's sampling record holds a temperature per row
    (wipa_decode_call.sample_rows).  The window is booked when it passes or the schedule ends (the last attempt is kept).
    Conditioning (``condition_on_previous_text`` / ``initial_prompt``) runs on this schedule too: a file's next window exists once its
    previous one is booked, so ``_WindowSource.pending`` hands it out with the prompt the rounds loop would build, and the prompt stands
    in front of the window's admission column (continuous.py).  ``prompt_budget`` bounds the history kept.
    ``word_timestamps``, ``best_of``, a custom ``decode_fn`` and fp8 models are refused by name, and so are ``seed`` with a custom
    ``stream_fn`` that does not declare ``stream_fn.retries = True`` and conditioning with one that does not declare
    ``stream_fn.prompts = True``.
"""
from __future__ import annotations

import inspect
import warnings
from collections import deque
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .audio import HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE

FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH  # 100 mel frames per second
INPUT_STRIDE = 2                               # mel frames per encoder output position (N_FRAMES // n_audio_ctx)
TIME_PRECISION = INPUT_STRIDE * HOP_LENGTH / SAMPLE_RATE  # 0.02 s per timestamp token

SEGMENT_KEYS = ("id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob")


def split_segments(tokens: Sequence[int], tb: int, time_offset: float, segment_size: int) -> Tuple[List[dict], int]:
    """One decoded window -> (segments, seek advance in mel frames).  ``tokens``: the window's sampled ids up to EOT, timestamps
    included; ``tb``: timestamp_begin; ``segment_size``: the window's content in mel frames (<= 3000).  Each segment is
    {"start", "end", "tokens"}.  Segments are cut at consecutive timestamp pairs; if the window ends in a single timestamp the
    tail after the last pair is a segment too and the whole window is consumed, otherwise ``seek`` moves to the last pair and the
    tail is decoded again with the next window.  Without any pair the window is one segment: up to its last timestamp if that is
    not <|0.00|>, else spanning the window."""
    tokens = [int(t) for t in tokens]
    is_ts = [t >= tb for t in tokens]
    single_timestamp_ending = is_ts[-2:] == [False, True]
    consecutive = [i + 1 for i in range(len(tokens) - 1) if is_ts[i] and is_ts[i + 1]]
    segments: List[dict] = []
    if consecutive:
        slices = list(consecutive)
        if single_timestamp_ending:
            slices.append(len(tokens))
        last = 0
        for cur in slices:
            sl = tokens[last:cur]
            segments.append({"start": time_offset + (sl[0] - tb) * TIME_PRECISION, "end": time_offset + (sl[-1] - tb) * TIME_PRECISION,
                             "tokens": sl})
            last = cur
        if single_timestamp_ending:
            return segments, segment_size
        return segments, (tokens[last - 1] - tb) * INPUT_STRIDE
    duration = segment_size * HOP_LENGTH / SAMPLE_RATE
    stamps = [t for t in tokens if t >= tb]
    if stamps and stamps[-1] != tb:
        duration = (stamps[-1] - tb) * TIME_PRECISION
    segments.append({"start": time_offset, "end": time_offset + duration, "tokens": tokens})
    return segments, segment_size


def _refuse(condition_on_previous_text, initial_prompt, word_timestamps, clip_timestamps, hallucination_silence_threshold, temperature,
            decode_options, can_align: bool = False, can_retry: bool = True, can_beam: bool = False) -> None:
    if word_timestamps and not can_align:
        raise NotImplementedError("word_timestamps=True is not implemented without a model: a custom decode_fn needs an align_fn")
    if clip_timestamps not in (None, "0", [0], (0,)):
        raise NotImplementedError("clip_timestamps is not implemented")
    if hallucination_silence_threshold is not None:
        raise NotImplementedError("hallucination_silence_threshold is not implemented")
    temps = (temperature,) if isinstance(temperature, (int, float)) else tuple(temperature)
    if not temps or float(temps[0]) != 0.0:
        raise NotImplementedError("temperature must be 0.0 or a tuple that starts with 0.0: only temperature 0 is run")
    for k in ("prompt", "prefix"):
        if decode_options.get(k) is not None:
            raise NotImplementedError(f"{k} is not implemented")
    if decode_options.get("beam_size") is not None:
        # beams are a capability of the decoder: the package's own has it, a custom decode_fn says so with a ``beams`` attribute
        if not can_beam:
            raise NotImplementedError("beam_size is not implemented for a custom decode_fn without a beams attribute: the temperature-0 "
                                      "decode of every window runs the beams (decode_fn.beams = True)")
        if condition_on_previous_text or initial_prompt is not None:
            raise NotImplementedError("beam_size with condition_on_previous_text=True / initial_prompt is not implemented: beams run on "
                                      "rows without prompts")
        if word_timestamps:
            raise NotImplementedError("beam_size with word_timestamps=True is not implemented")
    if decode_options.get("best_of") is not None and not can_retry:
        raise NotImplementedError("best_of is not implemented for a custom decode_fn without a fallback_fn: the candidates are drawn by "
                                  "the retries (fallback_fn(..., best_of=N))")


def _takes_prompts(fn: Callable) -> bool:
    try:
        params = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return "prompts" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _refuse_conditioning(condition_on_previous_text, initial_prompt, model, decode_fn, fallback_fn) -> None:
    """prompt conditioning needs decoders that take the rows' prompts: a custom one without a ``prompts`` parameter is refused (the
    pattern of ``align_fn`` for word timestamps), and so is an fp8-quantised model"""
    if not condition_on_previous_text and initial_prompt is None:
        return
    name = "condition_on_previous_text=True" if condition_on_previous_text else "initial_prompt"
    for what, fn in (("decode_fn", decode_fn), ("fallback_fn", fallback_fn)):
        if fn is not None and not _takes_prompts(fn):
            raise NotImplementedError(f"{name} is not implemented for a custom {what} without a prompts= parameter: every round's rows "
                                      f"carry their own prompts ({what}(..., prompts=[...]))")
    if decode_fn is None and getattr(model, "_fp8", None):
        raise NotImplementedError(f"{name} is not implemented for an fp8-quantised model: the ragged decode step runs on bf16 / f32 "
                                  "decoder tables")


def _model_decoder(model, decode_options: dict) -> Callable:
    """the default ``decode_fn``: windows [n, 480000] f32 + per-row languages (None: detect) -> DecodingResults, through the
    package's log-mel, encoder and ``decode(without_timestamps=False)``; rows are grouped by language"""
    import torch

    from . import audio as A
    from .decoding import DecodingOptions, decode

    def with_prompts(opts: dict, prompts, rows) -> dict:
        """the rows' own prompts (token ids; an empty one is no prompt), when the caller conditions on previous text"""
        if prompts is not None and any(len(prompts[i]) for i in rows):
            opts["prompts"] = [list(prompts[i]) for i in rows]
        return opts

    def with_adapters(opts: dict, row_adapters, rows) -> dict:
        """the rows' adapters of the model's bank (transcribe(row_adapters=[per file]): a window carries its file's)"""
        if row_adapters is not None:
            opts["row_adapters"] = [row_adapters[i] for i in rows]
        return opts

    def run(windows: np.ndarray, languages: List[Optional[str]], prompts=None, row_adapters=None):
        out = [None] * len(languages)
        dev_audio = torch.from_numpy(np.ascontiguousarray(windows)).to(model.device)
        mel = A.log_mel_spectrogram(dev_audio, n_mels=model.dims.n_mels)
        for lang in sorted(set(languages), key=lambda l: (l is not None, l or "")):
            rows = [i for i, l in enumerate(languages) if l == lang]
            opts = DecodingOptions(**with_adapters(with_prompts({**decode_options, "language": lang, "without_timestamps": False,
                                                                 "temperature": 0.0}, prompts, rows), row_adapters, rows))
            res = decode(model, mel[rows] if len(rows) != len(languages) else mel, opts)
            for i, r in zip(rows, res):
                out[i] = r
        return out

    def retry(results, languages: List[str], *, temperature: float, attempt: int, streams, seed: int, prompts=None, best_of=None,
              row_adapters=None):
        """the default ``fallback_fn``: the rows' encoder features (``DecodingResult.audio_features``) decoded again at
        ``temperature``, each row on its own stream and with the prompt it was first decoded with; ``best_of``: as that many
        candidates per row, of which decode() keeps the best"""
        out = [None] * len(results)
        feats = torch.stack([r.audio_features for r in results])
        # upstream's decode_with_fallback: above temperature 0 the beams are dropped (beam_size, patience), best_of takes their place
        sampling_options = {k: v for k, v in decode_options.items() if k not in ("beam_size", "patience")}
        for lang in sorted(set(languages)):
            rows = [i for i, l in enumerate(languages) if l == lang]
            opts = DecodingOptions(**with_adapters(with_prompts({**sampling_options, "language": lang, "without_timestamps": False,
                                                   "temperature": float(temperature), "seed": int(seed),
                                                   "sample_streams": [streams[i] for i in rows], "sample_attempt": int(attempt),
                                                   **({"best_of": int(best_of)} if best_of is not None else {})}, prompts, rows),
                                                   row_adapters, rows))
            res = decode(model, feats[rows] if len(rows) != len(languages) else feats, opts)
            for i, r in zip(rows, res):
                out[i] = r
        return out

    run.retry = retry
    return run


def _add_words(model, tok, to_align, prepend_punctuations, append_punctuations, align_fn) -> None:
    """one alignment call for the round's windows; every segment of ``to_align`` gains "words".  As upstream, the words are
    found and dealt on the tokens every segment was decoded with; a segment that was emptied (zero length, blank text) then
    keeps no words"""
    from . import timing

    results = [t[0] for t in to_align]
    kept = [t[1] for t in to_align]
    segs = [[{"tokens": toks} for toks in t[5]] for t in to_align]  # stand-ins that still hold their tokens
    sizes = [t[2] for t in to_align]
    offsets = [t[3] for t in to_align]
    langs = [t[4] for t in to_align]
    if align_fn is not None:
        timing.add_word_timestamps(segs, None, tok, None, sizes, offsets, prepend_punctuations, append_punctuations,
                                   align_fn=lambda text_tokens, _features, num_frames: align_fn(results, text_tokens, num_frames, langs))
        _keep_words(kept, segs)
        return
    import torch

    from .tokenizer import get_tokenizer

    # the sot_sequence names the language: windows are aligned per language, each group in one call
    for lang in sorted(set(langs), key=lambda l: l or ""):
        rows = [j for j, l in enumerate(langs) if l == lang]
        ltok = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=lang or "en", task="transcribe")
        feats = torch.stack([results[j].audio_features for j in rows])
        timing.add_word_timestamps([segs[j] for j in rows], model, ltok, feats, [sizes[j] for j in rows], [offsets[j] for j in rows],
                                   prepend_punctuations, append_punctuations)
    _keep_words(kept, segs)


def _keep_words(kept, segs) -> None:
    for window, stand_ins in zip(kept, segs):
        for seg, stand_in in zip(window, stand_ins):
            seg["words"] = stand_in["words"] if seg["tokens"] or not stand_in["tokens"] else []


def _needs_fallback(res, compression_ratio_threshold, logprob_threshold, no_speech_threshold) -> bool:
    """upstream's decode_with_fallback predicate on one decoded window"""
    needs_fallback = False
    if compression_ratio_threshold is not None and res.compression_ratio > compression_ratio_threshold:
        needs_fallback = True  # too repetitive
    if logprob_threshold is not None and res.avg_logprob < logprob_threshold:
        needs_fallback = True  # average log-probability too low
    if no_speech_threshold is not None and res.no_speech_prob > no_speech_threshold and logprob_threshold is not None \
            and res.avg_logprob < logprob_threshold:
        needs_fallback = False  # silence
    return needs_fallback


def _window_samples(clip: np.ndarray, seek: int, size: int) -> np.ndarray:
    """pad_or_trim of the window's own samples: ``size`` content frames from mel frame ``seek`` on, zero-padded to 30 s"""
    out = np.zeros(N_SAMPLES, dtype=np.float32)
    s0 = seek * HOP_LENGTH
    chunk = clip[s0:s0 + size * HOP_LENGTH]
    out[:len(chunk)] = chunk
    return out


def _last_tokens(history: Sequence[int], budget: int) -> List[int]:
    """the last ``budget`` tokens of a history (``history[-0:]`` would be all of it)"""
    return [int(t) for t in history[-budget:]] if budget > 0 else []


# ---------------------------------------------------------------- schedule="continuous"
def _refuse_continuous(model, seed, word_timestamps, condition_on_previous_text, initial_prompt, best_of, decode_fn, stream_fn=None) -> None:
    """what ``schedule="continuous"`` does not serve, each refused by the option's name before anything is decoded"""
    def no(name, why):
        raise NotImplementedError(f"transcribe(schedule='continuous'): {name} is not implemented ({why}); use schedule='rounds'")

    if seed is not None and stream_fn is not None and not getattr(stream_fn, "retries", False):
        no("seed", "the retries hand a window out again with a temperature, an attempt and a stream of its own; a custom stream_fn that "
                   "serves them declares stream_fn.retries = True, as a custom decode_fn brings a fallback_fn")
    if word_timestamps:
        no("word_timestamps", "the alignment runs on a round's windows")
    # prompts: the model's own stream serves them (a prompt per row in front of its admission column); a custom stream_fn that does
    # declares stream_fn.prompts = True and takes source.pending() entries of (clip, limit, draw, prompt) -- the pattern of `retries`
    if stream_fn is not None and not getattr(stream_fn, "prompts", False):
        if condition_on_previous_text:
            no("condition_on_previous_text", "every window is handed out with its file's prompt; a custom stream_fn that serves prompts "
                                             "declares stream_fn.prompts = True")
        if initial_prompt is not None:
            no("initial_prompt", "every window is handed out with its file's prompt; a custom stream_fn that serves prompts declares "
                                 "stream_fn.prompts = True")
    if best_of is not None:
        no("best_of", "candidate groups are drawn by the retries")
    if decode_fn is not None:
        no("decode_fn", "a custom decoder decodes whole batches; the continuous schedule's seam is stream_fn")
    if getattr(model, "_fp8", None):
        no("an fp8-quantised model", "the continuous step runs on bf16 / f32 decoder tables")


@dataclass
class StreamStats:
    """what a ``schedule="continuous"`` run did"""
    schedule: object = None                                   # what the stream returned: the run's continuous.ScheduleStats
    rows: int = 0                                             # rows of the decode state: min(slots, files)
    waited: List[int] = field(default_factory=list)           # the files that queued for a slot, in the order they got one
    groups: List[List[Tuple[int, int]]] = field(default_factory=list)     # per admitted group: its FRESH windows (file, seek)
    detected: List[List[Tuple[int, int]]] = field(default_factory=list)   # per detect_language call: the windows it looked at
    retries: List[Tuple[int, int, int]] = field(default_factory=list)     # (file, seek, attempt) of every retry, in the order they became pending
    prompt_budget: Optional[int] = None                       # conditioning: the history tokens a window's prompt keeps, counted from the end
    prompts: List[Tuple[int, int, int, int]] = field(default_factory=list)  # conditioning: (file, seek, history tokens, of which kept) per hand-out


@dataclass
class _WindowResult:
    tokens: List[int]
    avg_logprob: float
    no_speech_prob: float
    compression_ratio: float
    temperature: float
    language: Optional[str]


class _WindowSource:
    """``continuous.run_stream``'s source over the files of one ``transcribe`` call.  A file is a stream of windows with at most one in
    flight: its next window, the clip ``(file, seek)``, exists once the previous one has retired and ``books`` knows the seek.  Files
    take a place in input order, at most ``slots`` of them at a time, and keep it until their last window has retired; the others wait.
    ``temps`` and ``seed``: the temperature fallback.  ``pending`` then returns (clip, limit, draw) -- draw None for a window's first
    attempt, (temps[attempt], attempt, (seek, file)) for a retry -- and a window that fails the thresholds with temperatures left is not
    booked: the same clip becomes pending again.  ``on_booked(clip)``, when the stream sets it, hears of every window that is booked.
    ``prompt_budget`` (None: no conditioning): ``pending`` returns (clip, limit, draw, prompt) with the window's prompt columns --
    ``[sot_prev]`` + the last ``prompt_budget`` tokens of the file's ``all_tokens[prompt_reset_since:]``, what the rounds loop hands to
    ``decode(prompts=)``; empty without history.  A file has one window in flight and a failed attempt books nothing, so a retry is
    handed out with the prompt of its first attempt."""

    def __init__(self, clips, content_frames, books: _Books, slots: int, limit: int, stats: StreamStats, temps=(0.0,), seed=None,
                 prompt_budget: Optional[int] = None):
        self.clips, self.content_frames, self.books, self.limit, self.stats = clips, content_frames, books, int(limit), stats
        self.prompt_budget = prompt_budget
        self.temps, self.seed = tuple(float(t) for t in temps), seed
        self.attempt = {}              # file -> index in temps of its window in flight
        self.on_booked = None
        self.slots = int(slots)
        self.waiting = deque(i for i in range(len(clips)) if content_frames[i] > 0)
        self.active: List[int] = []    # files that hold a place, in the order they got it
        self.ready: List[int] = []     # active files whose next window has not been handed out
        self.size = {}                 # (file, seek) -> content frames of the window in flight
        self.first = True

    def pending(self):
        while self.waiting and len(self.active) < self.slots:
            i = self.waiting.popleft()
            self.active.append(i)
            self.ready.append(i)
            if not self.first:
                self.stats.waited.append(i)
        self.first = False
        out = []
        for i in self.ready:
            clip = (i, self.books.seek[i])
            self.size[clip] = min(N_FRAMES, self.content_frames[i] - self.books.seek[i])
            attempt = self.attempt.setdefault(i, 0)
            # the rounds schedule's retry: stream (seek, file index), the index in the schedule
            draw = (self.temps[attempt], attempt, (clip[1], i)) if self.seed is not None and attempt else None
            if self.prompt_budget is not None:
                history = self.books.all_tokens[i][self.books.prompt_reset_since[i]:]
                kept = _last_tokens(history, self.prompt_budget)
                self.stats.prompts.append((i, clip[1], len(history), len(kept)))
                out.append((clip, self.limit, draw, ([int(self.books.tok.sot_prev)] + kept) if kept else []))
            elif self.seed is None:
                out.append((clip, self.limit))
            else:
                out.append((clip, self.limit, draw))
        self.ready = []
        return out

    def group(self, clips):
        """the windows of one admitted group: (samples [n, 480000] f32, the files' languages, None where still unknown)"""
        self.stats.groups.append([tuple(c) for c in clips])
        windows = np.stack([_window_samples(self.clips[i], at, self.size[(i, at)]) for i, at in clips])
        return windows, [self.books.languages[i] for i, _ in clips]

    def detected(self, clips, languages):
        """the one detect_language call of a group told the languages of these windows' files"""
        self.stats.detected.append([tuple(c) for c in clips])
        for (i, _), lang in zip(clips, languages):
            self.books.languages[i] = lang

    def retired(self, clip, tokens, sum_logprob, no_speech):
        i, at = clip
        assert at == self.books.seek[i], "a file has one window in flight"
        from .decoding import compression_ratio

        tok = self.books.tok
        tokens = [int(t) for t in tokens]
        text = tok.decode([t for t in tokens if t < self.books.tb]).strip()
        comp = compression_ratio(text)
        attempt = self.attempt.get(i, 0)
        res = _WindowResult(tokens, float(sum_logprob) / (len(tokens) + 1), float(no_speech), comp, self.temps[attempt], self.books.languages[i])
        books = self.books
        if self.seed is not None and attempt + 1 < len(self.temps) and _needs_fallback(
                res, books.compression_ratio_threshold, books.logprob_threshold, books.no_speech_threshold):
            self.attempt[i] = attempt + 1  # not booked: the file keeps its place and the same window is pending again
            self.stats.retries.append((i, at, attempt + 1))
            self.ready.append(i)
            return
        self.attempt[i] = 0
        self.books.window(i, self.size.pop(clip), res, attempt > 0)  # upstream's "the last attempt is kept"
        if self.on_booked is not None:
            self.on_booked(clip)
        if self.books.seek[i] < self.content_frames[i]:
            self.ready.append(i)
        else:
            self.active.remove(i)


def continuous_prompt_budget(n_text_ctx: int, n_init: int, sample_len: int, check_every: int) -> int:
    """the most history tokens a window's prompt can keep on the continuous schedule: upstream's ``n_ctx // 2 - 1``, and what the column
    window leaves in front of a row that generates ``sample_len`` tokens -- a live row spans ``prompt_room + n_init + sample_len +
    2 * check_every - 1`` columns with ``prompt_room`` = budget + 1 (the ``sot_prev``), at most the default column limit.  With the
    defaults (448, 3, 224, 8) that is 196 tokens against upstream's 223; a ``sample_len`` of 197 or less restores 223."""
    from .continuous import default_column_limit

    return max(min(n_text_ctx // 2 - 1, default_column_limit(n_text_ctx, n_init, check_every) - n_init - int(sample_len) - 2 * check_every), 0)


def _transcribe_continuous(model, clips, content_frames, books: _Books, language, decode_options, stream_fn, slots: int,
                           check_every: int, temps=(0.0,), seed=None, conditioning: bool = False,
                           prompt_budget: Optional[int] = None) -> StreamStats:
    """``transcribe(schedule="continuous")``: every window of every file through min(slots, files) rows of one decode state.  The windows
    that become ready at the same check form one group: one log-mel call from the windows' own samples, one encoder call, one
    detect_language call for the windows of files whose language is still unknown, one admission."""
    if slots < 1 or check_every < 1:
        raise ValueError(f"transcribe: slots = {slots} and check_every = {check_every} must be positive")
    stats = StreamStats(rows=max(min(int(slots), len(clips)), 1))
    n_text_ctx = model.dims.n_text_ctx if model is not None else 448
    limit = decode_options.get("sample_len") or n_text_ctx // 2
    budget = None
    if conditioning:
        largest = continuous_prompt_budget(n_text_ctx, len(books.tok.sot_sequence), limit, check_every)
        budget = largest if prompt_budget is None else int(prompt_budget)
        if not 0 <= budget <= largest:
            raise ValueError(f"transcribe(schedule='continuous'): prompt_budget = {budget} outside 0 .. {largest} (n_text_ctx // 2 - 1, and what "
                             f"the column window leaves in front of sample_len = {limit} tokens at check_every = {check_every})")
        stats.prompt_budget = budget
    source = _WindowSource(clips, content_frames, books, stats.rows, limit, stats, temps, seed, prompt_budget=budget)
    more = {"prompt_room": budget + 1} if conditioning else {}  # the sot_prev in front of the history
    if stream_fn is None:
        from .continuous import stream_windows

        def stream_fn(source, slots, check_every, **kw):
            return stream_windows(model, source, {**decode_options, "language": language}, slots=slots, check_every=check_every, seed=seed, **kw)

    stats.schedule = stream_fn(source, slots=stats.rows, check_every=check_every, **more)
    return stats


class _Books:
    """The per-file state of a ``transcribe`` call and the bookkeeping of ONE decoded window, which both schedules share: the no-speech
    skip, ``split_segments``, the seek advance, the segment dicts, ``needs_fallback`` and upstream's prompt bookkeeping."""

    def __init__(self, tok, n: int, language, initial_ids, thresholds, condition_on_previous_text: bool):
        self.tok, self.tb = tok, int(tok.timestamp_begin)
        self.compression_ratio_threshold, self.logprob_threshold, self.no_speech_threshold = thresholds
        self.condition_on_previous_text = condition_on_previous_text
        self.seek = [0] * n
        self.languages: List[Optional[str]] = [language] * n
        self.all_segments: List[List[dict]] = [[] for _ in range(n)]
        # upstream's prompt bookkeeping, per file: all_tokens starts with the initial prompt, the next window's prompt is what came after
        # prompt_reset_since
        self.all_tokens: List[List[int]] = [list(initial_ids) for _ in range(n)]
        self.prompt_reset_since = [0] * n
        self.warned = False

    def window(self, i: int, size: int, res, retried: bool):
        """file i's window of ``size`` content frames at ``seek[i]`` was decoded to ``res``.  Returns None for a skipped window, else
        (the window's new segments, its time offset, the segments' decoded tokens) -- what the word alignment needs"""
        tok = self.tok
        if self.languages[i] is None:
            self.languages[i] = res.language  # detected on the file's first window, kept for the rest
        time_offset = self.seek[i] * HOP_LENGTH / SAMPLE_RATE
        tokens = [int(t) for t in res.tokens]
        if self.no_speech_threshold is not None:
            skip = res.no_speech_prob > self.no_speech_threshold
            if self.logprob_threshold is not None and res.avg_logprob > self.logprob_threshold:
                skip = False  # a confident transcript overrides the no-speech probability
            if skip:
                self.seek[i] += size
                return None
        needs_fallback = not retried and _needs_fallback(res, self.compression_ratio_threshold, self.logprob_threshold, self.no_speech_threshold)
        if needs_fallback and not self.warned:
            warnings.warn("whisper_ipa_amd.transcribe: a window failed compression_ratio_threshold / logprob_threshold; upstream would "
                          "retry at a higher temperature, this path runs temperature 0 only (segments carry needs_fallback=True)",
                          RuntimeWarning, stacklevel=3)
            self.warned = True
        at = self.seek[i]
        segs, advance = split_segments(tokens, self.tb, time_offset, size)
        self.seek[i] += advance
        first_new = len(self.all_segments[i])
        decoded_tokens = [list(sg["tokens"]) for sg in segs]  # the alignment sees what was decoded, emptied segments included
        for sg in segs:
            text = tok.decode([t for t in sg["tokens"] if t < tok.eot])
            if sg["start"] == sg["end"] or text.strip() == "":
                text, sg["tokens"] = "", []
            seg = {"id": len(self.all_segments[i]), "seek": at, "start": sg["start"], "end": sg["end"], "text": text, "tokens": sg["tokens"],
                   "temperature": res.temperature, "avg_logprob": res.avg_logprob, "compression_ratio": res.compression_ratio,
                   "no_speech_prob": res.no_speech_prob}
            if needs_fallback:
                seg["needs_fallback"] = True
            self.all_segments[i].append(seg)
            self.all_tokens[i].extend(sg["tokens"])
        if not self.condition_on_previous_text or res.temperature > 0.5:
            self.prompt_reset_since[i] = len(self.all_tokens[i])  # do not feed the prompt tokens if a high temperature was used
        if advance <= 0:  # a pair at <|0.00|> only: never stand still
            self.seek[i] += size
        return self.all_segments[i][first_new:], time_offset, decoded_tokens


def transcribe(model, audio, *, verbose: Optional[bool] = None, temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
               compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
               no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = False,
               initial_prompt: Optional[str] = None, word_timestamps: bool = False, clip_timestamps=None,
               hallucination_silence_threshold: Optional[float] = None, language: Optional[str] = None, decode_fn: Optional[Callable] = None,
               tokenizer=None, seed: Optional[int] = None, fallback_fn: Optional[Callable] = None,
               prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
               align_fn: Optional[Callable] = None, schedule: str = "rounds", slots: int = 64, check_every: int = 8,
               stream_fn: Optional[Callable] = None, stats_out: Optional[list] = None, prompt_budget: Optional[int] = None,
               **decode_options):
    """``audio``: a path, a 16 kHz mono float array, or a list of them.  Returns {"text", "segments", "language"} (a list of
    them for a list) with mlx_whisper's segment keys (``SEGMENT_KEYS``; plus ``needs_fallback`` where upstream would have
    retried).  ``condition_on_previous_text`` defaults to False here.  With True every window after a file's first is decoded with
    the file's previous tokens (timestamps included) as its prompt, ``<|startofprev|> ... <|startoftranscript|> ...``, until a window
    decoded above temperature 0.5 resets it; ``initial_prompt`` is the prompt of the first window (of every window until such a reset
    with conditioning on) and is left out of the returned ``text``.  ``decode_fn`` is then called as ``decode_fn(windows, languages,
    prompts=[ids per row])`` and ``fallback_fn`` gets ``prompts=`` too; a custom one without that parameter is refused.
    ``decode_fn(windows [n, 480000] f32, languages [n])`` -> objects with tokens / avg_logprob / no_speech_prob /
    compression_ratio / temperature / language replaces the model's decode (tests; ``tokenizer`` is then required when
    ``model`` is None).  ``seed``: run the temperature schedule (module docstring); segments then carry the temperature that
    produced them, and neither ``needs_fallback`` nor the warning appears where a retry ran.  ``fallback_fn(results, languages,
    temperature=, attempt=, streams=, seed=)`` -> new results for those rows replaces the model's retry; with a custom ``decode_fn``
    and no ``fallback_fn`` a seed changes nothing.  ``streams[j]`` = (seek in mel frames, file index), ``attempt`` = index in the
    schedule.  ``beam_size=N`` (with ``patience=``, ``length_penalty=``; rounds schedule): the temperature-0 decode of every window is a
    beam search (decoding.py); the retries above 0 drop ``beam_size`` / ``patience``, as upstream's ``decode_with_fallback`` does, and go on
    as without beams, with ``best_of`` if given.  A custom ``decode_fn`` serves beams when it has a true ``beams`` attribute.  Refused by
    name with beams: ``schedule="continuous"``, ``condition_on_previous_text`` / ``initial_prompt``, ``word_timestamps``.
    ``best_of=N``: every retry decodes N candidates per window and keeps the best (``fallback_fn`` then gets ``best_of=N``).  ``word_timestamps=True``: every segment gains ``"words"``: [{"word", "start", "end", "probability"}]
    (timing.py); ``align_fn(results, text_tokens, num_frames, languages)`` -> one list of WordTiming per window replaces the
    model's alignment (``results``: the windows' decode results, ``text_tokens[j]`` the ids below EOT of window j's segments,
    ``num_frames[j]`` its content in mel frames); it is required with a custom ``decode_fn``.
    ``schedule="continuous"``: the windows go through ``slots`` rows of ONE decode state with refill instead of one lockstep batch per
    round (``_transcribe_continuous``); the host looks at the rows every ``check_every`` steps.  ``seed`` runs the temperature schedule
    there too (a retried window is pending again with its own temperature; module docstring).  ``condition_on_previous_text`` /
    ``initial_prompt`` are served there as on the rounds schedule: a window is handed out with its file's prompt, which stands in front
    of the window's admission column and goes through one batched pass at the admission.  ``word_timestamps``,
    ``best_of``, a custom ``decode_fn`` and fp8 models are refused.
    ``stream_fn(source, slots=, check_every=)`` replaces the model's continuous decoder (tests); with a seed it must declare
    ``stream_fn.retries = True`` and take ``source.pending()`` entries of (clip, limit, draw); with conditioning it must declare
    ``stream_fn.prompts = True``, take entries of (clip, limit, draw, prompt) and a ``prompt_room=`` keyword.  ``stats_out``: a list
    that receives the run's ``StreamStats``.
    ``prompt_budget`` (both schedules, with conditioning): the history tokens a window's prompt keeps, counted as the last ones.  None
    on ``rounds`` is upstream's ``n_text_ctx // 2 - 1`` = 223.  None on ``continuous`` is the largest budget that fits the column window,
    ``min(n_text_ctx // 2 - 1, column_limit - n_init - sample_len - 2 * check_every)``: with the defaults that is 196 tokens against
    upstream's 223 at ``sample_len`` 224 (``continuous_prompt_budget``); a smaller ``sample_len`` restores 223.  So with the defaults
    the two schedules condition a window that has more than 196 tokens of history on different prompts; an explicit ``prompt_budget``
    of at most 196 gives both the same.
    A model with ``audio_ctx`` set is refused: the window loop, the seek arithmetic and the timestamp range assume 30 s windows."""
    if getattr(model, "audio_ctx", None) is not None:
        raise NotImplementedError(f"transcribe() on a model with audio_ctx={model.audio_ctx} is not implemented: its window loop, seek "
                                  "arithmetic and timestamp range assume 30 s windows; decode() / decode_continuous() serve audio_ctx")
    # an adapter of the model's bank per FILE: every window of a file carries it, and retries and conditioning keep it
    file_adapters = decode_options.pop("row_adapters", None)
    if file_adapters is not None:
        if model is None or decode_fn is not None or getattr(model, "adapter_bank", None) is None:
            raise NotImplementedError("transcribe(row_adapters=...) is served by the model's own decoder on a model with an adapter bank "
                                      "(Whisper.set_adapter_bank); a custom decode_fn takes no row_adapters")
        if schedule == "continuous":
            raise NotImplementedError("transcribe(schedule='continuous'): row_adapters is not implemented (its window source hands out no "
                                      "adapter with a window yet); use schedule='rounds'")
        if word_timestamps:
            raise NotImplementedError("word_timestamps=True with row_adapters is not implemented: the alignment pass takes no adapter bank")
        file_adapters = list(file_adapters)
        model.adapter_bank.ids(file_adapters)  # an unknown name is refused before anything is decoded
    _refuse(condition_on_previous_text, initial_prompt, word_timestamps, clip_timestamps, hallucination_silence_threshold, temperature,
            decode_options, can_align=align_fn is not None or (model is not None and decode_fn is None),
            can_retry=decode_fn is None or fallback_fn is not None,
            can_beam=(decode_fn is None and model is not None) or bool(getattr(decode_fn, "beams", False)))
    _refuse_conditioning(condition_on_previous_text, initial_prompt, model, decode_fn, fallback_fn)
    conditioning = bool(condition_on_previous_text) or initial_prompt is not None
    if prompt_budget is not None and (int(prompt_budget) < 0 or not conditioning):
        raise ValueError(f"transcribe: prompt_budget = {prompt_budget} must not be negative and comes with condition_on_previous_text=True or "
                         "an initial_prompt")
    if word_timestamps and align_fn is None and getattr(model, "_fp8", None):
        raise NotImplementedError("word_timestamps=True is not implemented for an fp8-quantised model: the alignment runs the "
                                  "teacher-forced decoder on bf16 / f32 weights")
    single = not isinstance(audio, (list, tuple))
    items = [audio] if single else list(audio)
    clips = []
    for a in items:
        if isinstance(a, str):
            from .audio import load_audio

            a = load_audio(a)
        a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"transcribe: audio is a path or a mono sample array, got shape {a.shape}")
        clips.append(a)
    if tokenizer is None:
        from .tokenizer import get_tokenizer

        tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language or "en", task="transcribe")
    tok, tb = tokenizer, int(tokenizer.timestamp_begin)
    temps = (float(temperature),) if isinstance(temperature, (int, float)) else tuple(float(t) for t in temperature)
    # upstream's decode_with_fallback: best_of belongs to the temperatures above 0 -- the first decode never sees it, every retry does
    best_of = decode_options.pop("best_of", None)
    if schedule not in ("rounds", "continuous"):
        raise ValueError(f"transcribe: schedule is 'rounds' or 'continuous', got {schedule!r}")
    if schedule == "continuous" and decode_options.get("beam_size") is not None:
        raise NotImplementedError("transcribe(schedule='continuous'): beam_size is not implemented (the slots of the continuous schedule "
                                  "are single rows); use schedule='rounds'")
    if schedule == "continuous":
        _refuse_continuous(model, seed, word_timestamps, condition_on_previous_text, initial_prompt, best_of, decode_fn, stream_fn)
    elif decode_fn is None:
        decode_fn = _model_decoder(model, decode_options)
        fallback_fn = fallback_fn or decode_fn.retry
    if seed is None:
        fallback_fn = None  # as ever: the flag and the warning

    n = len(clips)
    if file_adapters is not None and len(file_adapters) != n:
        raise ValueError(f"transcribe: row_adapters holds {len(file_adapters)} names for {n} files")
    content_frames = [len(a) // HOP_LENGTH for a in clips]
    initial_ids = [int(t) for t in tok.encode(" " + initial_prompt.strip())] if initial_prompt is not None else []
    books = _Books(tok, n, language, initial_ids, (compression_ratio_threshold, logprob_threshold, no_speech_threshold),
                   bool(condition_on_previous_text))
    seek, languages, all_segments, all_tokens, prompt_reset_since = (books.seek, books.languages, books.all_segments, books.all_tokens,
                                                                     books.prompt_reset_since)
    if schedule == "continuous":
        stats = _transcribe_continuous(model, clips, content_frames, books, language, decode_options, stream_fn, slots, check_every, temps, seed,
                                       conditioning=conditioning, prompt_budget=prompt_budget)
        if stats_out is not None:
            stats_out.append(stats)
    while schedule == "rounds":
        live = [i for i in range(n) if seek[i] < content_frames[i]]
        if not live:
            break
        # one batch per round: the next window of every file still in progress
        sizes = [min(N_FRAMES, content_frames[i] - seek[i]) for i in live]
        windows = np.zeros((len(live), N_SAMPLES), dtype=np.float32)
        for r, (i, size) in enumerate(zip(live, sizes)):
            windows[r] = _window_samples(clips[i], seek[i], size)
        prompts = [list(all_tokens[i][prompt_reset_since[i]:]) for i in live] if conditioning else None
        if conditioning and prompt_budget is not None:  # None: decode() keeps upstream's last n_text_ctx // 2 - 1
            prompts = [_last_tokens(p, int(prompt_budget)) for p in prompts]
        adapters = {"row_adapters": [file_adapters[i] for i in live]} if file_adapters is not None else {}
        if conditioning:
            results = list(decode_fn(windows, [languages[i] for i in live], prompts=prompts, **adapters))
        else:
            results = list(decode_fn(windows, [languages[i] for i in live], **adapters))
        to_align = []  # (result, the window's segments, content frames, time offset, language, the segments' decoded tokens): rows not skipped
        retried = set()  # rows of this round that went through the schedule
        if fallback_fn is not None:
            thresholds = (compression_ratio_threshold, logprob_threshold, no_speech_threshold)
            failing = [r for r in range(len(live)) if _needs_fallback(results[r], *thresholds)]
            for attempt in range(1, len(temps)):
                if not failing:
                    break
                # the failing rows of the round as ONE sub-batch; the language is the file's, or what this window's first decode detected
                more = {"prompts": [prompts[r] for r in failing]} if conditioning else {}  # the retry keeps the window's prompt
                if best_of is not None:
                    more["best_of"] = best_of
                if file_adapters is not None:
                    more["row_adapters"] = [file_adapters[live[r]] for r in failing]
                again = fallback_fn([results[r] for r in failing], [languages[live[r]] or results[r].language for r in failing],
                                    temperature=temps[attempt], attempt=attempt, streams=[(seek[live[r]], live[r]) for r in failing], seed=seed,
                                    **more)
                for r, res in zip(failing, again):
                    results[r] = res
                retried.update(failing)
                failing = [r for r in failing if _needs_fallback(results[r], *thresholds)]
        for row, (i, size, res) in enumerate(zip(live, sizes, results)):
            booked = books.window(i, size, res, row in retried)
            if booked is not None and word_timestamps:
                new_segments, time_offset, decoded_tokens = booked
                to_align.append((res, new_segments, size, time_offset, languages[i], decoded_tokens))
        if word_timestamps and to_align:
            _add_words(model, tok, to_align, prepend_punctuations, append_punctuations, align_fn)
    out = [{"text": tok.decode([t for t in all_tokens[i][len(initial_ids):] if t < tb]), "segments": all_segments[i], "language": languages[i]} for i in range(n)]
    return out[0] if single else out
