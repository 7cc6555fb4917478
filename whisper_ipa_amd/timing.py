"""Word timestamps: openai-whisper's timing.py (``find_alignment``, ``merge_punctuations``, ``add_word_timestamps``), which
mlx_whisper ports ([UPSTREAM-UNVERIFIED]: neither is at hand, the algorithm is restated from memory and its numeric core is
pinned to the local transformers copy of the same chain, tests/golden/alignment.npz).

The text tokens of a window go through ONE teacher-forced decoder pass (``wipa_decoder_align``, csrc/runtime.hip) that keeps the
cross-attention scores of the alignment heads: softmax over the window's own frames, z-score over the tokens, width-7 median
filter, mean over heads (csrc/align.hip), then dynamic time warping of the negated matrix on the GPU, one wave per window.  The
host only cuts the path into words: ``Tokenizer.split_to_word_tokens``, the jumps of the text index, the mean token
probability per word.

What differs from upstream, on purpose:
  * ``find_alignment`` is batched over windows and starts from the encoder output (``DecodingResult.audio_features``), not from
    the mel: ``transcribe`` aligns all windows of a round in one call, without a second log-mel or encoder pass;
  * upstream's duration heuristics are left out: the median / maximum word-duration clamps at sentence boundaries, the snapping
    of segment starts and ends to their first and last word, and moving ``seek`` to the end of the last word;
  * ``hallucination_silence_threshold`` is left out (still refused by ``transcribe``);
  * an fp8-quantised model is refused: the teacher-forced pass runs on bf16 / f32 weights.
  The two heuristics are unpinned recollections with nothing here to check them against; they wait for a recorded upstream fixture.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

TIME_PER_FRAME = 0.02  # seconds per encoder frame (tokens_per_second = 50)
PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"


@dataclass
class WordTiming:
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: float


def words_from_path(tokenizer, text_tokens: Sequence[int], text_indices, time_indices, token_probs) -> List[WordTiming]:
    """steps 7 and 8 of find_alignment for one window: the DTW path over rows = (text_tokens + [eot]) and ``token_probs[k]`` =
    probability of text_tokens[k] -> one WordTiming per word of split_to_word_tokens(text_tokens + [eot]) but the last (eot)"""
    text_tokens = [int(t) for t in text_tokens]
    if len(text_tokens) == 0:
        return []
    words, word_tokens = tokenizer.split_to_word_tokens(text_tokens + [tokenizer.eot])
    if len(word_tokens) <= 1:
        return []
    word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    text_indices, time_indices = np.asarray(text_indices), np.asarray(time_indices)
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = time_indices[jumps] * TIME_PER_FRAME
    start_times = jump_times[word_boundaries[:-1]]
    end_times = jump_times[word_boundaries[1:]]
    probs = np.asarray(token_probs, dtype=np.float64)
    word_probabilities = [float(np.mean(probs[i:j])) for i, j in zip(word_boundaries[:-1], word_boundaries[1:])]
    return [WordTiming(w, list(t), float(s), float(e), p)
            for w, t, s, e, p in zip(words, word_tokens, start_times, end_times, word_probabilities)]


def align_tokens(model, tokens_rows: Sequence[Sequence[int]], n_rows: Sequence[int], first_row: int, eot: int, features,
                 n_frames: Sequence[int], logits_rows: int = 0):
    """The device part on explicit token rows: ``tokens_rows[b]`` = [*sot_sequence, no_timestamps, *text, eot]; clip b's DTW runs on
    rows [first_row, first_row + n_rows[b]) and frames [0, n_frames[b]).  Returns (matrix [B, T, n_audio_ctx] f32 tensor on the
    device, [(text_indices, time_indices) numpy per clip], token_probs [B, T] numpy: entry (b, t) is the probability of
    tokens_rows[b][t + 1] under a softmax over the ids below ``eot``)."""
    import torch

    from . import _lib
    from .runtime import on_stream, ptr, sptr

    if getattr(model, "_fp8", None):
        raise NotImplementedError("word timestamps run the teacher-forced decoder on bf16 / f32 weights: not implemented for an fp8-quantised model")
    L = _lib.lib()
    pk = model.packed(teacher_forced=True, absorbed=False)
    dims, n_ctx = model.dims, model.n_audio_ctx  # the positions the model runs on (model.audio_ctx): n_frames is clipped to them
    B = len(tokens_rows)
    T = max(len(r) for r in tokens_rows)
    if T > dims.n_text_ctx:
        raise ValueError(f"align: {T} tokens exceed n_text_ctx = {dims.n_text_ctx}")
    heads = list(model.alignment_heads)
    tok = np.full((B, T), int(eot), dtype=np.int32)
    for b, r in enumerate(tokens_rows):
        tok[b, :len(r)] = np.asarray(r, dtype=np.int32)
    n_tok = np.array([len(r) for r in tokens_rows], dtype=np.int32)
    n_fr = np.clip(np.asarray(n_frames, dtype=np.int32), 1, n_ctx).astype(np.int32)
    n_row = np.asarray(n_rows, dtype=np.int32)
    heads_arr = np.asarray(heads, dtype=np.int32).reshape(-1)
    ld_path = T + n_ctx
    with on_stream() as s:
        dev = model.device
        d_tok = torch.from_numpy(tok).to(dev)
        d_sizes = torch.from_numpy(np.stack([n_tok, n_fr, n_row])).to(dev)
        feats = features.to(device=dev, dtype=model.dtype).contiguous()
        if tuple(feats.shape) != (B, n_ctx, dims.n_text_state):
            raise _lib.WipaError(f"align: audio features of shape {tuple(feats.shape)}, expected {(B, n_ctx, dims.n_text_state)} "
                                 f"(audio_ctx={model.audio_ctx!r})")
        need = L.wipa_decoder_align_workspace_bytes(C.byref(pk["cfg"]), B, T, len(heads), int(logits_rows))
        # the pass buffers and up to 1 GiB of logits block: the call's own, back in torch's pool when it returns
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        matrix = torch.empty(B, T, n_ctx, dtype=torch.float32, device=dev)
        path = torch.zeros(2, B, ld_path, dtype=torch.int32, device=dev)
        path_len = torch.zeros(B, dtype=torch.int32, device=dev)
        probs = torch.zeros(B, T, dtype=torch.float32, device=dev)
        i32p = C.POINTER(C.c_int32)
        _lib.check(L.wipa_decoder_align(C.byref(pk["cfg"]), pk["dec_tab"], ptr(d_tok), ptr(feats), heads_arr.ctypes.data_as(i32p), len(heads),
                                        ptr(d_sizes[0]), ptr(d_sizes[1]), ptr(d_sizes[2]), n_tok.ctypes.data_as(i32p),
                                        n_fr.ctypes.data_as(i32p), n_row.ctypes.data_as(i32p), int(first_row), int(eot), ptr(matrix),
                                        ptr(path[0]), ptr(path[1]), ld_path, ptr(path_len), ptr(probs), int(logits_rows), ptr(ws), ws.numel(),
                                        B, T, sptr(s)), "wipa_decoder_align")
        path_h, len_h, probs_h = path.cpu().numpy(), path_len.cpu().numpy(), probs.cpu().numpy()
    paths = [(path_h[0, b, :len_h[b]].astype(np.int64), path_h[1, b, :len_h[b]].astype(np.int64)) for b in range(B)]
    return matrix, paths, probs_h


def find_alignment(model, tokenizer, text_tokens: Sequence[Sequence[int]], features, num_frames: Sequence[int]) -> List[List[WordTiming]]:
    """upstream's find_alignment, batched: ``text_tokens[b]`` are window b's text tokens (< eot), ``features`` [B, n_audio_ctx, d]
    the windows' encoder outputs, ``num_frames[b]`` the window's content in mel frames.  One list of WordTiming per window, times
    relative to the window's start; a window without text tokens gives []."""
    text_tokens = [[int(t) for t in row] for row in text_tokens]
    if len(text_tokens) == 0:
        return []
    sot = list(tokenizer.sot_sequence)
    rows = [[*sot, tokenizer.no_timestamps, *row, tokenizer.eot] for row in text_tokens]
    n_rows = [len(row) + 1 if row else 0 for row in text_tokens]
    _, paths, probs = align_tokens(model, rows, n_rows, len(sot), tokenizer.eot, features, [int(n) // 2 for n in num_frames])
    out = []
    for b, row in enumerate(text_tokens):
        ti, tj = paths[b]
        out.append(words_from_path(tokenizer, row, ti, tj, probs[b, len(sot):len(sot) + len(row)]))
    return out


def merge_punctuations(alignment: List[WordTiming], prepended: str = PREPEND_PUNCTUATIONS, appended: str = APPEND_PUNCTUATIONS) -> None:
    """in place: a word that is only opening punctuation is glued onto the word after it, closing punctuation onto the word
    before it; the absorbed entries are left empty (no word, no tokens)"""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:  # prepended punctuation: backwards
        previous, following = alignment[i], alignment[j]
        if previous.word.startswith(" ") and previous.word.strip() in prepended:
            following.word = previous.word + following.word
            following.tokens = previous.tokens + following.tokens
            previous.word = ""
            previous.tokens = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):  # appended punctuation: forwards
        previous, following = alignment[i], alignment[j]
        if not previous.word.endswith(" ") and following.word in appended:
            previous.word = previous.word + following.word
            previous.tokens = previous.tokens + following.tokens
            following.word = ""
            following.tokens = []
        else:
            i = j
        j += 1


def deal_words(segments: List[dict], alignment: List[WordTiming], eot: int, time_offset: float) -> None:
    """the words of one window, dealt to its segments by token count (upstream's add_word_timestamps loop): a segment takes words
    until their tokens cover its text tokens.  Each segment gains "words": [{"word", "start", "end", "probability"}]."""
    word_index = 0
    for segment in segments:
        saved_tokens = 0
        words = []
        n_text = len([t for t in segment["tokens"] if t < eot])
        while word_index < len(alignment) and saved_tokens < n_text:
            timing = alignment[word_index]
            if timing.word:
                words.append({"word": timing.word, "start": round(time_offset + timing.start, 2), "end": round(time_offset + timing.end, 2),
                              "probability": timing.probability})
            saved_tokens += len(timing.tokens)
            word_index += 1
        segment["words"] = words


def add_word_timestamps(segments_by_window: List[List[dict]], model, tokenizer, features, num_frames: Sequence[int],
                        time_offsets: Sequence[float], prepend_punctuations: str = PREPEND_PUNCTUATIONS,
                        append_punctuations: str = APPEND_PUNCTUATIONS, align_fn: Optional[Callable] = None) -> None:
    """``segments_by_window[b]``: the segments of window b (dicts with "tokens"); all windows are aligned in ONE find_alignment
    call (``align_fn(text_tokens, features, num_frames)`` replaces it) and every segment gains "words"."""
    if len(segments_by_window) == 0:
        return
    eot = tokenizer.eot
    text_tokens = [[t for seg in segs for t in seg["tokens"] if t < eot] for segs in segments_by_window]
    if align_fn is not None:
        alignments = align_fn(text_tokens, features, list(num_frames))
    else:
        alignments = find_alignment(model, tokenizer, text_tokens, features, num_frames)
    for segs, alignment, offset in zip(segments_by_window, alignments, time_offsets):
        alignment = [WordTiming(w.word, list(w.tokens), w.start, w.end, w.probability) for w in alignment]
        merge_punctuations(alignment, prepend_punctuations, append_punctuations)
        deal_words(segs, alignment, eot, offset)


def align(model, audio, texts, language: str = "en", tokenizer=None) -> List[List[WordTiming]]:
    """Forced alignment of KNOWN transcripts: ``audio`` one clip or a list (paths or 16 kHz mono arrays, each <= 30 s), ``texts``
    the matching transcript(s).  Tokenises, runs log-mel and the encoder, and calls find_alignment; one list of WordTiming per
    clip (after merge_punctuations, emptied entries dropped)."""
    import torch

    from . import audio as A

    single = not isinstance(audio, (list, tuple))
    items = [audio] if single else list(audio)
    text_list = [texts] if isinstance(texts, str) else list(texts)
    if len(items) != len(text_list):
        raise ValueError(f"align: {len(items)} clips but {len(text_list)} transcripts")
    if tokenizer is None:
        from .tokenizer import get_tokenizer

        tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language, task="transcribe")
    windows = np.zeros((len(items), A.N_SAMPLES), dtype=np.float32)
    frames = []
    for r, a in enumerate(items):
        if isinstance(a, str):
            a = A.load_audio(a)
        a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"align: audio is a path or a mono sample array, got shape {a.shape}")
        if len(a) > A.N_SAMPLES:
            raise ValueError(f"align: clip {r} has {len(a) / A.SAMPLE_RATE:.1f} s; forced alignment takes clips of at most 30 s")
        windows[r, :len(a)] = a
        frames.append(len(a) // A.HOP_LENGTH)
    mel = A.log_mel_spectrogram(torch.from_numpy(windows).to(model.device), n_mels=model.dims.n_mels)
    feats = model.embed_audio(mel)
    text_tokens = [tokenizer.encode(t) for t in text_list]
    out = []
    for alignment in find_alignment(model, tokenizer, text_tokens, feats, frames):
        merge_punctuations(alignment)
        out.append([w for w in alignment if w.word])
    return out[0] if single else out
