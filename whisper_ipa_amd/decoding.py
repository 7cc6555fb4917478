"""KV-cached greedy and temperature-sampling decoding with the surface of ``mlx_whisper.decoding`` used by the
reference: ``DecodingOptions``, ``DecodingResult``, ``decode(model, mel_or_features, options)``
(scripts/transcribe_single.py:49-56; scripts/train_whisper_ipa.py:338-362;
scripts/evaluate_model.py:170-201).

The whole loop runs on the GPU: one decoder step is captured into a hipGraph by
csrc/runtime.hip and replayed; token ids, EOT latches and log-prob sums stay in device
memory; the host only looks at the last token column every few steps to stop early.

``temperature > 0`` (upstream's GreedyDecoder.update with a Categorical draw) runs when ``DecodingOptions.seed`` is given: the draw
is a Gumbel-max over counter-based Philox noise in the step's tail (csrc/elementwise.hip: row_pick<.., SAMPLE>), a pure function of
(seed, the row's stream, attempt, position, column) -- reproducible, and independent of the batch a row is decoded in.  Seed,
attempt, 1 / T and the streams live in a small device record the replayed step graph reads; nothing of them is baked into it.

Prompt conditioning (``DecodingOptions.prompt`` / ``prefix`` / ``prompts``; ``transcribe(condition_on_previous_text=True)``): every row's
initial tokens are ``[sot_prev] + history + sot_sequence + prefix`` (upstream's ``_get_initial_tokens``), so the rows of one batch differ
in length.  They are packed RIGHT-ALIGNED to one prompt width P (``pack_prompts``): row b's tokens sit in columns [P - n_b, P), the
columns before them are padding, one position counter serves the batch and generation starts at column P for every row; the device
kernels take the rows' first columns (``starts``) and give every row its own position embeddings, its own attention window and its
own sampling counter (include/wipa.h: wipa_decoder_begin_ragged / wipa_decode_call.starts_dev).  P is the longest row rounded up to a
multiple of 16 where that leaves room to generate.  ONE documented deviation from upstream: ``sample_len`` is clamped to
``n_text_ctx - P`` for the whole batch, so a row with a short prompt decoded next to one with the full 223-token history can generate
448 - 227 = 221 tokens, not 224.  Without any prompt or prefix ``decode`` makes exactly the library calls it made before.

Best-of-N (``DecodingOptions.best_of`` at a temperature above 0; upstream's ``n_group = best_of`` with MaximumLikelihoodRanker): every
clip is decoded as a GROUP of N candidate rows that share the clip's audio -- the decode state holds it once per clip
(``wipa_model_cfg.dec_n_group``) and the features are never replicated.  Candidate k of a row with stream (lo, hi) draws from stream
(lo, hi + (k << 24)), so candidate 0 is the row's draw without ``best_of`` and a window's candidates do not depend on its neighbours.
``wipa_rank_groups`` picks, on the device, the candidate with the highest ``sum_logprobs / penalty(length)`` (first maximum) and the
host reads the winners only.  ONE deviation from upstream: a candidate of length 0 scores -inf where upstream divides by zero.

Beam search (``DecodingOptions.beam_size`` / ``patience`` / ``length_penalty`` at temperature 0; upstream's BeamSearchDecoder with
MaximumLikelihoodRanker): every clip is decoded as a group of ``beam_size`` rows that share its audio, like best-of.  The step's tail
(csrc/beam.hip) takes every row's ``beam_size + 1`` best continuations, keeps per clip the best ``beam_size`` that do not end and moves the
ones that do into the clip's finished store (``round(beam_size * patience)`` sequences); the self-attention cache is never permuted --
a beam reads its history through an ancestor table (csrc/attention.hip, decode_attn_kernel<.., BEAM>).  ``wipa_beam_finalize`` ranks on
the device and the host reads one row per clip.  Not served with beams: prompts / prefixes, a temperature above 0, fp8 decoder tables.
"""
from __future__ import annotations

import os

import ctypes as C
import zlib
from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .runtime import on_stream, ptr, sptr, stream, stream_id
from .tokenizer import Tokenizer, get_tokenizer


@dataclass(frozen=True)
class DecodingOptions:
    task: str = "transcribe"
    language: Optional[str] = None
    temperature: float = 0.0
    sample_len: Optional[int] = None
    best_of: Optional[int] = None
    beam_size: Optional[int] = None
    patience: Optional[float] = None
    length_penalty: Optional[float] = None
    prompt: Optional[Union[str, List[int]]] = None
    prefix: Optional[Union[str, List[int]]] = None
    suppress_tokens: Optional[Union[str, Sequence[int]]] = "-1"
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = True
    prompts: Optional[Sequence[Optional[Sequence[int]]]] = None  # one prompt (token ids, or None) PER ROW: what transcribe's conditioning uses
    row_adapters: Optional[Sequence[Optional[str]]] = None  # one adapter name of the model's bank (Whisper.set_adapter_bank), or None, PER ROW (per clip with best_of)
    seed: Optional[int] = None          # temperature > 0 needs one: sampling is opt-in and reproducible
    sample_streams: Optional[Sequence] = None  # per-row (lo, hi) Philox streams; default (row, 0)
    sample_attempt: int = 0             # which retry of the row this is (transcribe's fallback schedule index)


@dataclass
class DecodingResult:
    audio_features: torch.Tensor
    language: str
    language_probs: Optional[dict] = None
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    avg_logprob: float = float("nan")
    no_speech_prob: float = float("nan")
    temperature: float = float("nan")
    compression_ratio: float = float("nan")


def compression_ratio(text: str) -> float:
    """the text's UTF-8 bytes over their zlib-compressed bytes (the fallback's repetition test); nan for an empty text"""
    raw = text.encode("utf-8")
    return len(raw) / max(len(zlib.compress(raw)), 1) if text else float("nan")


@dataclass
class GreedyTokens:
    tokens: np.ndarray        # [B, n_init + n_steps] int64 (EOT-latched)
    n_steps: int              # generated positions
    sum_logprobs: np.ndarray  # [B]
    last_logits: Optional[torch.Tensor] = None  # [B, V] f32 logits of the last executed step (device)
    n_init: Optional[int] = None               # ragged prompts: the common prompt width P (tokens[:, P:] is what was generated)
    starts: Optional[np.ndarray] = None        # ragged prompts: [B] first own column of every row
    sot_logits: Optional[torch.Tensor] = None  # ragged prompts: [B, V] f32 logits at the rows' <|startoftranscript|> column (device copy)
    winner: Optional[np.ndarray] = None        # ranked candidate groups: [clips] the winning candidate of every clip
    lengths: Optional[np.ndarray] = None       # ranked candidate groups: [clips, G] generated tokens before the first EOT, per candidate


class DecoderState:
    """The caller-owned decode blob of wipa_decoder_* (tokens, position, logits, KV caches)."""

    def __init__(self, model, B: int, pk=None):
        L = _lib.lib()
        self.model, self.B = model, B
        pk = pk or model.packed()
        self.layout = _lib.DecLayout()
        _lib.check(L.wipa_decoder_layout(C.byref(pk["cfg"]), B, C.byref(self.layout)), "wipa_decoder_layout")
        self.layout_key = tuple(getattr(self.layout, f) for f, _ in self.layout._fields_)
        with on_stream():
            self.blob = torch.empty(self.layout.total_bytes, dtype=torch.uint8, device=model.device)

    def _view(self, off: int, nbytes: int, dtype):
        return self.blob[off : off + nbytes].view(dtype)

    @property
    def tokens(self) -> torch.Tensor:
        lay = self.layout
        return self._view(lay.tokens, self.B * lay.ld_tok * 4, torch.int32).view(self.B, lay.ld_tok)

    @property
    def pos(self) -> torch.Tensor:
        return self._view(self.layout.pos, 4, torch.int32)

    @property
    def sum_logprobs(self) -> torch.Tensor:
        return self._view(self.layout.sum_logprobs, self.B * 4, torch.float32)

    @property
    def not_done(self) -> torch.Tensor:
        return self._view(self.layout.not_done, 4, torch.int32)

    def beam_buffer(self, n_group: int, max_candidates: int) -> torch.Tensor:
        """the caller-owned beam buffer of this state (include/wipa.h: wipa_beam_bytes).  Kept, and re-made only to grow: the step graph
        is keyed on its address."""
        need = int(_lib.lib().wipa_beam_bytes(self.B, n_group, max_candidates, self.layout.ld_tok))
        buf = getattr(self, "_beam_buf", None)
        if buf is None or buf.numel() < need:
            stream().synchronize()  # nothing enqueued may still read the old one
            with on_stream():
                self._beam_buf = buf = torch.empty(need, dtype=torch.uint8, device=self.blob.device)
        return buf

    @property
    def logits(self) -> torch.Tensor:
        lay = self.layout
        return self._view(lay.logits, self.B * lay.ld_logits * 4, torch.float32).view(self.B, lay.ld_logits)[:, : self.model.dims.n_vocab]

    def sample_record(self, sample: "Sampling") -> torch.Tensor:
        """the device sampling record of this state (include/wipa.h), rewritten in stream order with ``sample``'s values.  ONE buffer
        per state: the step graph is keyed on its address, so a new seed / temperature / attempt replays the captured graph."""
        L = _lib.lib()
        nbytes = int(L.wipa_sample_record_bytes(self.B))
        streams = sample.streams if sample.streams is not None else [(b, 0) for b in range(self.B)]
        if len(streams) != self.B:
            raise ValueError(f"sample_streams: {len(streams)} streams for {self.B} rows")
        flat = (C.c_uint32 * (2 * self.B))(*[int(v) & 0xFFFFFFFF for pair in streams for v in pair])
        host = np.zeros(nbytes, dtype=np.uint8)
        _lib.check(L.wipa_sample_record_fill(host.ctypes.data, nbytes, int(sample.seed) & 0xFFFFFFFFFFFFFFFF, int(sample.attempt),
                                             float(sample.temperature), flat, self.B), "wipa_sample_record_fill")
        if getattr(self, "_sample_rec", None) is None:
            self._sample_rec = torch.empty(nbytes, dtype=torch.uint8, device=self.blob.device)
        self._sample_rec.copy_(torch.from_numpy(host))  # on the caller's library stream: after every step already enqueued
        return self._sample_rec

    @property
    def starts(self) -> torch.Tensor:
        """the device array int32 [B] of the rows' first own columns (ragged prompts).  ONE buffer per state: the step graph is keyed
        on its address, so every ragged decode of this state replays the same captured step."""
        if getattr(self, "_starts", None) is None:
            self._starts = torch.zeros(self.B, dtype=torch.int32, device=self.blob.device)
        return self._starts

    def adapter_bank(self, bank, ids: Sequence[int]) -> "_lib.AdapterBankC":
        """the wipa_adapter_bank of this state for ``bank`` (lora.AdapterBank), its device array of row ids rewritten in stream order with
        ``ids`` (one per row, -1: no adapter).  ONE struct and ONE id array per (state, bank): the step graph is keyed on their addresses,
        so another assignment of adapters to rows replays the captured graph.  The state keeps every bank it has been used with alive
        (its A / B device pointers are baked into the graphs captured under the struct's address): a replaced bank's tensors are
        freed with the state (``Whisper._invalidate`` releases the states), not before."""
        if len(ids) != self.B or any(not -1 <= int(i) < len(bank) for i in ids):
            raise _lib.WipaError(f"row_adapters: {len(ids)} ids for {self.B} rows, each -1 or below {len(bank)}: {list(ids)[:8]}")
        if getattr(self, "_bank_ids", None) is None:
            self._bank_ids = torch.full((self.B,), -1, dtype=torch.int32, device=self.blob.device)
            self._bank_structs = {}
        self._bank_ids.copy_(torch.tensor([int(i) for i in ids], dtype=torch.int32))  # a plain copy on the caller's library stream
        held = self._bank_structs.get(id(bank))
        if held is None or held[0] is not bank:
            from .lora import SITES

            n_layer = bank.n_layer
            A, B = (C.c_void_p * (n_layer * _lib.BANK_SITES))(), (C.c_void_p * (n_layer * _lib.BANK_SITES))()
            mask = 0
            for (l, site), t in bank.A.items():
                i = SITES.index(site)
                mask |= 1 << i
                A[l * _lib.BANK_SITES + i], B[l * _lib.BANK_SITES + i] = t.data_ptr(), bank.B[(l, site)].data_ptr()
            struct = _lib.AdapterBankC(len(bank), bank.rank, mask, A, B, bank.gain.data_ptr(), self._bank_ids.data_ptr())
            held = self._bank_structs[id(bank)] = (bank, struct, A, B)
        return held[1]

    def prompt_workspace(self, pk, P: int) -> torch.Tensor:
        """the caller-owned workspace of wipa_decoder_prefill_ragged for a prompt width of P; kept, and re-made only to grow (its
        address is part of the prompt pass's graph key)"""
        need = int(_lib.lib().wipa_decoder_prompt_workspace_bytes(C.byref(pk["cfg"]), self.B, P))
        ws = getattr(self, "_prompt_ws", None)
        if ws is None or ws.numel() < need:
            stream().synchronize()  # nothing enqueued may still read the old one
            with on_stream():
                self._prompt_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.blob.device)
        return ws

    def release(self):
        _lib.lib().wipa_decoder_release(ptr(self.blob))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _layout_of(pk, B: int) -> tuple:
    """the blob layout the packed configuration needs, as a comparable tuple"""
    lay = _lib.DecLayout()
    _lib.check(_lib.lib().wipa_decoder_layout(C.byref(pk["cfg"]), B, C.byref(lay)), "wipa_decoder_layout")
    return tuple(getattr(lay, f) for f, _ in lay._fields_)


def _packed_for(model, B: int, new_tokens: Optional[int]):
    """the weight tables + cfg for a decode of B clips x new_tokens positions: cross_attention="auto" picks the absorbed or
    the cached form from the measured table (Whisper.use_absorbed)"""
    return model.packed(absorbed=model.use_absorbed(B, new_tokens))


def _state_for(model, B: int, pk=None) -> DecoderState:
    """one decode blob per (model, library stream); re-made when the batch, the device or the LAYOUT changes.  The layout
    follows the configuration (dtype, cached / absorbed cross-attention, fp8 tables): a bf16 model that decoded with the
    absorbed form holds ONE copy of the features where the cached form needs K and V of every layer (24 x the bytes at
    whisper-small), so e.g. quantize_weights() after a first decode must not find the old blob."""
    pk = pk or model.packed()
    states = model.__dict__.setdefault("_dec_states", {})
    sid = (stream_id(), int(pk["cfg"].dec_cross_absorbed), int(pk["cfg"].dec_n_group))  # one blob per library stream, cross-attention form and group size
    st = states.get(sid)
    if st is not None and (st.B != B or st.blob.device != model.device or st.layout_key != _layout_of(pk, B)):
        stream().synchronize()
        st.release()
        st = None
    if st is None:
        st = DecoderState(model, B, pk)
        states[sid] = st
    return st


# ---------------------------------------------------------------- best-of-N: candidate groups
STREAM_HI_CANDIDATE_SHIFT = 24  # candidate k of a row with stream (lo, hi) draws from (lo, hi + (k << 24))


def candidate_streams(streams: Sequence, n_group: int) -> List[tuple]:
    """per-clip (lo, hi) streams -> per-row streams of clips x n_group candidates, clip-major.  Candidate 0 keeps the clip's stream."""
    out = []
    for lo, hi in streams:
        lo, hi = int(lo), int(hi)
        if n_group > 1 and not 0 <= hi < (1 << STREAM_HI_CANDIDATE_SHIFT):
            raise ValueError(f"sample_streams: hi = {hi} must be below 2**{STREAM_HI_CANDIDATE_SHIFT} with best_of > 1 (the candidate index "
                             "lives in the bits above)")
        out.extend((lo, hi + (k << STREAM_HI_CANDIDATE_SHIFT)) for k in range(n_group))
    return out


def length_penalty_table(n: int, length_penalty: Optional[float]) -> np.ndarray:
    """penalty[length] for length 0..n exactly as upstream's MaximumLikelihoodRanker computes it, in Python floats: ``length`` when
    ``length_penalty`` is None, else ``((5 + length) / 6) ** length_penalty`` (Google NMT)."""
    if length_penalty is None:
        return np.array([float(length) for length in range(n + 1)], dtype=np.float64)
    return np.array([((5 + length) / 6) ** length_penalty for length in range(n + 1)], dtype=np.float64)


def _grouped(pk: dict, n_group: int) -> dict:
    """``pk`` with cfg.dec_n_group = n_group: the same tables behind a copy of the cfg as it is NOW (cross_splits and the weights'
    generation may change between decodes); n_group 1 is ``pk`` itself"""
    if n_group <= 1:
        return pk
    cfg = _lib.ModelCfg.from_buffer_copy(pk["cfg"])
    cfg.dec_n_group = int(n_group)
    return {**pk, "cfg": cfg}


def _rank_groups(st: "DecoderState", n_group: int, sample_begin: int, n: int, eot: int, length_penalty: Optional[float], s):
    """wipa_rank_groups on the state's rows -> host (winner tokens [clips, sample_begin + n] int64, winner sums [clips], winner [clips],
    lengths [clips, G]): clips x columns come back, not rows x columns"""
    clips = st.B // n_group
    dev = st.blob.device
    pen = torch.from_numpy(length_penalty_table(n, length_penalty)).to(dev)
    winner = torch.empty(clips, dtype=torch.int32, device=dev)
    length = torch.empty(st.B, dtype=torch.int32, device=dev)
    width = sample_begin + n
    best = torch.empty(clips, width, dtype=torch.int32, device=dev)
    best_sum = torch.empty(clips, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().wipa_rank_groups(ptr(st.tokens), st.layout.ld_tok, st.B, n_group, sample_begin, n, eot, ptr(st.sum_logprobs), ptr(pen),
                                           ptr(winner), ptr(length), ptr(best), width, ptr(best_sum), sptr(s)), "wipa_rank_groups")
    return (best.cpu().numpy().astype(np.int64), best_sum.cpu().numpy().copy(), winner.cpu().numpy().astype(np.int64),
            length.cpu().numpy().astype(np.int64).reshape(clips, n_group))


@dataclass(frozen=True)
class Beams:
    """what a beam decode needs besides n_group = beam_size: the size of a clip's finished store, round(beam_size * patience)"""
    max_candidates: int


def _beam_finalize(st: "DecoderState", buf: torch.Tensor, n_group: int, beams: Beams, sample_begin: int, n: int, eot: int,
                   length_penalty: Optional[float], s):
    """wipa_beam_finalize on the state's rows -> host (winner tokens [clips, sample_begin + n + 1] int64, eot behind the winner's last
    token; winner sums [clips]; winner lengths [clips]): clips x columns come back"""
    clips = st.B // n_group
    dev = st.blob.device
    pen = torch.from_numpy(length_penalty_table(n, length_penalty)).to(dev)
    width = sample_begin + n + 1
    best = torch.empty(clips, width, dtype=torch.int32, device=dev)
    best_sum = torch.empty(clips, dtype=torch.float32, device=dev)
    best_len = torch.empty(clips, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().wipa_beam_finalize(ptr(buf), ptr(st.tokens), st.layout.ld_tok, st.B, n_group, beams.max_candidates, sample_begin, n, eot,
                                             ptr(st.sum_logprobs), ptr(pen), ptr(best), width, ptr(best_sum), ptr(best_len), sptr(s)),
               "wipa_beam_finalize")
    return best.cpu().numpy().astype(np.int64), best_sum.cpu().numpy().copy(), best_len.cpu().numpy().astype(np.int64)


def _mask(model, ids: Sequence[int]) -> torch.Tensor:
    cache = model.__dict__.setdefault("_mask_cache", {})
    key = tuple(sorted(set(int(i) for i in ids)))
    m = cache.get(key)
    if m is None:
        host = torch.zeros(model.dims.n_vocab, dtype=torch.float32)
        if key:
            host[list(key)] = float("-inf")
        with on_stream() as s:
            m = host.to(model.device)
        s.synchronize()  # masks are shared by every library stream
        cache[key] = m
    return m


@dataclass
class Sampling:
    """what a sampling decode needs besides the logits (DecodingOptions.seed / temperature / sample_streams / sample_attempt)"""
    seed: int
    temperature: float
    streams: Optional[Sequence] = None  # per-row (lo, hi); None: (row, 0)
    attempt: int = 0


@dataclass
class GreedyHandle:
    state: "DecoderState"
    stream: torch.cuda.Stream
    n_init: int
    steps: int  # decoder steps enqueued (prompt positions included)
    keep: tuple = ()  # tensors that must outlive the enqueued work


def _use_prefill(n_init: int, total_steps: int) -> bool:
    """Batched prompt pass (wipa_decoder_prefill) unless WIPA_NO_PREFILL=1 asks for the step-by-step prompt."""
    return n_init >= 2 and total_steps >= n_init and os.environ.get("WIPA_NO_PREFILL") != "1"


def timestamp_rules(tok: Tokenizer, max_initial_timestamp: Optional[float] = 1.0) -> "_lib.DecodeRules":
    """ApplyTimestampRules' parameters for ``tok`` as the wipa_decode_rules the step's tail takes (include/wipa.h):
    max_initial_timestamp_index = round(max_initial_timestamp / 0.02), 50 for the default of 1.0 s; None -> -1, no cap."""
    index = -1 if max_initial_timestamp is None else int(round(float(max_initial_timestamp) / 0.02))
    return _lib.DecodeRules(int(tok.timestamp_begin), int(tok.no_timestamps), index)


def decode_call(n_init: int, eot: int, m_first, m_always, rules=None, sample_rec=None, starts=None, beam=None, continuous: bool = False,
                prompted: bool = False, sample_rows=None, no_speech=None, no_speech_token: int = 0, bank=None) -> "_lib.DecodeCall":
    """The wipa_decode_call (include/wipa.h) of a decode: the masks, ``rules`` (``timestamp_rules``), ``sample_rec`` (the state's device
    sampling record), ``starts`` (the state's device array of first columns; ``n_init`` is then the prompt width P), ``beam`` (the state's
    beam buffer, max_candidates), ``bank`` (the state's wipa_adapter_bank: ``DecoderState.adapter_bank``) and what a continuous stepper
    adds.  None / 0 / False: not used.  It holds addresses only: the tensors
    stay the caller's to keep alive."""
    buf, max_candidates = beam if beam is not None else (None, 0)
    return _lib.DecodeCall(int(n_init), int(eot), ptr(m_first), ptr(m_always), C.pointer(rules) if rules is not None else None, ptr(sample_rec),
                           ptr(sample_rows), ptr(starts), int(continuous), int(prompted), ptr(no_speech), int(no_speech_token), ptr(buf),
                           buf.numel() if buf is not None else 0, int(max_candidates), C.pointer(bank) if bank is not None else None)


def _dec_run(L, pk, st, B, n_init, eot, m_first, m_always, n, use_graph, rules, s, sample_rec=None, starts=None, beam=None, bank=None):
    call = decode_call(n_init, eot, m_first, m_always, rules, sample_rec, starts, beam, bank=bank)
    _lib.check(L.wipa_decoder_run_ex(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, C.byref(call), n, int(use_graph), sptr(s)),
               "wipa_decoder_run_ex")


def _dec_prefill(L, pk, st, B, n_init, eot, m_first, m_always, use_graph, rules, s, sample_rec=None, beam=None, bank=None):
    call = decode_call(n_init, eot, m_first, m_always, rules, sample_rec, None, beam, bank=bank)
    _lib.check(L.wipa_decoder_prefill_ex(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, C.byref(call), int(use_graph), sptr(s)),
               "wipa_decoder_prefill_ex")


def _begin_with(initial_tokens: Sequence[int]):
    """how a decode without per-row prompts begins: wipa_decoder_begin with one prompt of 1..4 tokens for every row (no ``starts``)"""
    n_init = len(initial_tokens)
    init = (C.c_int32 * n_init)(*[int(t) for t in initial_tokens])

    def begin(L, pk, st, B, s):
        _lib.check(L.wipa_decoder_begin(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), B, init, n_init, sptr(s)), "wipa_decoder_begin")
        return None

    return begin


def _bank_of(model, st, row_ids: Optional[Sequence[int]], n_group: int = 1):
    """the state's wipa_adapter_bank for a decode whose rows carry ``row_ids`` (one per clip; candidates share their clip's), or None"""
    if row_ids is None:
        return None
    bank = getattr(model, "_bank", None)
    if bank is None:
        raise _lib.WipaError("row_adapters needs an adapter bank on the model: Whisper.set_adapter_bank(lora.AdapterBank(...))")
    return st.adapter_bank(bank, [int(i) for i in row_ids for _ in range(n_group)])


def _open(model, L, pk, st, audio_features: torch.Tensor, B: int, s, begin, bank=None):
    """the opening of every decode, on the library stream ``s``: the features in the model's dtype into the state
    (wipa_decoder_set_audio; with ``bank`` its cross K / V terms behind it: wipa_decoder_adapt_cross), then ``begin``.  Returns (the
    features, which must outlive the enqueued work, and what ``begin`` returns: the state's device array of first columns, or None)"""
    feats = audio_features.to(device=model.device, dtype=model.dtype).contiguous()
    if tuple(feats.shape[-2:]) != (model.n_audio_ctx, model.dims.n_text_state):  # the state is sized for the effective N
        raise _lib.WipaError(f"decode: audio features of shape {tuple(feats.shape)} given to a model that runs on "
                             f"[.., {model.n_audio_ctx}, {model.dims.n_text_state}] (audio_ctx={model.audio_ctx!r})")
    _lib.check(L.wipa_decoder_set_audio(C.byref(pk["cfg"]), pk["dec_tab"], ptr(feats), ptr(st.blob), st.blob.numel(), B, sptr(s)),
               "wipa_decoder_set_audio")
    if bank is not None:
        _lib.check(L.wipa_decoder_adapt_cross(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, ptr(feats), feats.shape[0], None,
                                              C.byref(bank), sptr(s)), "wipa_decoder_adapt_cross")
    return feats, begin(L, pk, st, B, s)


def greedy_launch(model, audio_features: torch.Tensor, initial_tokens: Sequence[int], suppress_always: Sequence[int],
                  suppress_first: Sequence[int], eot: int, max_new_tokens: int, use_graph: bool = True, rules=None) -> GreedyHandle:
    """Enqueue cross-KV projection + a FIXED number of decoder steps on the current library
    stream and return without synchronising (EOT rows are latched on the device, so running
    past the end of a row is harmless).  Pair with greedy_collect()."""
    L = _lib.lib()
    B = audio_features.shape[0]
    n_init = len(initial_tokens)
    max_new_tokens = min(max_new_tokens, model.dims.n_text_ctx - n_init)
    pk = _packed_for(model, B, max_new_tokens)
    m_always = _mask(model, suppress_always)
    m_first = _mask(model, list(suppress_always) + list(suppress_first))
    begin = _begin_with(initial_tokens)
    total = (n_init - 1) + max_new_tokens
    with on_stream() as s:
        st = _state_for(model, B, pk)
        feats, _ = _open(model, L, pk, st, audio_features, B, s, begin)
        rest = total
        if _use_prefill(n_init, total):  # the prompt positions and the first new token in one batched pass
            _dec_prefill(L, pk, st, B, n_init, eot, m_first, m_always, use_graph, rules, s)
            rest = total - n_init
        _dec_run(L, pk, st, B, n_init, eot, m_first, m_always, rest, use_graph, rules, s)
    return GreedyHandle(st, s, n_init, total, (feats, m_always, m_first, rules))


def greedy_collect(h: GreedyHandle) -> GreedyTokens:
    """Wait for a greedy_launch() and bring the token ids to the host."""
    with torch.cuda.stream(h.stream):
        toks = h.state.tokens[:, : h.steps + 1].cpu().numpy().astype(np.int64)
        slp = h.state.sum_logprobs.cpu().numpy().copy()
    h.stream.synchronize()
    return GreedyTokens(toks, h.steps - (h.n_init - 1), slp, h.state.logits)


def _for_candidates(sample: Optional[Sampling], clips: int, n_group: int) -> Optional[Sampling]:
    """``sample`` for clips x n_group candidate rows: its per-CLIP streams become per-row ones (``candidate_streams``)"""
    if n_group <= 1:
        return sample
    if sample is None:
        raise ValueError("n_group > 1 needs a sampling decode (sample=...): greedy candidates would all be the same row")
    return replace(sample, streams=candidate_streams(sample.streams if sample.streams is not None else [(c, 0) for c in range(clips)], n_group))


def _decode_loop(model, audio_features: torch.Tensor, P: int, max_new_tokens: int, begin, run_prompt, suppress_always, suppress_first,
                 eot: int, stop_on_eot: bool, use_graph: bool, check_every: int, rules, sample: Optional[Sampling], n_group: int, rank: bool,
                 length_penalty: Optional[float], sot_back: Optional[int] = None, beams: Optional[Beams] = None,
                 row_ids: Optional[Sequence[int]] = None) -> GreedyTokens:
    """The decode loop of ``greedy_decode_tokens`` and ``ragged_decode_tokens``, for a prompt of ``P`` columns and ``max_new_tokens``
    already clamped to n_text_ctx - P.  The caller supplies how to begin -- ``begin(L, pk, st, B, s)`` returns the state's device array
    of first columns, or None -- and how the batched prompt pass is run: ``run_prompt(L, pk, st, B, m_first, m_always, rec, starts, s)``
    returns the logits of the <|startoftranscript|> column, or None.  ``sample`` is per ROW here (``_for_candidates``).
    ``beams``: the rows are clips x ``n_group`` BEAMS -- the state's beam buffer is begun behind the tokens, prompt pass and steps are the
    beam entry points (``run_prompt`` takes the buffer as ``beam=``), the loop stops when no clip is still collecting (the state's
    ``not_done``) and the winners of wipa_beam_finalize come back."""
    L = _lib.lib()
    B = audio_features.shape[0] * n_group
    pk = _grouped(_packed_for(model, B, max_new_tokens), n_group)
    st = _state_for(model, B, pk)
    m_always = _mask(model, suppress_always)
    m_first = _mask(model, list(suppress_always) + list(suppress_first))
    total = (P - 1) + max_new_tokens
    done_steps = 0
    sot_logits = None
    with on_stream() as s:
        bank = _bank_of(model, st, row_ids, n_group)  # ``row_ids``: an adapter of the model's bank per clip (-1: none)
        feats, starts = _open(model, L, pk, st, audio_features, B, s, begin, bank)
        rec = st.sample_record(sample) if sample is not None else None
        beam = None
        if beams is not None:
            buf = st.beam_buffer(n_group, beams.max_candidates)
            _lib.check(L.wipa_beam_begin(ptr(buf), buf.numel(), B, n_group, beams.max_candidates, st.layout.ld_tok, sptr(s)), "wipa_beam_begin")
            beam = (buf, beams.max_candidates)
        if _use_prefill(P, total):  # the whole prompt and the first new token in one batched pass
            sot_logits = run_prompt(L, pk, st, B, m_first, m_always, rec, starts, s, **({"beam": beam} if beam is not None else {}),
                                    **({"bank": bank} if bank is not None else {}))
            done_steps = P
        elif sot_back is not None:  # the steps up to the <|startoftranscript|> column: its logits are those of the call's last step
            n = P - sot_back + 1
            _dec_run(L, pk, st, B, P, eot, m_first, m_always, n, use_graph, rules, s, rec, starts, bank=bank)
            sot_logits = st.logits.clone()
            done_steps = n
        while done_steps < total:
            n = min(check_every if stop_on_eot else total, total - done_steps)
            if done_steps < P - 1:  # the rest of the prompt walk rides with the first generated columns
                n = min(total - done_steps, n + (P - 1 - done_steps))
            _dec_run(L, pk, st, B, P, eot, m_first, m_always, n, use_graph, rules, s, rec, starts, beam, bank)
            done_steps += n
            if stop_on_eot and done_steps >= P:
                if beam is not None:  # live beams never hold EOT: the step's tail counts the clips whose finished store is not full
                    if int(st.not_done.cpu()) == 0:  # synchronises the library stream
                        break
                    continue
                last = st.tokens[:, done_steps].cpu()  # synchronises the library stream
                if bool((last == eot).all()):
                    break
        winner = lengths = None
        if beam is not None:  # fill-up and ranking on the device; the winners come back: clips x columns
            toks, slp, best_len = _beam_finalize(st, beam[0], n_group, beams, P, done_steps - (P - 1), eot, length_penalty, s)
            lengths = best_len.reshape(-1, 1)
        elif rank and n_group > 1:  # the winners only come back: clips x columns
            toks, slp, winner, lengths = _rank_groups(st, n_group, P, done_steps - (P - 1), eot, length_penalty, s)
        else:
            toks = st.tokens[:, : done_steps + 1].cpu().numpy().astype(np.int64)  # synchronises: the host arrays of begin are consumed
            slp = st.sum_logprobs.cpu().numpy().copy()
        last_logits = st.logits
        if sot_logits is not None and n_group > 1:
            sot_logits = sot_logits[::n_group]  # the candidates of a clip share their prompt: one row per clip
    n_steps = done_steps - (P - 1)
    if stop_on_eot:
        # the reference stops at the first step after which every row ends in EOT
        body = toks[:, P:]
        all_eot = (body == eot).all(axis=0)
        if all_eot.any():
            n_steps = int(np.argmax(all_eot)) + 1
            toks = toks[:, : P + n_steps]
    return GreedyTokens(toks, n_steps, slp, last_logits, sot_logits=sot_logits, winner=winner, lengths=lengths)


def greedy_decode_tokens(model, audio_features: torch.Tensor, initial_tokens: Sequence[int], suppress_always: Sequence[int],
                         suppress_first: Sequence[int], eot: int, max_new_tokens: Optional[int] = None,
                         stop_on_eot: bool = True, use_graph: bool = True, check_every: int = 8, rules=None,
                         sample: Optional[Sampling] = None, n_group: int = 1, rank: bool = False,
                         length_penalty: Optional[float] = None, beams: Optional[Beams] = None,
                         row_ids: Optional[Sequence[int]] = None) -> GreedyTokens:
    """DecodingTask._main_loop (see module docstring): temperature 0, or a Categorical draw per step with ``sample``.
    ``row_ids``: one id of the model's adapter bank per clip (-1: the base model): every row decodes under its own adapter.
    ``audio_features`` [B, 1500, d] in the model dtype.  ``rules`` (``timestamp_rules``): ApplyTimestampRules in every greedy
    update, on the device; ``initial_tokens`` is then the prompt without <|notimestamps|>.
    ``n_group`` > 1 (upstream's n_group = best_of): every clip is decoded as ``n_group`` candidate rows, clip-major, that share the
    clip's features in the decode state; ``sample.streams`` are per CLIP and candidate k draws from ``candidate_streams``' stream k.
    The result holds all clips x n_group rows -- or, with ``rank``, the winners of wipa_rank_groups only (one row per clip, plus
    ``winner`` and ``lengths``), read back as clips x columns.
    ``beams``: the ``n_group`` rows of a clip are BEAMS at temperature 0 (``sample`` must be None; ``n_group`` 1 is a beam of one).  The
    result holds one row per clip, the winner of wipa_beam_finalize with eot behind its last token, and ``lengths`` [clips, 1]."""
    if beams is not None and sample is not None:
        raise ValueError("beams run at temperature 0: sample must be None")
    if beams is None:
        sample = _for_candidates(sample, audio_features.shape[0], n_group)
    n_init = len(initial_tokens)
    if max_new_tokens is None:
        max_new_tokens = model.dims.n_text_ctx // 2
    max_new_tokens = min(max_new_tokens, model.dims.n_text_ctx - n_init)

    def run_prompt(L, pk, st, B, m_first, m_always, rec, starts, s, beam=None, bank=None):
        _dec_prefill(L, pk, st, B, n_init, eot, m_first, m_always, use_graph, rules, s, rec, beam, bank)

    return _decode_loop(model, audio_features, n_init, max_new_tokens, _begin_with(initial_tokens), run_prompt, suppress_always, suppress_first,
                        eot, stop_on_eot, use_graph, check_every, rules, sample, n_group, rank, length_penalty, beams=beams, row_ids=row_ids)


# ---------------------------------------------------------------- prompt conditioning: per-row prompts
PROMPT_WIDTH_MULTIPLE = 16  # P is rounded up to it: at most n_text_ctx / 16 captured step graphs per state (P is in the graph key)


def _token_ids(tok: Tokenizer, text_or_ids) -> List[int]:
    """upstream: a string becomes ``encode(" " + s.strip())``, a list of ids is taken as it is"""
    if isinstance(text_or_ids, str):
        return [int(t) for t in tok.encode(" " + text_or_ids.strip())]
    return [int(t) for t in text_or_ids]


def initial_tokens(tok: Tokenizer, sot_sequence: Sequence[int], prompt, prefix, n_ctx: int, sample_len: int) -> List[int]:
    """DecodingTask._get_initial_tokens of upstream, literally: ``sot_sequence + prefix[-(n_ctx // 2 - sample_len):]`` (a bound of
    0 keeps everything: ``[-0:]``), and with a non-empty prompt ``[sot_prev] + prompt[-(n_ctx // 2 - 1):]`` in front of it."""
    tokens = [int(t) for t in sot_sequence]
    if prefix is not None and len(prefix):
        prefix_tokens = _token_ids(tok, prefix)
        max_prefix_len = n_ctx // 2 - sample_len
        prefix_tokens = prefix_tokens[-max_prefix_len:]
        tokens = tokens + prefix_tokens
    if prompt is not None and len(prompt):
        prompt_tokens = _token_ids(tok, prompt)
        tokens = [int(tok.sot_prev)] + prompt_tokens[-(n_ctx // 2 - 1):] + tokens
    return tokens


def resolve_prompts(options: DecodingOptions, B: int) -> Optional[List]:
    """the prompt of every row (string, ids or None) from ``options.prompt`` (one for all rows) or ``options.prompts`` (one per
    row); None when no row has one.  Giving both is a ValueError."""
    if options.prompt is not None and options.prompts is not None:
        raise ValueError("DecodingOptions: give prompt (one for all rows) or prompts (one per row), not both")
    if options.prompts is not None:
        rows = list(options.prompts)
        if len(rows) != B:
            raise ValueError(f"DecodingOptions.prompts: {len(rows)} prompts for {B} rows")
    else:
        rows = [options.prompt] * B
    rows = [r if (r is not None and len(r)) else None for r in rows]
    return rows if any(r is not None for r in rows) else None


def pack_prompts(rows: Optional[Sequence[Sequence[int]]], n_ctx: int, sample_len: int, pad_to: Optional[int] = None):
    """Per-row initial tokens -> ``(tokens [B, P] int32, starts [B] int32, P)``: row b right-aligned in columns [P - n_b, P), token 0
    before them.  P = the longest row rounded up to a multiple of 16, unless that would leave fewer than ``min(sample_len, n_ctx -
    longest)`` columns to generate in: then P = longest.  ``pad_to``: this P instead (a row decoded alone at the width of a batch).
    ``rows`` None (no row has a prompt or a prefix): None -- there is no ragged path to take."""
    if rows is None:
        return None
    rows = [[int(t) for t in r] for r in rows]
    if not rows or any(len(r) < 1 for r in rows):
        raise ValueError("pack_prompts: every row holds at least one initial token")
    longest = max(len(r) for r in rows)
    if longest > n_ctx:
        raise ValueError(f"pack_prompts: {longest} initial tokens exceed n_text_ctx = {n_ctx}")
    if pad_to is not None:
        P = int(pad_to)
        if P < longest or P > n_ctx:
            raise ValueError(f"pack_prompts: pad_to = {P} outside {longest}..{n_ctx}")
    else:
        P = -(-longest // PROMPT_WIDTH_MULTIPLE) * PROMPT_WIDTH_MULTIPLE
        if n_ctx - P < min(sample_len, n_ctx - longest):
            P = longest
    tokens = np.zeros((len(rows), P), dtype=np.int32)
    starts = np.zeros(len(rows), dtype=np.int32)
    for b, r in enumerate(rows):
        starts[b] = P - len(r)
        tokens[b, P - len(r):] = r
    return tokens, starts, P


def ragged_decode_tokens(model, audio_features: torch.Tensor, rows: Sequence[Sequence[int]], suppress_always: Sequence[int],
                         suppress_first: Sequence[int], eot: int, max_new_tokens: Optional[int] = None, stop_on_eot: bool = True,
                         use_graph: bool = True, check_every: int = 8, rules=None, sample: Optional[Sampling] = None,
                         pad_to: Optional[int] = None, sot_back: Optional[int] = None, n_group: int = 1, rank: bool = False,
                         length_penalty: Optional[float] = None, row_ids: Optional[Sequence[int]] = None) -> GreedyTokens:
    """``greedy_decode_tokens`` for rows with their OWN initial tokens (``rows[b]``: [sot_prev] + history + sot_sequence + prefix), packed
    by ``pack_prompts``.  ``tokens`` of the result are [B, P + n_steps] with the padding in front; ``n_init`` = P.  The prompt goes through
    one batched pass (wipa_decoder_prefill_ragged); with WIPA_NO_PREFILL=1 it is walked column by column by the replayed decode step,
    which is what the batched pass is tested against.  ``sot_back``: the rows' <|startoftranscript|> sits ``sot_back`` columns before P
    (len(sot_sequence) + len(prefix)); the unfiltered logits of that column come back as ``sot_logits`` (upstream's
    ``logits[:, sot_index]`` for no_speech_prob).  ``max_new_tokens`` is clamped to n_text_ctx - P.
    ``n_group`` / ``rank`` / ``length_penalty``: candidate groups as in ``greedy_decode_tokens``: ``rows`` and ``sample.streams`` are per
    clip, every candidate of a clip starts from the clip's own initial tokens, ``sot_logits`` and ``starts`` stay per clip.
    ``row_ids``: one id of the model's adapter bank per clip (-1: the base model); the prompt pass is then
    wipa_decoder_prefill_ragged_bank and the prompt columns of a row run under the row's adapter like its steps."""
    clips = audio_features.shape[0]
    n_ctx = model.dims.n_text_ctx
    if getattr(model, "_fp8", None):
        raise NotImplementedError("prompt conditioning is not implemented for an fp8-quantised model: the ragged decode step runs on "
                                  "bf16 / f32 decoder tables")
    if len(rows) != clips:
        raise ValueError(f"ragged_decode_tokens: {len(rows)} rows of initial tokens for {clips} clips")
    sample = _for_candidates(sample, clips, n_group)
    if max_new_tokens is None:
        max_new_tokens = n_ctx // 2
    tokens_h, starts_h, P = pack_prompts(rows, n_ctx, max_new_tokens, pad_to)
    max_new_tokens = min(max_new_tokens, n_ctx - P)
    if max_new_tokens < 1:
        raise ValueError(f"ragged_decode_tokens: a prompt width of {P} leaves no room to generate in n_text_ctx = {n_ctx}")
    if sot_back is not None and not 1 <= sot_back <= P - int(starts_h.max()):
        raise ValueError(f"ragged_decode_tokens: sot_back = {sot_back} outside the shortest row")
    clip_starts_h = starts_h
    if n_group > 1:  # every candidate starts from its clip's initial tokens; the features are not replicated
        tokens_h, starts_h = np.repeat(tokens_h, n_group, axis=0), np.repeat(starts_h, n_group)
    tokens_h = np.ascontiguousarray(tokens_h, dtype=np.int32)
    starts_h = np.ascontiguousarray(starts_h, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)

    def begin(L, pk, st, B, s):
        starts = st.starts
        _lib.check(L.wipa_decoder_begin_ragged(C.byref(pk["cfg"]), ptr(st.blob), st.blob.numel(), B, tokens_h.ctypes.data_as(i32p),
                                               starts_h.ctypes.data_as(i32p), P, ptr(starts), sptr(s)), "wipa_decoder_begin_ragged")
        return starts

    def run_prompt(L, pk, st, B, m_first, m_always, rec, starts, s, bank=None):
        ws = st.prompt_workspace(pk, P)
        args = (C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, P, P - sot_back if sot_back is not None else -1, eot,
                ptr(m_first), ptr(m_always), int(use_graph), C.byref(rules) if rules is not None else None,
                ptr(rec) if rec is not None else None, ptr(starts), ptr(ws), ws.numel())
        if bank is None:
            _lib.check(L.wipa_decoder_prefill_ragged(*args, sptr(s)), "wipa_decoder_prefill_ragged")
        else:
            _lib.check(L.wipa_decoder_prefill_ragged_bank(*args, C.byref(bank), sptr(s)), "wipa_decoder_prefill_ragged_bank")
        if sot_back is None:
            return None
        ld = st.layout.ld_logits  # the pass leaves the <|startoftranscript|> column's logits at the head of its workspace
        return ws[: B * ld * 4].view(torch.float32).view(B, ld)[:, : model.dims.n_vocab].clone()

    g = _decode_loop(model, audio_features, P, max_new_tokens, begin, run_prompt, suppress_always, suppress_first, eot, stop_on_eot, use_graph,
                     check_every, rules, sample, n_group, rank, length_penalty, sot_back, row_ids=row_ids)
    g.n_init, g.starts = P, (clip_starts_h if rank and n_group > 1 else starts_h).copy()
    return g


def forced_decode_logits(model, audio_features: torch.Tensor, tokens: np.ndarray, n_init: int, suppress_always: Sequence[int],
                         suppress_first: Sequence[int], eot: int, use_graph: bool = True, rules=None, row_ids: Optional[Sequence[int]] = None):
    """The KV-cached decode-step path (prompt prefill + replayed step graph -- the kernels greedy_decode_tokens runs) driven
    along a GIVEN token history: after every step the greedy choice is read and then overwritten with ``tokens[:, p + 1]``.
    ``tokens`` [B, n_init + n_steps] int (host).  Returns (step logits [B, n_steps, V] f32 on the device, unfiltered, and the
    path's own greedy choices [B, n_steps] int64 on the host).  A measurement aid: with the history of an f32 reference it
    gives the logit error of a low-precision model at every step, independent of where its own greedy ids would part
    (DecodingTask._main_loop, transcribe_single.py:55)."""
    L = _lib.lib()
    tokens = np.asarray(tokens)
    B, total_len = tokens.shape
    assert B == audio_features.shape[0] and 2 <= n_init < total_len <= model.dims.n_text_ctx
    n_steps = total_len - n_init
    pk = _packed_for(model, B, n_steps)
    st = _state_for(model, B, pk)
    m_always = _mask(model, suppress_always)
    m_first = _mask(model, list(suppress_always) + list(suppress_first))
    assert (tokens[:, :n_init] == tokens[0, :n_init]).all(), "one prompt for all rows"
    V = model.dims.n_vocab
    with on_stream() as s:
        forced = torch.from_numpy(tokens.astype(np.int32)).to(model.device)
        trace = torch.empty(B, n_steps, V, dtype=torch.float32, device=model.device)
        chosen = torch.empty(B, n_steps, dtype=torch.int32, device=model.device)
        bank = _bank_of(model, st, row_ids)  # ``row_ids``: an adapter of the model's bank per row (-1: none)
        feats, _ = _open(model, L, pk, st, audio_features, B, s, _begin_with(tokens[0, :n_init]), bank)
        _dec_prefill(L, pk, st, B, n_init, eot, m_first, m_always, use_graph, rules, s, bank=bank)
        for i in range(n_steps):
            p = n_init + i  # the token position the last step has just filled
            trace[:, i].copy_(st.logits)
            chosen[:, i].copy_(st.tokens[:, p])
            st.tokens[:, p].copy_(forced[:, p])
            if i + 1 < n_steps:
                _dec_run(L, pk, st, B, n_init, eot, m_first, m_always, 1, use_graph, rules, s, bank=bank)
        out_chosen = chosen.cpu().numpy().astype(np.int64)
    return trace, out_chosen


def _sot_pass(model, audio_features: torch.Tensor, tokenizer: Tokenizer) -> GreedyTokens:
    """one decoder step on the prompt [sot], every logit but the language tokens masked in the greedy update; ``last_logits``
    are the UNFILTERED logits of that position"""
    lang = set(tokenizer.all_language_tokens)
    not_lang = [i for i in range(model.dims.n_vocab) if i not in lang]
    # with n_init = 1 the greedy kernel applies mask_first at position 0
    return greedy_decode_tokens(model, audio_features, [tokenizer.sot], not_lang, [], eot=-1, max_new_tokens=1, stop_on_eot=False)


def _no_speech_from(last_logits: torch.Tensor, tokenizer: Tokenizer) -> np.ndarray:
    with on_stream():
        return torch.softmax(last_logits.float(), dim=-1)[:, tokenizer.no_speech].cpu().numpy().astype(np.float64)


def detect_language(model, audio_features: torch.Tensor, tokenizer: Tokenizer, with_no_speech: bool = False):
    """Whisper.detect_language (train_whisper_ipa.py:339 via language=None): one decoder pass on
    [sot]; every logit but the language tokens masked; argmax.  Returns (language token ids [B], probs); with
    ``with_no_speech`` also the no-speech probabilities of the same pass (``no_speech_probs``)."""
    lang = list(tokenizer.all_language_tokens)
    res = _sot_pass(model, audio_features, tokenizer)
    with on_stream():
        probs = torch.softmax(res.last_logits[:, lang].float(), dim=-1).cpu().numpy()
    if with_no_speech:
        return res.tokens[:, 1], probs, _no_speech_from(res.last_logits, tokenizer)
    return res.tokens[:, 1], probs


def no_speech_probs(model, audio_features: torch.Tensor, tokenizer: Tokenizer) -> np.ndarray:
    """DecodingResult.no_speech_prob of upstream's DecodingTask: softmax of the unfiltered logits after the prompt's first token
    [sot] at <|nospeech|>, per row -- the decoder pass detect_language makes."""
    return _no_speech_from(_sot_pass(model, audio_features, tokenizer).last_logits, tokenizer)


def _suppress_lists(options: DecodingOptions, tok: Tokenizer):
    suppress = options.suppress_tokens
    if isinstance(suppress, str):
        suppress = [int(t) for t in suppress.split(",")]
    suppress = list(suppress or [])
    if -1 in suppress:
        suppress = [t for t in suppress if t >= 0] + list(tok.non_speech_tokens)
    suppress += [tok.transcribe, tok.translate, tok.sot, tok.sot_prev, tok.sot_lm, tok.no_speech]
    first = [tok.encode(" ")[0], tok.eot] if options.suppress_blank else []
    return sorted(set(suppress)), first


def best_of_group(options: DecodingOptions) -> int:
    """upstream's DecodingTask._verify_options for the sampling options, and the candidates per clip they ask for (n_group = best_of or
    1).  ``best_of`` needs a temperature above 0 (upstream's ValueError) and, like every sampling decode here, a seed; with it
    ``length_penalty`` lies in 0..1 (upstream's ValueError) and ``patience``, which belongs to the beams, is refused.  A decode without
    ``best_of`` is checked as it always was: both options are ignored there, and beams stay refused (``_refuse_unsupported``)."""
    if options.beam_size is not None and options.best_of is not None:
        raise ValueError("beam_size and best_of can't be given together")
    if options.temperature == 0 and options.best_of is not None:
        raise ValueError("best_of with greedy sampling (T=0) is not compatible")
    if options.best_of is None:
        return 1
    if options.length_penalty is not None and not (0 <= options.length_penalty <= 1):
        raise ValueError("length_penalty (alpha) should be a value between 0 and 1")
    if options.patience is not None:
        raise NotImplementedError("patience is not implemented: it belongs to beam search (beam_size), which is not implemented")
    n = int(options.best_of)
    if n < 1 or n != options.best_of:
        raise ValueError(f"best_of must be a positive integer, got {options.best_of!r}")
    if n > 64:
        raise ValueError(f"best_of = {n}: at most 64 candidates per clip (wipa_rank_groups ranks a group in one wave)")
    if options.seed is None:
        raise NotImplementedError("best_of needs DecodingOptions.seed: sampling is opt-in and reproducible by construction "
                                  "(temperature without a seed is not implemented)")
    if n > 1 and options.sample_streams is not None:
        candidate_streams(options.sample_streams, n)  # hi >= 2**24 is a ValueError
    return n


def beam_group(options: DecodingOptions, model) -> Optional[tuple]:
    """upstream's DecodingTask._verify_options for the beam options and what they ask for: None without ``beam_size``, else
    ``(beam_size, max_candidates)`` with ``max_candidates = round(beam_size * patience)`` (``patience`` None is 1.0).  ``beam_size`` is an
    int in 1..16 (1: the beam path with one row per clip), ``patience`` is above 0 with 1 <= max_candidates <= 64, ``length_penalty`` lies
    in 0..1 (upstream's ValueError).  Refused by name: a model that is not a loaded Whisper on bf16 / f32 decoder tables, a temperature
    above 0 (upstream drops the beams there; ``transcribe`` does that itself), prompts and prefixes."""
    if options.beam_size is None:
        return None
    n = options.beam_size
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= 16:
        raise ValueError(f"beam_size must be an integer between 1 and 16, got {n!r}")
    n = int(n)
    if options.patience is not None and not options.patience > 0:
        raise ValueError("patience should be a positive number")
    max_candidates = round(n * (1.0 if options.patience is None else float(options.patience)))
    if not 1 <= max_candidates <= 64:
        raise ValueError(f"round(beam_size * patience) = {max_candidates} must lie between 1 and 64")
    if options.length_penalty is not None and not (0 <= options.length_penalty <= 1):
        raise ValueError("length_penalty (alpha) should be a value between 0 and 1")
    if model is None or not hasattr(model, "packed") or not hasattr(model, "dims"):
        raise NotImplementedError("beam_size is served by decode() on a loaded Whisper model only (bf16 / f32 decoder tables)")
    if getattr(model, "_fp8", None):
        raise NotImplementedError("beam_size is not implemented for an fp8-quantised model: the beam step runs on bf16 / f32 decoder tables")
    if options.temperature != 0.0:
        raise NotImplementedError("beam_size at a temperature above 0 is not implemented: beams run at temperature 0 (upstream's fallback "
                                  "drops beam_size above 0; transcribe() does the same)")
    if (options.prompt is not None and len(options.prompt)) or (options.prefix is not None and len(options.prefix)) or options.prompts is not None:
        raise NotImplementedError("beam_size with prompt / prefix / prompts is not implemented: beams run on rows without prompts")
    return n, int(max_candidates)


MAX_DECODE_ROWS = 65535  # rows of one decode state: the step's kernels put the row on a 16-bit grid axis


def _refuse_unsupported(options: DecodingOptions) -> None:
    """what a path that decodes one row per clip does not serve.  ``decode()`` serves best_of itself (``best_of_group``) and shows this
    function the options without it, as it does with the prompts."""
    if options.beam_size or (options.best_of or 1) > 1:
        raise NotImplementedError("beam_size is not implemented (the reference's decoder has no beam search either) and best_of is "
                                  "served by decode() only, at a temperature above 0 with a seed")
    if options.temperature != 0.0 and options.seed is None:
        raise NotImplementedError("temperature above 0 needs DecodingOptions.seed: sampling is opt-in and reproducible by construction "
                                  "(temperature without a seed is not implemented)")
    if options.temperature < 0.0:
        raise ValueError(f"temperature must be >= 0, got {options.temperature}")
    if not options.without_timestamps and (options.prompt is not None or options.prefix is not None):
        raise NotImplementedError("prompt / prefix conditioning is not implemented on the timestamp path")
    if getattr(options, "prompts", None) is not None:
        raise NotImplementedError("prompts (per-row prompt conditioning) is served by decode() only")
    if getattr(options, "row_adapters", None) is not None:
        raise NotImplementedError("row_adapters (an adapter of the model's bank per row) is served by decode() and decode_continuous() only")


def _row_adapter_ids(model, options: DecodingOptions, n_rows: int, beams: bool) -> Optional[List[int]]:
    """``options.row_adapters`` as ids of the model's adapter bank, one per clip (None without it).  Refused by name: no bank on the
    model, a count that differs from the clips', an unknown name, beam search."""
    if options.row_adapters is None:
        return None
    bank = getattr(model, "_bank", None)
    if bank is None:
        raise _lib.WipaError("row_adapters needs an adapter bank on the model: Whisper.set_adapter_bank(lora.AdapterBank(...))")
    if beams:
        raise NotImplementedError("row_adapters with beam_size is not implemented: beam search decodes one adapter at a time (Whisper.set_adapter)")
    if len(options.row_adapters) != n_rows:
        raise ValueError(f"row_adapters: {len(options.row_adapters)} names for {n_rows} clips")
    return bank.ids(options.row_adapters)


def decode(model, mel: torch.Tensor, options: DecodingOptions = DecodingOptions(), **kwargs):
    """mlx_whisper.decoding.decode: accepts a mel [B,3000,n_mels] / [3000,n_mels] or encoded
    features [B,1500,d] / [1500,d]; returns a DecodingResult or a list of them."""
    if kwargs:
        options = DecodingOptions(**{**options.__dict__, **kwargs})
    # decode() serves prompts itself: they are resolved first and the refusals see the options without them
    n_rows = 1 if mel.dim() == 2 else mel.shape[0]
    prompts = resolve_prompts(options, n_rows)
    prefix = options.prefix if (options.prefix is not None and len(options.prefix)) else None
    n_group = best_of_group(options)  # decode() serves best_of itself too: candidate groups that share one encoder output
    beam = beam_group(options, model)  # ... and beams, before it touches the features: groups of beam_size rows
    if beam is not None:
        n_group = beam[0]
    _refuse_unsupported(replace(options, prompt=None, prefix=None, prompts=None, best_of=None, beam_size=None, row_adapters=None))
    row_ids = _row_adapter_ids(model, options, n_rows, beam is not None)
    if (prompts is not None or prefix is not None) and getattr(model, "_fp8", None):
        raise NotImplementedError("prompt / prefix conditioning is not implemented for an fp8-quantised model: the ragged decode step "
                                  "runs on bf16 / f32 decoder tables")
    single = mel.dim() == 2
    if single:
        mel = mel[None]
    d = model.dims
    if model.is_features(mel):  # by the effective N (model.audio_ctx); features of another length are refused
        feats = mel
    else:
        feats = model.embed_audio(mel)
    if options.fp16 and model.dtype == torch.float32:
        # DecodingOptions.fp16=True (default; transcribe_single.py:49-52) casts the features to fp16
        # before cross-attention while the weights stay f32
        with on_stream():
            feats = feats.to(torch.float16).to(torch.float32)
    B = feats.shape[0]
    tok = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=options.language or "en",
                        task=options.task)
    # without_timestamps=False: mlx_whisper.transcribe's decode (the reference's scripts/evaluate_model.py:112-119): the prompt is
    # the three-token sot_sequence and ApplyTimestampRules runs in every greedy update
    timed = not options.without_timestamps
    rules = timestamp_rules(tok, options.max_initial_timestamp) if timed else None
    initial = list(tok.sot_sequence) if timed else list(tok.sot_sequence_including_notimestamps)
    languages = [options.language or "en"] * B
    lang_probs = [None] * B
    no_speech = [float("nan")] * B  # filled on the timestamp path only: the without_timestamps=True path stays as it was
    if options.language is None:
        # NOTE: one language per batch row in the reference; rows may differ, so decode per detected group
        if timed:
            lang_tokens, probs, nsp = detect_language(model, feats, tok, with_no_speech=True)
            no_speech = [float(v) for v in nsp]
        else:
            lang_tokens, probs = detect_language(model, feats, tok)
        from .tokenizer import LANGUAGES
        languages = [LANGUAGES[int(t) - tok.sot - 1] for t in lang_tokens]
        lang_probs = [dict(zip(LANGUAGES[: tok.num_languages], p.tolist())) for p in probs]
    elif timed and prompts is None and prefix is None:
        no_speech = [float(v) for v in no_speech_probs(model, feats, tok)]
    always, first = _suppress_lists(options, tok)
    sample_len = options.sample_len or d.n_text_ctx // 2
    # temperature 0 with a seed is the greedy path, bit for bit; above 0 every row draws from its own stream, whichever language
    # group it lands in
    streams = None
    if options.temperature != 0.0:
        streams = [(int(a), int(b)) for a, b in options.sample_streams] if options.sample_streams is not None else [(i, 0) for i in range(B)]
        if len(streams) != B:
            raise ValueError(f"sample_streams: {len(streams)} streams for {B} rows")
    results: List[Optional[DecodingResult]] = [None] * B
    # best_of: a clip's candidates ride in ONE state and share its audio there; the ranker leaves one row per clip
    group_kw = dict(n_group=n_group, rank=True, length_penalty=options.length_penalty) if n_group > 1 else {}
    if beam is not None:  # the beams of a clip ride in one state too; wipa_beam_finalize leaves one row per clip
        group_kw = dict(n_group=n_group, length_penalty=options.length_penalty, beams=Beams(beam[1]))
    per_call = max(1, MAX_DECODE_ROWS // n_group)  # more rows than a state holds: chunks of whole groups
    for lang in sorted(set(languages)):
        lang_rows = [i for i, l in enumerate(languages) if l == lang]
        init = list(initial)
        init[1] = tok.to_language_token(lang)
        for rows in ([lang_rows] if n_group == 1 and beam is None else [lang_rows[c:c + per_call] for c in range(0, len(lang_rows), per_call)]):
            sub = feats[rows] if len(rows) != B else feats
            sample = None if streams is None else Sampling(int(options.seed), float(options.temperature), [streams[i] for i in rows],
                                                           int(options.sample_attempt))
            if prompts is None and prefix is None:  # no row has a prompt: the path without prompts, call for call
                g = greedy_decode_tokens(model, sub, init, always, first, tok.eot, max_new_tokens=sample_len, rules=rules, sample=sample,
                                         **group_kw, **({"row_ids": [row_ids[i] for i in rows]} if row_ids is not None else {}))
                n_init = len(init)
            else:
                own = [initial_tokens(tok, init, prompts[i] if prompts is not None else None, prefix, d.n_text_ctx, sample_len) for i in rows]
                sot_back = len(initial_tokens(tok, init, None, prefix, d.n_text_ctx, sample_len))  # sot_sequence + prefix: the same for every row
                g = ragged_decode_tokens(model, sub, own, always, first, tok.eot, max_new_tokens=sample_len, rules=rules, sample=sample,
                                         sot_back=sot_back if timed else None, **group_kw,
                                         **({"row_ids": [row_ids[i] for i in rows]} if row_ids is not None else {}))
                n_init = g.n_init
                if timed:  # upstream's logits[:, sot_index] of the prompted pass
                    nsp = _no_speech_from(g.sot_logits, tok)
                    for j, i in enumerate(rows):
                        no_speech[i] = float(nsp[j])
            for j, i in enumerate(rows):  # with best_of row j of g is clip j's winner
                row = g.tokens[j, n_init:].tolist()
                if tok.eot in row:
                    row = row[: row.index(tok.eot)]
                text = tok.decode([t for t in row if t < tok.timestamp_begin]).strip()  # tokens keeps the timestamps, text does not
                comp = compression_ratio(text)
                results[i] = DecodingResult(audio_features=feats[i], language=lang, language_probs=lang_probs[i], tokens=row,
                                            text=text, avg_logprob=float(g.sum_logprobs[j]) / (len(row) + 1),
                                            temperature=options.temperature, compression_ratio=comp, no_speech_prob=no_speech[i])
    return results[0] if single else results
