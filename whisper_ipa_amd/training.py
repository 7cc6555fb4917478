"""Decoder-only fine-tune step (f32) with the semantics of the reference's ``train_step``
(scripts/train_whisper_ipa.py:266-311): encoder frozen (:187), teacher forcing on
``tokens[:, :-1]`` against ``tokens[:, 1:]`` (:228-232), masked CE with the batch-GLOBAL valid count
(:242-261), gradients w.r.t. every ``decoder.*`` tensor (tied embedding included), PER-TENSOR clip
(:287-303), mlx-style AdamW without bias correction (:513).

mlx's ``nn.value_and_grad`` is replaced by an explicit forward that saves activations and a
hand-written backward; every arithmetic step is a libwipa kernel (GEMMs through wipa_gemm on
operands transposed by wipa_transpose, flash-style attention backward, LayerNorm/GELU/CE backward,
fused clip+AdamW over one flat parameter buffer).  torch only owns the buffers.

``train_encoder_layers`` (no counterpart in the reference) adds the last K encoder blocks, or the whole encoder with its conv stem, to
what is trained: an encoder forward that keeps its activations, the gradient of the encoder output out of the decoder's backward, and
an encoder backward that shares the decoder's block halves; the stem's backward is csrc/conv_bwd.hip plus K-major GEMMs.

Data parallel (one process per GPU): the (sum CE, valid count) pair is all-reduced BEFORE the
backward so the normalisation is global, the flat gradient buffer is all-reduced in buckets AFTER
it, and the per-tensor clip runs on the reduced gradients -- single-process semantics are kept.
"""
from __future__ import annotations


import ctypes as C
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, lora as lora_mod, ops, parallel
from .runtime import on_stream, ptr, sptr
from .whisper import Whisper, parameter_names

QK_SCALE = 64 ** -0.25
OPT_CHUNK = 4096


def _ceil(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _stem_rows(B: int, N: int) -> SimpleNamespace:
    """Row counts of the conv stem's training buffers for B clips of N positions, for the forward that fills them and the backward
    that contracts over them.  ``R`` rows per clip in the padded layouts: 2N frames and a zero halo row either side.  ``M1`` /
    ``M2``: the rows of conv1's / conv2's GEMM (R, and N + 1 with the last one dead, per clip).  ``Kc1`` / ``Kc2``: those in whole
    32-row K-steps, the contraction lengths of the two weight-gradient GEMMs and the rows of dz1 / of the padded dz2.
    ``padded`` / ``z1``: the rows of the padded mel and of conv1's output (and its GELU).  Rows past M1 + 4 exist (as zeros) for
    the weight gradients' padded contractions, which read them as OVERLAPPING rows (_wgrad_rows): three mel rows from each of
    Kc1 rows, three rows from every second of 2 Kc2."""
    R = 2 * N + 2
    M1, M2 = B * R, B * (N + 1)
    Kc1, Kc2 = _ceil(M1, 32), _ceil(M2, 32)
    return SimpleNamespace(R=R, M1=M1, M2=M2, Kc1=Kc1, Kc2=Kc2, padded=max(M1 + 4, Kc1 + 3), z1=max(M1 + 4, 2 * Kc2 + 2))


class FrozenFeatureCache:
    """HBM-resident cache of the FROZEN encoder's output, keyed by clip (dataset index).

    The reference recomputes ``model.embed_audio(mel)`` in every training step although the encoder is frozen
    (scripts/train_whisper_ipa.py:187,223): its output is a pure function of the clip.  whisper-small
    features are 1500 x 768 f32 = 4.6 MB per clip, so the 7 000 training clips of data/v2_filtered are 32 GB of a 288 GB
    HBM: keep them.  A clip's features are computed once, by the same kernels, and are bit-identical whatever batch they are
    computed in (tests/test_gpu_training.py), so training with the cache gives bit-identical losses and parameters.
    Clips beyond ``max_clips`` are simply recomputed every time (spill to recompute, no eviction).  The entries are
    functions of the encoder weights: the model counts every change of an ``encoder.*`` tensor (load_weights / update /
    set_dtype / quantize_weights -> ``Whisper._enc_generation``) and the cache drops itself when the count moved, so stale
    features cannot survive an encoder update; DecoderTrainer itself never touches encoder tensors.
    With ``model.audio_ctx`` = N a row is N x d (five times as many clips fit at N = 300); a change of it counts as an encoder update.
    The bit-identity across batches holds while every encoder GEMM runs in the tile kernels, i.e. for batches of more than 256 / N
    clips: below that wipa_gemm takes the weight-streaming kernel, whose summation order differs in the last bits (N <= 256 only)."""

    def __init__(self, model: Whisper, max_clips: int):
        self.model, self.max_clips = model, int(max_clips)
        self.slots: Dict[int, int] = {}
        self.store: Optional[torch.Tensor] = None  # [max_clips, 1500, d] f32, allocated on first use
        self._pinned = None  # ring of [pinned int64 [2, n], event of the last upload]: host staging of the gather indices
        self._ring = 0
        self.hits = self.misses = 0
        self._enc_generation = model._enc_generation

    @property
    def row_shape(self):
        """(N, d): N the positions the model runs on -- changing model.audio_ctx counts as an encoder change and drops the entries"""
        return (self.model.n_audio_ctx, self.model.dims.n_audio_state)

    def _drop_if_encoder_changed(self) -> None:
        if self._enc_generation != self.model._enc_generation:
            self.clear()
            if self.store is not None and tuple(self.store.shape[1:]) != self.row_shape:
                self.store = None  # rows of another length (model.audio_ctx changed): allocated again on first use
            self._enc_generation = self.model._enc_generation

    @staticmethod
    def clips_that_fit(model: Whisper, fraction_of_free: float = 0.5) -> int:
        free, _ = torch.cuda.mem_get_info(model.device)
        return int(free * fraction_of_free) // (model.n_audio_ctx * model.dims.n_audio_state * 4)

    def clear(self) -> None:
        self.slots.clear()
        self.hits = self.misses = 0

    def missing(self, keys) -> List[bool]:
        """per key: True when the clip's features are not cached (its audio / mel is needed)"""
        self._drop_if_encoder_changed()
        return [int(k) not in self.slots for k in keys]

    def assemble(self, keys, mel_of_missing: Optional[torch.Tensor]) -> torch.Tensor:
        """features [B, 1500, d] f32 for ``keys``; ``mel_of_missing`` [n_missing, 3000, n_mels] holds the mel of the keys
        for which missing() is True, in order (None when there are none)."""
        self._drop_if_encoder_changed()
        keys = [int(k) for k in keys]
        miss_pos = [i for i, k in enumerate(keys) if k not in self.slots]
        n_miss = 0 if mel_of_missing is None else mel_of_missing.shape[0]
        if n_miss != len(miss_pos):
            raise _lib.WipaError(f"FrozenFeatureCache: {len(miss_pos)} clips are not cached but the mel of {n_miss} was given")
        with on_stream():
            out = torch.empty(len(keys), *self.row_shape, dtype=torch.float32, device=self.model.device)
            if miss_pos:
                fresh = self.model.embed_audio(mel_of_missing)
                for j, i in enumerate(miss_pos):
                    out[i].copy_(fresh[j])
                    k = keys[i]
                    if k not in self.slots and len(self.slots) < self.max_clips:
                        if self.store is None:
                            self.store = torch.empty(self.max_clips, *self.row_shape, dtype=torch.float32, device=self.model.device)
                        self.slots[k] = len(self.slots)
                        self.store[self.slots[k]].copy_(fresh[j])
            miss = set(miss_pos)
            hit_pos = [i for i in range(len(keys)) if i not in miss]
            if hit_pos:
                # the two index vectors go up through a pinned staging buffer with non-blocking copies: a torch.tensor(...,
                # device=...) from pageable memory makes the host wait for the stream to drain, i.e. for the whole previous step,
                # and the GPU then idles while the host enqueues this one (7 ms per step at 32 x 64)
                n = len(hit_pos)
                # a ring of four staging buffers, each guarded by the event of its last upload: the host may run several steps
                # ahead of the GPU, and a buffer must not be rewritten before its copy has been executed
                if self._pinned is None or self._pinned[0][0].shape[1] < n:
                    self._pinned = [[torch.empty(2, max(n, 64), dtype=torch.int64).pin_memory(), None] for _ in range(4)]
                    self._ring = 0
                buf = self._pinned[self._ring]
                self._ring = (self._ring + 1) % len(self._pinned)
                if buf[1] is not None:
                    buf[1].synchronize()
                buf[0][0, :n] = torch.tensor([self.slots[keys[i]] for i in hit_pos], dtype=torch.int64)
                buf[0][1, :n] = torch.tensor(hit_pos, dtype=torch.int64)
                dev = buf[0][:, :n].to(self.model.device, non_blocking=True)
                buf[1] = torch.cuda.Event()
                buf[1].record(torch.cuda.current_stream(self.model.device))
                if n == len(keys) and hit_pos == list(range(n)):
                    torch.index_select(self.store, 0, dev[0], out=out)
                else:
                    out.index_copy_(0, dev[1], self.store.index_select(0, dev[0]))
        self.hits += len(hit_pos)
        self.misses += len(miss_pos)
        return out


CLIP_SCOPES = ("reference", "all")


def clip_reaches(name: str, scope: str = "reference") -> bool:
    """Does the reference's ``clip_grad_dict`` (train_whisper_ipa.py:287-303) reach the gradient ``name``?  It walks dict
    values only: a tensor below a list (``decoder.blocks.{i}....``; mlx_whisper keeps the blocks in a Python list, and the
    reference's flatten_params :50-53 has the matching list branch) is handed back as it came (:299-300)."""
    if scope == "all":
        return True
    return not any(part.isdigit() for part in name.split("."))


def resolve_train_encoder_layers(value, n_audio_layer: int) -> Tuple[int, bool]:
    """``train_encoder_layers`` -> (index of the first trained encoder block, whether the conv stem is trained).  0 gives
    (n_audio_layer, False): no block; K gives the last K blocks; "all" every block and the stem."""
    if value == "all":
        return 0, True
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= n_audio_layer:
        raise _lib.WipaError(f"train_encoder_layers must be 0, 1..{n_audio_layer} or 'all', got {value!r}")
    return n_audio_layer - value, False


def parameter_shape(dims, name: str) -> Tuple[int, ...]:
    """shape of the tensor ``name`` (mlx_whisper's flat key names; conv weights [out, 3, in]) from the dimensions alone"""
    enc = name.startswith("encoder.")
    d = dims.n_audio_state if enc else dims.n_text_state
    leaf = name.split(".", 1)[1]
    if leaf in ("conv1.weight", "conv2.weight"):
        return (d, 3, dims.n_mels if leaf == "conv1.weight" else d)
    if leaf == "token_embedding.weight":
        return (dims.n_vocab, d)
    if leaf == "positional_embedding":
        return (dims.n_text_ctx, d)
    if leaf.endswith("mlp1.weight"):
        return (4 * d, d)
    if leaf.endswith("mlp2.weight"):
        return (d, 4 * d)
    if leaf.endswith("mlp1.bias"):
        return (4 * d,)
    return (d, d) if leaf.endswith(".weight") and "ln" not in leaf.split(".")[-2] else (d,)


def flat_layout(dims, train_encoder_layers=0) -> Dict:
    """Layout of the trainer's flat buffers from the dimensions alone: ``names`` / ``offsets`` / ``sizes`` -- every ``decoder.*``
    tensor in parameter_names order, exactly as a decoder-only trainer lays them out, then the trained ``encoder.*`` tensors in
    parameter_names order (stem, blocks, ln_post) -- and ``segments``: (label, lo, hi) of the contiguous gradient segments in the
    order the backward finishes them (and hands them to the SegmentReducer): decoder tail, decoder blocks from the last,
    decoder head, encoder.ln_post, encoder blocks from the last, stem."""
    first, stem = resolve_train_encoder_layers(train_encoder_layers, dims.n_audio_layer)
    every = parameter_names(dims)
    names = [n for n in every if n.startswith("decoder.")]

    def trained(n: str) -> bool:
        if not n.startswith("encoder."):
            return False
        part = n.split(".")
        if part[1] == "blocks":
            return int(part[2]) >= first
        return part[1] == "ln_post" if not stem else True

    if first < dims.n_audio_layer:
        names += [n for n in every if trained(n)]
    sizes = [_numel(parameter_shape(dims, n)) for n in names]
    offsets, total = {}, 0
    for n, sz in zip(names, sizes):
        offsets[n] = total
        total += sz

    def span(prefix: str) -> Tuple[int, int]:
        idx = [i for i, n in enumerate(names) if n.startswith(prefix)]
        return (offsets[names[idx[0]]], offsets[names[idx[-1]]] + sizes[idx[-1]])

    Lt = dims.n_text_layer
    dec_blocks = [span(f"decoder.blocks.{l}.") for l in range(Lt)]
    tail = span("decoder.ln.")
    segments = [("decoder.tail", *tail)] + [(f"decoder.blocks.{l}", *dec_blocks[l]) for l in reversed(range(Lt))]
    segments.append(("decoder.head", 0, dec_blocks[0][0]))
    if first < dims.n_audio_layer:
        segments.append(("encoder.ln_post", *span("encoder.ln_post.")))
        segments += [(f"encoder.blocks.{l}", *span(f"encoder.blocks.{l}.")) for l in reversed(range(first, dims.n_audio_layer))]
        if stem:
            segments.append(("encoder.stem", *span("encoder.conv")))
    return dict(names=names, sizes=sizes, offsets=offsets, total=total, segments=segments, first_block=first, stem=stem)


class DecoderTrainer:
    def __init__(self, model: Whisper, lr: float = 1e-5, max_grad_norm: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, f32_split: Optional[bool] = None, clip_scope: str = "reference",
                 train_encoder_layers=0, spec_augment=None, lora=None):
        """``lora`` (a ``lora.LoRAConfig``; default None: the trainer as it is without one, launch for launch): low-rank adapters on the
        targeted decoder linears.  The flat p / g / m / v buffers hold the adapter tensors only (``lora.adapter_layout``); the base
        tensors stay where ``model._params`` has them and are never written.  The forward adds every adapted linear's term with
        wipa_lora_fwd after its base GEMM (after the split-K sum where there is one; one call per adapted half of the fused cross
        key | value projection), the backward calls wipa_lora_bwd and computes no weight, bias or LayerNorm-parameter gradient of the
        base: the input-gradient GEMMs, attention and LayerNorm backward stay, the tied-embedding gradient, its transposes and the
        embedding scatter are skipped.  A data-parallel step all-reduces adapter bytes only.  ``clip_scope`` applies by name as it
        stands: adapter names contain a block index, so ``"reference"`` clips none of them and ``"all"`` clips each.  The feature
        cache and ``spec_augment`` work as on any decoder-only trainer.  Refused: ``train_encoder_layers != 0``, ``leaves()`` and
        ``differentiable_logits``, a step while the model has an adapter applied (Whisper.set_adapter).  ``adapter()`` /
        ``save_adapter(dir)`` / ``adapter_applied()`` are the way out.  Not built: adapters on encoder blocks or the embedding,
        dropout on the adapter path.
        ``spec_augment`` (an ``audio.SpecAugment``; default None: the step as it is without one, launch for launch): every training
        step masks the padded f32 copy of the mel it makes anyway -- the buffer of _encoder_forward, or embed_audio's on a
        decoder-only trainer -- with one launch (csrc/spec_augment.hip); the caller's mel is never modified.  Row b draws from the
        stream (clip_keys[b], step_count) when train_step is given ``clip_keys``, else (rank * B + b, step_count): no two ranks
        share a stream, and a clip draws a new mask every time it returns.  ``n_frames`` (train_step / loss_and_grads_from_mel):
        every clip's own length in frames, the time axis its masks are drawn over; under ``model.audio_ctx`` = N the axis is the
        first 2N frames.  Such a trainer refuses the feature cache and loss_and_grads(features): augmented features are not a
        function of the clip.  Nothing outside the training step augments.
        ``train_encoder_layers``: 0 (default) trains the decoder alone, the reference's step (its encoder is frozen,
        train_whisper_ipa.py:187).  K in 1..n_audio_layer also trains the last K encoder blocks and ``encoder.ln_post``;
        ``"all"`` every block, ``ln_post`` and the conv stem (``conv1.*``, ``conv2.*``).  The sinusoidal positional table of
        the encoder is never a parameter (as in mlx_whisper).  Such a trainer steps from the mel (train_step /
        loss_and_grads_from_mel): an encoder forward that keeps its activations, the decoder's forward and backward, then the
        encoder's backward.  The per-tensor clip is ``clip_reaches`` by name, as it stands: under ``clip_scope="reference"``
        ``encoder.conv*`` and ``encoder.ln_post.*`` are clipped and ``encoder.blocks.N.*`` are not (the blocks are a list, like
        the decoder's); ``"all"`` clips each tensor.  The reference has no counterpart of any non-zero value.
        ``f32_split`` (default: the model's setting -- on unless the model was built with f32_split=False): split-bf16 products in the large GEMMs of the step.
        ``clip_scope``: which tensors the per-tensor clip reaches.  ``"reference"`` (default) is ``clip_grad_dict`` as the
        reference wrote it (train_whisper_ipa.py:287-303): it recurses through dict values only, so the ``decoder.blocks``
        LIST is passed through (:299-300) and only ``token_embedding.weight``, ``positional_embedding`` and ``ln.*`` are
        clipped; ``"all"`` clips every decoder tensor by its own norm (what that function's docstring intends)."""
        if clip_scope not in CLIP_SCOPES:
            raise _lib.WipaError(f"DecoderTrainer: clip_scope {clip_scope!r}: one of {CLIP_SCOPES}")
        self.clip_scope = clip_scope
        if model.dtype != torch.float32:
            raise _lib.WipaError("DecoderTrainer: the fine-tune step runs in float32 (reference: set_dtype(mx.float32))")
        self.model, self.lr, self.max_grad_norm = model, lr, max_grad_norm
        self.b1, self.b2 = betas
        self.eps, self.wd = eps, weight_decay
        self.L = _lib.lib()
        self.f32_split = model.f32_split if f32_split is None else bool(f32_split)
        d = model.dims
        self.train_encoder_layers = train_encoder_layers
        self._enc_first, self._train_stem = resolve_train_encoder_layers(train_encoder_layers, d.n_audio_layer)
        self.trains_encoder = self._enc_first < d.n_audio_layer
        if self.trains_encoder and d.n_audio_state != d.n_text_state:
            raise _lib.WipaError("DecoderTrainer: train_encoder_layers needs an encoder as wide as the decoder")
        self.lora = lora
        if lora is not None:
            if not isinstance(lora, lora_mod.LoRAConfig):
                raise _lib.WipaError(f"DecoderTrainer: lora must be a LoRAConfig, got {type(lora).__name__}")
            if self.trains_encoder:
                raise _lib.WipaError(f"DecoderTrainer: lora together with train_encoder_layers={train_encoder_layers!r}: adapters sit on "
                                     "a frozen model (train_encoder_layers must be 0)")
            if getattr(model, "_adapter", None) is not None:
                raise _lib.WipaError("DecoderTrainer: lora on a model that has an adapter applied: set_adapter(None) first")
        self._lora_sites = frozenset(lora.sites()) if lora is not None else frozenset()
        layout = flat_layout(d, train_encoder_layers) if lora is None else lora_mod.adapter_layout(d, lora)
        self.names = layout["names"]  # decoder tensors first, as without encoder layers, then the trained encoder tensors
        self.offsets, sizes, total = layout["offsets"], layout["sizes"], layout["total"]
        # contiguous gradient segments, in the order the backward finishes them: each is all-reduced (_reduce_segment) while the
        # earlier blocks still compute
        self.segments = layout["segments"]
        self._segments_done = 0
        if lora is None:
            P = model.flat_parameters()
            self.shapes = {n: parameter_shape(d, n) for n in self.names}
        else:
            P = lora_mod.init_adapter(d, lora)
            self.shapes = {n: lora_mod.adapter_shape(d, lora, n) for n in self.names}
        assert all(tuple(P[n].shape) == self.shapes[n] for n in self.names)
        # so that every tensor starts 16-byte aligned in the flat buffers: wipa_sum_slabs writes the weight gradients there and
        # refuses any other address (the optimiser, wipa_clip_adamw, walks its chunks float by float and would not mind)
        assert all(s % 4 == 0 for s in sizes)
        self.n_params = total
        with on_stream():
            dev = model.device
            self.flat_p = torch.empty(total, dtype=torch.float32, device=dev)
            self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
            self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
            self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
            for n in self.names:
                self.p(n).copy_(P[n])
                if lora is None:
                    model._params[n] = self.p(n)  # the model now reads the optimiser's buffer directly
            # chunk tables for the flat multi-tensor optimiser
            ch_off, ch_len, ch_seg, seg_first = [], [], [], [0]
            for si, (n, s) in enumerate(zip(self.names, sizes)):
                o = self.offsets[n]
                for c0 in range(0, s, OPT_CHUNK):
                    ch_off.append(o + c0)
                    ch_len.append(min(OPT_CHUNK, s - c0))
                    ch_seg.append(si)
                seg_first.append(len(ch_off))
            self.n_chunks, self.n_seg = len(ch_off), len(sizes)
            self.ch_off = torch.tensor(ch_off, dtype=torch.int64, device=dev)
            self.ch_len = torch.tensor(ch_len, dtype=torch.int32, device=dev)
            self.ch_seg = torch.tensor(ch_seg, dtype=torch.int32, device=dev)
            self.seg_first = torch.tensor(seg_first, dtype=torch.int32, device=dev)
            self.partial = torch.empty(self.n_chunks, dtype=torch.float32, device=dev)
            self.coef = torch.empty(self.n_seg, dtype=torch.float32, device=dev)
            self.norms = torch.empty(self.n_seg, dtype=torch.float32, device=dev)
            self.seg_clip = torch.tensor([int(clip_reaches(n, clip_scope)) for n in self.names], dtype=torch.int32, device=dev)
        model._invalidate()
        self.step_count = 0
        self._colsum_ws = None  # partial sums of the chunked bias-gradient reduction (wipa_colsum)
        self._slabs = None      # split-K partial outputs (_gemm_k_sliced): one workspace, its uses are ordered on the library stream
        self._ar_events = None  # HIP events around the last step's exposed all-reduce wait (_join_reductions)
        self.feature_cache: Optional[FrozenFeatureCache] = None  # enable_feature_cache()
        self._spec_augment = None
        self.spec_augment = spec_augment
        self._leaves = None     # autograd leaves over flat_p (leaves())
        self._lora_ws = None    # wipa_lora_bwd's scratch, sized by the largest call so far
        self._ln_scratch = None  # where wipa_layernorm_bwd leaves the dw / db a LoRA trainer does not keep
        self._kv_frozen = {}    # block -> (the tensors it was made of, cross key | value weight as one [2d, d] matrix) of a LoRA trainer
        model._trainer = self   # Whisper.logits differentiates through this trainer under torch.enable_grad()

    @property
    def spec_augment(self):
        return self._spec_augment

    @spec_augment.setter
    def spec_augment(self, aug) -> None:
        if aug is not None and self.feature_cache is not None:
            raise _lib.WipaError("DecoderTrainer: spec_augment on a trainer with a feature cache: augmented features cannot be cached")
        self._spec_augment = aug

    def _augment_streams(self, B: int, clip_keys) -> List[Tuple[int, int]]:
        """row b's stream: (clip_keys[b], step_count), or (rank * B + b, step_count) without keys"""
        if clip_keys is not None:
            keys = [int(k) for k in clip_keys]
            if len(keys) != B:
                raise _lib.WipaError(f"DecoderTrainer: {len(keys)} clip_keys for {B} clips")
        else:
            rank = parallel.world()[0]
            keys = [rank * B + b for b in range(B)]
        return [(k, self.step_count) for k in keys]

    def _augment_padded(self, padded: torch.Tensor, B: int, F: int, clip_keys, n_frames) -> None:
        """mask the padded f32 mel in place: frame t of clip b at row b*(F + 2) + t + 1; halo rows are not touched"""
        n_mels = self.model.dims.n_mels
        self._spec_augment.mask_in_place(padded, n_mels, (F + 2) * n_mels, n_mels, B, F, n_mels, self._augment_streams(B, clip_keys),
                                         n_frames)

    def feature_cache_capacity_default(self) -> int:
        return FrozenFeatureCache.clips_that_fit(self.model)

    def enable_feature_cache(self, max_clips: Optional[int] = None) -> "FrozenFeatureCache":
        """Keep the frozen encoder's output per clip in HBM (FrozenFeatureCache); ``max_clips`` defaults to what half of the
        free device memory holds.  Refused by a trainer that trains encoder layers: the features then change with every step."""
        self._decoder_only("enable_feature_cache")
        if self._spec_augment is not None:
            raise _lib.WipaError("DecoderTrainer.enable_feature_cache on a trainer with spec_augment: augmented features cannot be cached")
        n = FrozenFeatureCache.clips_that_fit(self.model) if max_clips is None else int(max_clips)
        self.feature_cache = FrozenFeatureCache(self.model, max(0, n))
        return self.feature_cache

    def _decoder_only(self, what: str) -> None:
        if self.trains_encoder:
            raise _lib.WipaError(f"DecoderTrainer.{what} is decoder-only and this trainer has train_encoder_layers="
                                 f"{self.train_encoder_layers!r}: step from the mel (train_step / loss_and_grads_from_mel)")

    # ---- views into the flat buffers
    def w(self, name: str) -> torch.Tensor:
        """the weight ``name`` as the step reads it: the flat buffer's view of a trained tensor, the model's own tensor of a frozen one"""
        return self.p(name) if name in self.offsets else self.model._params[name]

    def p(self, name: str) -> torch.Tensor:
        o = self.offsets[name]
        return self.flat_p[o:o + _numel(self.shapes[name])].view(self.shapes[name])

    def g(self, name: str) -> torch.Tensor:
        o = self.offsets[name]
        return self.flat_g[o:o + _numel(self.shapes[name])].view(self.shapes[name])

    def grads(self) -> Dict[str, torch.Tensor]:
        return {n: self.g(n) for n in self.names}

    def _gw(self, name: str) -> Optional[torch.Tensor]:
        """where the backward leaves the gradient of ``name``: its view of flat_g, or None for a tensor this trainer does not train
        (every base tensor of a LoRA trainer) -- the backward then skips that gradient"""
        return self.g(name) if name in self.offsets else None

    # ---- low-rank adapters (lora=...)
    def adapter(self) -> Dict[str, torch.Tensor]:
        """name -> the current adapter tensor (a view of the flat parameter buffer)"""
        self._lora_only("adapter")
        return {n: self.p(n) for n in self.names}

    def load_adapter(self, adapter: Dict[str, torch.Tensor]) -> None:
        """overwrite the adapter tensors (e.g. with lora.load_adapter's); the optimiser moments are kept"""
        self._lora_only("load_adapter")
        lora_mod.check_adapter(self.model.dims, self.lora, adapter)
        with on_stream():
            for n in self.names:
                self.p(n).copy_(torch.as_tensor(adapter[n]).to(device=self.model.device, dtype=torch.float32))

    def save_adapter(self, directory: str, extra: Optional[Dict] = None) -> None:
        """adapter_model.safetensors + adapter_config.json (lora.save_adapter); audio_ctx is the model's"""
        self._lora_only("save_adapter")
        with on_stream():
            cpu = {n: t.detach().cpu() for n, t in self.adapter().items()}
        lora_mod.save_adapter(directory, cpu, self.lora, dict(dict(audio_ctx=self.model.audio_ctx), **(extra or {})))

    def adapter_applied(self):
        """``with trainer.adapter_applied():`` the model runs with the trainer's current adapter merged into its weights
        (Whisper.set_adapter) -- validation -- and is the base model again on exit.  No step may run inside."""
        self._lora_only("adapter_applied")
        trainer = self

        class _Applied:
            def __enter__(self):
                trainer.model.set_adapter(trainer.adapter(), trainer.lora)
                return trainer.model

            def __exit__(self, *exc):
                trainer.model.set_adapter(None)
                return False

        return _Applied()

    def _lora_only(self, what: str) -> None:
        if self.lora is None:
            raise _lib.WipaError(f"DecoderTrainer.{what} needs a trainer built with lora=LoRAConfig(...)")

    def _no_lora(self, what: str) -> None:
        if self.lora is not None:
            raise _lib.WipaError(f"DecoderTrainer.{what} on a LoRA trainer: the base tensors are no leaves here; step with train_step / "
                                 "loss_and_grads")

    def _lora_fwd(self, site: str, S: Dict, key: str, x, y, M: int, K: int, N: int, c: float = 1.0) -> None:
        """y [M, N] (row stride y.stride(0)) += c s (x A^T) B^T for the adapted linear ``site`` (decoder.blocks.l.attn.query ...); nothing
        when it carries no adapter.  ``c``: the column scale of the base linear, which the term sits inside.  Keeps u in S[key]."""
        if site.split(".", 3)[-1] not in self._lora_sites or not site.startswith("decoder."):
            return
        r = self.lora.rank
        with on_stream() as s:
            u = torch.empty(M, r, dtype=torch.float32, device=y.device)
            _lib.check(self.L.wipa_lora_fwd(ptr(x), x.stride(0), ptr(self.p(site + ".lora_A")), ptr(self.p(site + ".lora_B")), ptr(y),
                                            y.stride(0), ptr(u), M, K, N, r, float(c) * self.lora.scale, sptr(s)), "wipa_lora_fwd")
        S[key] = u

    def _lora_bwd(self, site: str, S: Dict, key: str, dy, x, dx, M: int, K: int, N: int) -> None:
        """the adapter gradients of ``site`` into flat_g, and dx += its input gradient (dx None: an input that carries none).  ``dy`` is
        the gradient of the linear BEFORE its column scale, as _lin_bwd takes it (the attention backward has multiplied dq and dk by
        QK_SCALE already), so the gain is s alone."""
        if key not in S:
            return
        r = self.lora.rank
        need = self.L.wipa_lora_workspace_bytes(M, K, N, r)
        with on_stream() as s:
            if self._lora_ws is None or self._lora_ws.numel() * 4 < need:
                self._lora_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dy.device)
            _lib.check(self.L.wipa_lora_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(S[key]), ptr(self.p(site + ".lora_A")),
                                            ptr(self.p(site + ".lora_B")), ptr(self.g(site + ".lora_A")), ptr(self.g(site + ".lora_B")),
                                            ptr(dx), 0 if dx is None else dx.stride(0), 1, M, K, N, r, self.lora.scale,
                                            ptr(self._lora_ws), self._lora_ws.numel() * 4, sptr(s)), "wipa_lora_bwd")

    def _kv_weight(self, pre: str) -> torch.Tensor:
        """cross_attn.key.weight | cross_attn.value.weight of block ``pre`` as one [2d, d] matrix: the pair's view of the flat
        parameter buffer, or for a LoRA trainer (whose base tensors lie apart) a copy made once per pair of base tensors"""
        if self.lora is None:
            return self._kv_pair(self.flat_p, pre)
        k, v = self.model._params[f"{pre}.cross_attn.key.weight"], self.model._params[f"{pre}.cross_attn.value.weight"]
        hit = self._kv_frozen.get(pre)
        if hit is None or hit[0] is not k or hit[1] is not v:
            hit = self._kv_frozen[pre] = (k, v, torch.cat([k, v]))
        return hit[2]

    # ---- kernel helpers (all on the library stream)
    def _gemm(self, *a, **kw):
        return ops.gemm(*a, f32_split=self.f32_split, **kw)

    def _lin(self, x, M, K, W, N, bias=None, scale=None, residual=None, out=None):
        """out[M,N] = (x[M,K] W[N,K]^T + bias) * scale (+ residual)"""
        out = torch.empty(x.shape[0], N, dtype=torch.float32, device=x.device) if out is None else out
        return self._mm(x, W, out, M, N, K, x.stride(0), W.stride(0), bias=bias, scale=scale, residual=residual)

    def _mm(self, A, W, out, M, N, K, lda, ldw, bias=None, scale=None, residual=None, w_trans=False):
        """out[M,N] = (A[M,K] W[N,K]^T + bias) * scale (+ residual).  The decoder's GEMMs over the B*T token rows (2048 x 768)
        are 96 tiles of 128 x 128 -- a third of the chip -- so K is cut into slices computed by separate workgroups (slabs
        summed in a fixed order, then scale / residual: wipa_sum_slabs_ex) whenever the tile grid alone leaves CUs idle."""
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        plain = out.dim() == 2 and out.shape[0] == M and out.shape[1] == N and out.is_contiguous() and (
            residual is None or (residual.is_contiguous() and residual.shape == out.shape))
        # two workgroups of this kernel fit a CU: aim at (just under) 512 of them, at least four K-steps each.  Measured on the
        # fine-tune step: 480 workgroups (5 slices of a 96-tile GEMM) 144.9 ms, 288 (3 slices) 147.1, 768 (8 slices) 148.1
        slices = max(1, min(16, 512 // max(tiles, 1), K // 128)) if M >= 512 and plain else 1
        return self._gemm_k_sliced(A, W, out, M, N, K, lda, ldw, slices, bias, scale, residual, epilogue=True, w_trans=w_trans)

    def _gemm_k_sliced(self, A, W, out, M, N, K, lda, ldw, slices, bias=None, scale=None, residual=None, epilogue=False, **trans):
        """out[M,N] = (A W^T + bias) * scale (+ residual) with K cut into ``slices`` (the caller's rule; more than one needs a
        contiguous ``out``): wipa_gemm writes one [M, N] slab per slice into the shared workspace and one more launch sums them
        in a fixed order -- wipa_sum_slabs, or wipa_sum_slabs_ex with scale and residual under ``epilogue``.  One slice: the plain
        GEMM with everything in its own epilogue."""
        if slices <= 1:
            return self._gemm(A, W, out, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=out.stride(0), bias=bias, residual=residual,
                              col_scale_n=(N if scale is not None else 0), col_scale=(scale or 1.0), **trans)
        if self._slabs is None or self._slabs.numel() < slices * M * N:
            self._slabs = torch.empty(slices * M * N, dtype=torch.float32, device=out.device)
        self._gemm(A, W, self._slabs, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=N, bias=bias, k_slices=slices, slab_stride=M * N, **trans)
        with on_stream() as s:
            if epilogue:
                _lib.check(self.L.wipa_sum_slabs_ex(ptr(self._slabs), slices, M * N, ptr(out), M * N, ptr(residual),
                                                    float(scale) if scale is not None else 1.0, sptr(s)), "wipa_sum_slabs_ex")
            else:
                _lib.check(self.L.wipa_sum_slabs(ptr(self._slabs), slices, M * N, ptr(out), M * N, 0, sptr(s)), "wipa_sum_slabs")
        return out

    def _transpose(self, a, rows, cols, rows_pad):
        """a[rows, cols] (row stride a.stride(0)) -> [cols, rows_pad] with zero padding"""
        out = torch.empty(cols, rows_pad, dtype=a.dtype, device=a.device)
        with on_stream() as s:
            _lib.check(self.L.wipa_transpose(ptr(a), a.stride(0), ptr(out), rows_pad, rows, cols, rows_pad, 0, sptr(s)),
                       "wipa_transpose")
        return out

    def _lin_bwd(self, dy, M, N, x, xT, K, W, dW, db=None, dx=None, accumulate_dx=False, need_dx=True):
        """y = x W^T + b:  dx (+)= dy W ; dW = dy^T x ; db = colsum(dy).
        dy [M(+pad), N], x [M, K]; xT = transpose(x) [K, Mp] may be passed to share it between linears."""
        Mp = _ceil(M, 32)
        out_dx = None
        # wipa_gemm reads K-major operands (a_trans / w_trans): W as it is stored is the K-major form of W^T, dy and x as they
        # are stored are the K-major forms of dy^T and x^T -- no transposed copies.  Needs whole 32-float K-steps and row
        # counts that are multiples of 4; anything else takes the transposing path.
        kmajor = M % 32 == 0 and N % 32 == 0 and K % 4 == 0 and W.stride(1) == 1 and dy.stride(1) == 1 and x.stride(1) == 1
        if need_dx:
            out_dx = dx if dx is not None else torch.empty(dy.shape[0], K, dtype=torch.float32, device=dy.device)
            if kmajor:
                self._mm(dy, W, out_dx, M, K, N, dy.stride(0), W.stride(0), residual=(out_dx if accumulate_dx else None), w_trans=True)
            else:
                Np = _ceil(N, 32)
                WT = self._transpose(W, N, K, Np)  # [K, Np]
                # contraction over n: A = dy (row stride ld, first Np columns must be readable and zero beyond N)
                self._mm(dy, WT, out_dx, M, K, Np, dy.stride(0), Np, residual=(out_dx if accumulate_dx else None))
        if dW is None:  # a frozen weight (the base of a LoRA trainer): no weight gradient, no bias gradient
            return out_dx
        if kmajor:
            A_op, W_op, lda, ldw, Kc, flags = dy, x, dy.stride(0), x.stride(0), M, dict(a_trans=True, w_trans=True)
        else:
            dyT = self._transpose(dy, M, N, Mp)  # [N, Mp]
            if xT is None:
                xT = self._transpose(x, M, K, Mp)
            A_op, W_op, lda, ldw, Kc, flags = dyT, xT, Mp, xT.stride(0), Mp, {}
        # weight gradient: small [N, K] output, contraction over all M tokens.  When the tile grid alone cannot fill the
        # chip (768 x 768 over 48 000 encoder positions is 36 tiles), K is split into slabs that are summed in order.
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        slices = max(1, min(16, 512 // tiles, (Mp // 32) // 8)) if dW.is_contiguous() else 1
        self._gemm_k_sliced(A_op, W_op, dW, N, K, Kc, lda, ldw, slices, **flags)
        if db is not None:
            self._colsum(dy, M, N, db)
        return out_dx

    def _kv_pair(self, flat: torch.Tensor, pre: str) -> torch.Tensor:
        """cross_attn.key.weight | cross_attn.value.weight of block ``pre`` as one [2d, d] matrix of a flat buffer"""
        d = self.model.dims.n_text_state
        o = self.offsets[f"{pre}.cross_attn.key.weight"]
        assert self.offsets[f"{pre}.cross_attn.value.weight"] == o + d * d
        return flat[o:o + 2 * d * d].view(2 * d, d)

    def _colsum(self, dy, M, N, db):
        with on_stream() as s:
            if self._colsum_ws is None:
                self._colsum_ws = torch.empty(64 * 4 * self.model.dims.n_text_state, dtype=torch.float32, device=dy.device)
            _lib.check(self.L.wipa_colsum(ptr(dy), dy.stride(0), M, N, ptr(db), 0, ptr(self._colsum_ws), self._colsum_ws.numel(),
                                          sptr(s)), "wipa_colsum")

    def _wgrad_rows(self, dy, x, ldx, Kc, n_out, n_in, dW):
        """dW[n_out, n_in] = sum over the Kc rows r of dy[r, :n_out]^T x[r*ldx : r*ldx + n_in]: the weight gradient of a
        convolution run as a GEMM over OVERLAPPING rows (ldx < n_in; conv1: ldx = n_mels, conv2: ldx = 2d), both operands read
        K-major in place -- no im2col copy.  Kc a multiple of 32; rows of dy that stand for no output (the halo rows of each
        clip, the padding up to Kc) must be zero, x readable and finite over all Kc rows."""
        tiles = ((n_out + 127) // 128) * ((n_in + 127) // 128)
        slices = max(1, min(16, 512 // tiles, (Kc // 32) // 8))
        self._gemm_k_sliced(dy, x, dW, n_out, n_in, Kc, dy.stride(0), ldx, slices, a_trans=True, w_trans=True)

    def _ln(self, x, w, b):
        return ops.layernorm(x, w, b, out_dtype=torch.float32)

    def _ln_bwd(self, x, dy, w, dx, accumulate, dw, db, M, D):
        with on_stream() as s:
            if dw is None:  # a frozen LayerNorm (LoRA trainer): the kernel's dw / db go to a scratch nobody reads
                if self._ln_scratch is None or self._ln_scratch.numel() < 2 * D:
                    self._ln_scratch = torch.empty(2 * D, dtype=torch.float32, device=x.device)
                dw, db = self._ln_scratch[:D], self._ln_scratch[D:2 * D]
            stats = torch.empty(2 * M + 64 * D, dtype=torch.float32, device=x.device)  # (mean, rstd) + chunked dw / db partials
            _lib.check(self.L.wipa_layernorm_bwd(ptr(x), ptr(dy), ptr(w), ptr(dx), int(accumulate), ptr(dw), ptr(db), ptr(stats),
                                                 stats.numel(), M, D, 1e-5, sptr(s)), "wipa_layernorm_bwd")

    def _attn(self, q, k, v, B, H, Tq, Tk, causal):
        """q [B*Tq, d], k/v [B*Tk, d] row-major -> (out [B*Tq, d], lse [B,H,Tq], desc)"""
        d = H * 64
        with on_stream() as s:
            out = torch.empty(B * Tq, d, dtype=torch.float32, device=q.device)
            lse = torch.empty(B, H, Tq, dtype=torch.float32, device=q.device)
            a = _lib.AttnDesc()
            a.q, a.k, a.v, a.out, a.lse = ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse)
            a.q_bs, a.q_rs, a.q_hs = Tq * q.stride(0), q.stride(0), 64
            a.k_bs, a.k_rs, a.k_hs = Tk * k.stride(0), k.stride(0), 64
            a.v_bs, a.v_rs, a.v_hs = Tk * v.stride(0), v.stride(0), 64
            a.o_bs, a.o_rs, a.o_hs = Tq * d, d, 64
            a.B, a.H, a.Tq, a.Tk, a.causal, a.dtype = B, H, Tq, Tk, int(causal), 0
            _lib.check(self.L.wipa_attention(C.byref(a), sptr(s)), "wipa_attention")
        return out, lse, a

    def _attn_bwd(self, desc, out, d_out, lse, dq, dk, dv, split: bool = False):
        """``split``: the split-product kernels (wipa_attention_bwd_ex, f32_split = 1) -- the encoder's self-attention of a trainer
        with f32_split; the decoder's calls keep the exact kernels"""
        with on_stream() as s:
            dvec = torch.empty_like(lse)
            if split:
                _lib.check(self.L.wipa_attention_bwd_ex(C.byref(desc), ptr(out), ptr(d_out), ptr(lse), ptr(dq), ptr(dk), ptr(dv),
                                                        ptr(dvec), QK_SCALE, 1, sptr(s)), "wipa_attention_bwd_ex")
                return
            _lib.check(self.L.wipa_attention_bwd(C.byref(desc), ptr(out), ptr(d_out), ptr(lse), ptr(dq), ptr(dk), ptr(dv),
                                                 ptr(dvec), QK_SCALE, sptr(s)), "wipa_attention_bwd")

    # ---- forward + backward ------------------------------------------------------------
    def _self_attn_fwd(self, pre: str, S: Dict, x: torch.Tensor, B: int, T: int, H: int, causal: bool) -> torch.Tensor:
        """the self-attention half of block ``pre`` (decoder or encoder) on x [B*T, d]: LayerNorm, q, k, v, attention, out +
        residual.  Fills what _self_attn_bwd reads (x_a, h1, q, k, v, a, lse1, desc1) and returns x_b."""
        W = self.w
        M, d = B * T, H * 64
        S["x_a"] = x
        S["h1"] = self._ln(x, W(f"{pre}.attn_ln.weight"), W(f"{pre}.attn_ln.bias"))
        S["q"] = self._lin(S["h1"], M, d, W(f"{pre}.attn.query.weight"), d, W(f"{pre}.attn.query.bias"), QK_SCALE)
        S["k"] = self._lin(S["h1"], M, d, W(f"{pre}.attn.key.weight"), d, None, QK_SCALE)
        S["v"] = self._lin(S["h1"], M, d, W(f"{pre}.attn.value.weight"), d, W(f"{pre}.attn.value.bias"))
        if self._lora_sites:
            self._lora_fwd(f"{pre}.attn.query", S, "u_q", S["h1"], S["q"], M, d, d, QK_SCALE)
            self._lora_fwd(f"{pre}.attn.key", S, "u_k", S["h1"], S["k"], M, d, d, QK_SCALE)
            self._lora_fwd(f"{pre}.attn.value", S, "u_v", S["h1"], S["v"], M, d, d)
        S["a"], S["lse1"], S["desc1"] = self._attn(S["q"], S["k"], S["v"], B, H, T, T, causal)
        x_b = self._lin(S["a"], M, d, W(f"{pre}.attn.out.weight"), d, W(f"{pre}.attn.out.bias"), residual=x)
        if self._lora_sites:
            self._lora_fwd(f"{pre}.attn.out", S, "u_o", S["a"], x_b, M, d, d)
        return x_b

    def _mlp_fwd(self, pre: str, S: Dict, x_c: torch.Tensor) -> torch.Tensor:
        """the MLP half of block ``pre`` (decoder or encoder) on x_c [M, d]: LayerNorm, mlp1, GELU, mlp2 + residual.  Fills what
        _mlp_bwd reads (x_c, h3, z, u) and returns the block's output."""
        W = self.w
        M, d = x_c.shape
        S["x_c"] = x_c
        S["h3"] = self._ln(x_c, W(f"{pre}.mlp_ln.weight"), W(f"{pre}.mlp_ln.bias"))
        S["z"] = self._lin(S["h3"], M, d, W(f"{pre}.mlp1.weight"), 4 * d, W(f"{pre}.mlp1.bias"))
        if self._lora_sites:
            self._lora_fwd(f"{pre}.mlp1", S, "u_m1", S["h3"], S["z"], M, d, 4 * d)
        S["u"] = torch.empty_like(S["z"])
        with on_stream() as s:
            _lib.check(self.L.wipa_gelu(ptr(S["z"]), ptr(S["u"]), S["z"].numel(), sptr(s)), "wipa_gelu")
        x_next = self._lin(S["u"], M, 4 * d, W(f"{pre}.mlp2.weight"), d, W(f"{pre}.mlp2.bias"), residual=x_c)
        if self._lora_sites:
            self._lora_fwd(f"{pre}.mlp2", S, "u_m2", S["u"], x_next, M, 4 * d, d)
        return x_next

    def _forward(self, audio_features: torch.Tensor, tok_in: torch.Tensor):
        """Teacher-forced decoder on ``tok_in`` [B, T] int32 (device, contiguous) and features [B, 1500, d]: returns the
        zero-padded logits [ceil32(B*T), ceil32(V)] f32 and the saved activations the backward needs."""
        m, dm, L = self.model, self.model.dims, self.L
        P = self.w  # every decoder tensor is in the flat buffer (self.p) unless this is a LoRA trainer, whose base is the model's own
        B, T = tok_in.shape
        d, H, V, Ta = dm.n_text_state, dm.n_text_head, dm.n_vocab, self.model.n_audio_ctx
        M, Mp = B * T, _ceil(B * T, 32)
        Vp = _ceil(V, 32)
        if tuple(audio_features.shape) != (B, Ta, d):  # Ta: the positions the model runs on (model.audio_ctx)
            raise _lib.WipaError(f"DecoderTrainer: audio features of shape {tuple(audio_features.shape)}, expected {(B, Ta, d)} "
                                 f"(audio_ctx={m.audio_ctx!r})")
        with on_stream() as s:
            dev = m.device
            feats = audio_features.to(device=dev, dtype=torch.float32).contiguous().view(B * Ta, d)
            # [d, ceil32(B*Ta)], shared by all layers; not needed when the weight-gradient GEMM reads feats K-major
            # (nor by a LoRA trainer, which has no such GEMM)
            featsT = None if (B * Ta) % 32 == 0 or self.lora is not None else self._transpose(feats, B * Ta, d, _ceil(B * Ta, 32))
            x = torch.empty(M, d, dtype=torch.float32, device=dev)
            _lib.check(L.wipa_embed_tokens(ptr(tok_in), T, B, T, 0, None, ptr(P("decoder.token_embedding.weight")), 0, None,
                                           ptr(P("decoder.positional_embedding")), ptr(x), d, sptr(s)), "wipa_embed_tokens")
            saved = []
            for l in range(dm.n_text_layer):
                pre = f"decoder.blocks.{l}"
                S = {}
                S["x_b"] = self._self_attn_fwd(pre, S, x, B, T, H, causal=True)
                S["h2"] = self._ln(S["x_b"], P(f"{pre}.cross_attn_ln.weight"), P(f"{pre}.cross_attn_ln.bias"))
                S["qc"] = self._lin(S["h2"], M, d, P(f"{pre}.cross_attn.query.weight"), d, P(f"{pre}.cross_attn.query.bias"), QK_SCALE)
                if self._lora_sites:
                    self._lora_fwd(f"{pre}.cross_attn.query", S, "u_qc", S["h2"], S["qc"], M, d, d, QK_SCALE)
                # cross key | value as ONE projection over the B*1500 encoder rows: key.weight and value.weight are adjacent in
                # the flat parameter buffer, i.e. one [2d, d] matrix (grid of 750 instead of two of 375 tiles: 2.9 rounds on
                # the 256 CUs instead of 1.5 twice); the key half is scaled in the epilogue, the value half carries its bias
                kv = torch.empty(B * Ta, 2 * d, dtype=torch.float32, device=dev)
                bkv = torch.cat([torch.zeros_like(P(f"{pre}.cross_attn.value.bias")), P(f"{pre}.cross_attn.value.bias")])
                self._gemm(feats, self._kv_weight(pre), kv, M=B * Ta, N=2 * d, K=d, lda=d, ldw=d, ldc=2 * d, bias=bkv,
                           col_scale_n=d, col_scale=QK_SCALE)
                S["kc"], S["vc"] = kv[:, :d], kv[:, d:]
                if self._lora_sites:  # one call per adapted half, on the half's strided view of kv
                    self._lora_fwd(f"{pre}.cross_attn.key", S, "u_kc", feats, S["kc"], B * Ta, d, d, QK_SCALE)
                    self._lora_fwd(f"{pre}.cross_attn.value", S, "u_vc", feats, S["vc"], B * Ta, d, d)
                S["c"], S["lse2"], S["desc2"] = self._attn(S["qc"], S["kc"], S["vc"], B, H, T, Ta, False)
                x_c = self._lin(S["c"], M, d, P(f"{pre}.cross_attn.out.weight"), d, P(f"{pre}.cross_attn.out.bias"), residual=S["x_b"])
                if self._lora_sites:
                    self._lora_fwd(f"{pre}.cross_attn.out", S, "u_oc", S["c"], x_c, M, d, d)
                x = self._mlp_fwd(pre, S, x_c)
                saved.append(S)
            x_L = x
            hf = self._ln(x_L, P("decoder.ln.weight"), P("decoder.ln.bias"))
            E = P("decoder.token_embedding.weight")
            logits = torch.zeros(Mp, Vp, dtype=torch.float32, device=dev)  # padding rows/cols stay zero
            self._gemm(hf, E, logits, M=M, N=V, K=d, lda=d, ldw=d, ldc=Vp)
        ctx = dict(saved=saved, x_L=x_L, hf=hf, feats=feats, featsT=featsT, tok_in=tok_in, B=B, T=T)
        return logits, ctx

    def _new_reducer(self, group) -> "parallel.SegmentReducer":
        """the reducer of one backward over self.flat_g, no segment handed over yet"""
        self._segments_done = 0
        return parallel.SegmentReducer(self.flat_g, group)

    def _reduce_segment(self, reducer, label: str) -> None:
        """Hand the finished gradient segment ``label`` of self.segments to ``reducer``.  DP: it is all-reduced (SUM; every rank
        already divided by the GLOBAL count) asynchronously on RCCL's stream while the earlier blocks are still in their
        backward.  The backward finishes the segments in flat_layout's order, nothing else."""
        i = self._segments_done
        due = self.segments[i][0] if i < len(self.segments) else None
        if label != due:
            raise _lib.WipaError(f"DecoderTrainer: the backward finished gradient segment {label!r} where flat_layout has {due!r} next")
        self._segments_done = i + 1
        reducer.reduce(*self.segments[i][1:])

    def _backward(self, ctx: Dict, dlogits: torch.Tensor, reducer, d_feats: Optional[torch.Tensor] = None) -> None:
        """Reverse pass from ``dlogits`` [ceil32(B*T), ceil32(V)] f32 (zero in the padding; consumed) into self.flat_g: the
        gradient of every ``decoder.*`` tensor, tied embedding included.  Every finished segment goes to ``reducer``
        (_reduce_segment), which the caller made (_new_reducer) and joins (_join_reductions).
        ``d_feats`` [B*N, d] (trainers that train encoder layers): receives the gradient of the encoder output, summed over the
        decoder layers in the order the backward visits them."""
        m, dm, L = self.model, self.model.dims, self.L
        P, G = self.w, self._gw  # G gives None for a tensor that is not trained (a LoRA trainer's base): that gradient is skipped
        lora = self.lora is not None
        saved, x_L, hf, feats, featsT, tok_in = ctx["saved"], ctx["x_L"], ctx["hf"], ctx["feats"], ctx["featsT"], ctx["tok_in"]
        B, T = ctx["B"], ctx["T"]
        d, H, V, Ta = dm.n_text_state, dm.n_text_head, dm.n_vocab, self.model.n_audio_ctx
        M, Mp = B * T, _ceil(B * T, 32)
        Vp = _ceil(V, 32)
        with on_stream() as s:
            dev = m.device
            self.flat_g.zero_()
            E = P("decoder.token_embedding.weight")
            # logits = hf E^T : dhf = dlogits E ; dE = dlogits^T hf
            ET = self._transpose(E, V, d, Vp)  # [d, Vp]
            dhf = torch.empty(M, d, dtype=torch.float32, device=dev)
            self._mm(dlogits, ET, dhf, M, d, Vp, Vp, Vp)  # 96 tiles over a 51 872-long contraction: eight K slices
            if not lora:  # the embedding is frozen under LoRA: no dE GEMM and neither of its transposes
                dlT = self._transpose(dlogits, M, V, Mp)  # [V, Mp]
                hfT = self._transpose(hf, M, d, Mp)
                self._gemm(dlT, hfT, G("decoder.token_embedding.weight"), M=V, N=d, K=Mp, lda=Mp, ldw=Mp, ldc=d)
                del dlT
            del dlogits
            dx = torch.empty(M, d, dtype=torch.float32, device=dev)
            self._ln_bwd(x_L, dhf, P("decoder.ln.weight"), dx, False, G("decoder.ln.weight"), G("decoder.ln.bias"), M, d)
            if not lora:
                self._reduce_segment(reducer, "decoder.tail")
            for l in reversed(range(dm.n_text_layer)):
                pre = f"decoder.blocks.{l}"
                S = saved[l]
                self._mlp_bwd(pre, S, dx, M, d)
                # x_c = x_b + c Wco^T + bco
                dc = self._lin_bwd(dx, M, d, S["c"], None, d, P(f"{pre}.cross_attn.out.weight"), G(f"{pre}.cross_attn.out.weight"),
                                   G(f"{pre}.cross_attn.out.bias"))
                if lora:
                    self._lora_bwd(f"{pre}.cross_attn.out", S, "u_oc", dx, S["c"], dc, M, d, d)
                dqc = torch.empty(M, d, dtype=torch.float32, device=dev)
                dkv = torch.empty(B * Ta, 2 * d, dtype=torch.float32, device=dev)  # d(key) | d(value), strides of the forward's kv
                dkc, dvc = dkv[:, :d], dkv[:, d:]
                self._attn_bwd(S["desc2"], S["c"], dc, S["lse2"], dqc, dkc, dvc)
                # one weight-gradient GEMM for the [2d, d] pair, value bias apart.  Its input gradient is the encoder output's: none
                # while the encoder is frozen; else the last decoder layer writes d_feats and the others add
                if not lora:
                    self._lin_bwd(dkv, B * Ta, 2 * d, feats, featsT, d, self._kv_pair(self.flat_p, pre), self._kv_pair(self.flat_g, pre),
                                  None, dx=d_feats, accumulate_dx=(l != dm.n_text_layer - 1), need_dx=d_feats is not None)
                    self._colsum(dvc, B * Ta, d, G(f"{pre}.cross_attn.value.bias"))
                else:  # the input of these two is the frozen encoder output: adapter gradients only, no dx
                    self._lora_bwd(f"{pre}.cross_attn.key", S, "u_kc", dkc, feats, None, B * Ta, d, d)
                    self._lora_bwd(f"{pre}.cross_attn.value", S, "u_vc", dvc, feats, None, B * Ta, d, d)
                del dkv, dkc, dvc
                dh2 = self._lin_bwd(dqc, M, d, S["h2"], None, d, P(f"{pre}.cross_attn.query.weight"), G(f"{pre}.cross_attn.query.weight"),
                                    G(f"{pre}.cross_attn.query.bias"))
                if lora:
                    self._lora_bwd(f"{pre}.cross_attn.query", S, "u_qc", dqc, S["h2"], dh2, M, d, d)
                self._ln_bwd(S["x_b"], dh2, P(f"{pre}.cross_attn_ln.weight"), dx, True, G(f"{pre}.cross_attn_ln.weight"),
                             G(f"{pre}.cross_attn_ln.bias"), M, d)
                self._self_attn_bwd(pre, S, dx, B, M, Mp, d)
                saved[l] = None
                self._reduce_segment(reducer, pre)
            if lora:  # no embedding scatter, no head segment: adapter_layout ends with block 0
                return
            _lib.check(L.wipa_embed_bwd(ptr(tok_in), ptr(dx), B, T, d, ptr(G("decoder.token_embedding.weight")),
                                        ptr(G("decoder.positional_embedding")), sptr(s)), "wipa_embed_bwd")
            if T < dm.n_text_ctx:
                G("decoder.positional_embedding")[T:].zero_()
            self._reduce_segment(reducer, "decoder.head")

    def _join_reductions(self, reducer, s) -> None:
        """wait for every segment's all-reduce on the compute stream ``s``: the time it stalls here is the all-reduce time the
        backward did NOT hide (last_allreduce_exposed_ms)"""
        self._ar_events = None
        if self._segments_done != len(self.segments):
            raise _lib.WipaError(f"DecoderTrainer: the backward finished {self._segments_done} of {len(self.segments)} gradient segments")
        if reducer.pending:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            reducer.wait()
            e1.record(s)
            self._ar_events = (e0, e1)

    def _mlp_bwd(self, pre: str, S: Dict, dx: torch.Tensor, M: int, d: int) -> None:
        """the MLP half of block ``pre`` (decoder or encoder), x_next = x_c + u W2^T + b2: its parameter gradients, and dx += the
        gradient through mlp_ln"""
        P, G = self.w, self._gw
        du = self._lin_bwd(dx, M, d, S["u"], None, 4 * d, P(f"{pre}.mlp2.weight"), G(f"{pre}.mlp2.weight"), G(f"{pre}.mlp2.bias"))
        self._lora_bwd(f"{pre}.mlp2", S, "u_m2", dx, S["u"], du, M, 4 * d, d)
        dz = torch.empty_like(du)
        with on_stream() as s:
            _lib.check(self.L.wipa_gelu_bwd(ptr(S["z"]), ptr(du), ptr(dz), dz.numel(), sptr(s)), "wipa_gelu_bwd")
        dh3 = self._lin_bwd(dz, M, 4 * d, S["h3"], None, d, P(f"{pre}.mlp1.weight"), G(f"{pre}.mlp1.weight"), G(f"{pre}.mlp1.bias"))
        self._lora_bwd(f"{pre}.mlp1", S, "u_m1", dz, S["h3"], dh3, M, d, 4 * d)
        self._ln_bwd(S["x_c"], dh3, P(f"{pre}.mlp_ln.weight"), dx, True, G(f"{pre}.mlp_ln.weight"), G(f"{pre}.mlp_ln.bias"), M, d)

    def _self_attn_bwd(self, pre: str, S: Dict, dx: torch.Tensor, B: int, M: int, Mp: int, d: int, split: bool = False) -> None:
        """the self-attention half of block ``pre`` (decoder or encoder), x_b = x_a + a Wo^T + bo: its parameter gradients, and
        dx += the gradient through attn_ln"""
        P, G = self.w, self._gw
        dev = dx.device
        da = self._lin_bwd(dx, M, d, S["a"], None, d, P(f"{pre}.attn.out.weight"), G(f"{pre}.attn.out.weight"), G(f"{pre}.attn.out.bias"))
        self._lora_bwd(f"{pre}.attn.out", S, "u_o", dx, S["a"], da, M, d, d)
        dq = torch.empty(M, d, dtype=torch.float32, device=dev)
        dk = torch.empty(M, d, dtype=torch.float32, device=dev)
        dv = torch.empty(M, d, dtype=torch.float32, device=dev)
        self._attn_bwd(S["desc1"], S["a"], da, S["lse1"], dq, dk, dv, split)
        h1T = None if M % 32 == 0 else self._transpose(S["h1"], M, d, Mp)  # shared by the three projections
        dh1 = self._lin_bwd(dq, M, d, S["h1"], h1T, d, P(f"{pre}.attn.query.weight"), G(f"{pre}.attn.query.weight"),
                            G(f"{pre}.attn.query.bias"))
        self._lin_bwd(dk, M, d, S["h1"], h1T, d, P(f"{pre}.attn.key.weight"), G(f"{pre}.attn.key.weight"), None, dx=dh1,
                      accumulate_dx=True)
        self._lin_bwd(dv, M, d, S["h1"], h1T, d, P(f"{pre}.attn.value.weight"), G(f"{pre}.attn.value.weight"),
                      G(f"{pre}.attn.value.bias"), dx=dh1, accumulate_dx=True)
        self._lora_bwd(f"{pre}.attn.query", S, "u_q", dq, S["h1"], dh1, M, d, d)
        self._lora_bwd(f"{pre}.attn.key", S, "u_k", dk, S["h1"], dh1, M, d, d)
        self._lora_bwd(f"{pre}.attn.value", S, "u_v", dv, S["h1"], dh1, M, d, d)
        self._ln_bwd(S["x_a"], dh1, P(f"{pre}.attn_ln.weight"), dx, True, G(f"{pre}.attn_ln.weight"), G(f"{pre}.attn_ln.bias"), M, d)

    # ---- encoder: training forward (keeps activations) + backward -----------------------------
    def _encoder_forward(self, mel: torch.Tensor, clip_keys=None, n_frames=None):
        """AudioEncoder.__call__ in f32 on a mel [B, 3000, n_mels] (or [B, 2N, n_mels] with ``model.audio_ctx`` = N), composed
        from the per-kernel entry points like the decoder's _forward: conv1 and conv2 as GEMMs over overlapping rows of the
        padded layouts wipa_encoder_forward uses (their PRE-GELU values kept), then per block the two halves the decoder's blocks
        have as well (_self_attn_fwd, non-causal, and _mlp_fwd), then ln_post.  Blocks below
        the first trained one are not saved (their buffers go back to the allocator as the walk leaves them), and the stem's
        only under "all".  Returns (features [B, N, d], what _encoder_backward needs)."""
        m, dm, L = self.model, self.model.dims, self.L
        W = self.w
        d, H, N, n_mels = dm.n_audio_state, dm.n_audio_head, m.n_audio_ctx, dm.n_mels
        if mel.dim() == 2:
            mel = mel[None]
        B, F = mel.shape[0], 2 * N
        full = 2 * dm.n_audio_ctx
        if mel.shape[1] not in (full, F) or mel.shape[2] != n_mels:
            raise _lib.WipaError(f"DecoderTrainer: a mel of shape {tuple(mel.shape)}, expected [B, {full}, {n_mels}]"
                                 + (f" or [B, {F}, {n_mels}] (audio_ctx={m.audio_ctx})" if F != full else ""))
        M, K1 = B * N, _ceil(3 * n_mels, 32)
        rows = _stem_rows(B, N)
        R, M1, M2 = rows.R, rows.M1, rows.M2
        with on_stream() as s:
            dev = m.device
            mel32 = mel.to(device=dev, dtype=torch.float32).contiguous()
            padded = torch.zeros(rows.padded, n_mels, dtype=torch.float32, device=dev)  # frame t of clip b at row b*R + t + 1
            _lib.check(L.wipa_mel_pad_cast_frames(ptr(mel32), mel32.shape[1] * n_mels, B, n_mels, F, ptr(padded), 0, sptr(s)),
                       "wipa_mel_pad_cast_frames")
            if self._spec_augment is not None:
                self._augment_padded(padded, B, F, clip_keys, n_frames)
            w1 = torch.zeros(d, K1, dtype=torch.float32, device=dev)  # K padded to whole 32-float steps with zero columns
            w1[:, : 3 * n_mels].copy_(W("encoder.conv1.weight").reshape(d, 3 * n_mels))
            # conv1 (k3, p1), pre-activation: GEMM row g = b*R + t reads the padded rows g..g+2 and lands at row g + 1; the two
            # dead rows of each clip are written as zero -- gelu(0) = 0, so one GELU over the buffer leaves conv2's halos zero
            z1 = torch.zeros(rows.z1, d, dtype=torch.float32, device=dev)
            self._gemm(padded, w1, z1, M=M1, N=d, K=K1, lda=n_mels, ldw=K1, ldc=d, bias=W("encoder.conv1.bias"), rg_in=R, rg_valid=F,
                       rg_stride=R * d, c_offset=d, zero_invalid_rows=True)
            c1 = torch.empty_like(z1)
            _lib.check(L.wipa_gelu(ptr(z1), ptr(c1), z1.numel(), sptr(s)), "wipa_gelu")
            # conv2 (k3, s2, p1), pre-activation: row b*(N+1) + t reads c1 rows 2t..2t+2 of clip b (row N of each group is dead)
            z2 = torch.empty(M, d, dtype=torch.float32, device=dev)
            self._gemm(c1, W("encoder.conv2.weight").reshape(d, 3 * d), z2, M=M2, N=d, K=3 * d, lda=2 * d, ldw=3 * d, ldc=d,
                       bias=W("encoder.conv2.bias"), rg_in=N + 1, rg_valid=N, rg_stride=N * d)
            x = torch.empty(M, d, dtype=torch.float32, device=dev)
            _lib.check(L.wipa_conv_stem_gelu_pos(ptr(z2), ptr(m._enc_pos), ptr(x), B, N, d, sptr(s)), "wipa_conv_stem_gelu_pos")
            stem = dict(padded=padded, z1=z1, c1=c1, z2=z2) if self._train_stem else None
            del padded, z1, c1, z2, w1
            saved = {}
            for l in range(dm.n_audio_layer):
                pre = f"encoder.blocks.{l}"
                S = {}
                x = self._mlp_fwd(pre, S, self._self_attn_fwd(pre, S, x, B, N, H, causal=False))
                if l >= self._enc_first:
                    saved[l] = S
                del S  # of a block that is not trained: its buffers go back to the allocator here
            feats = self._ln(x, W("encoder.ln_post.weight"), W("encoder.ln_post.bias"))
        return feats.view(B, N, d), dict(saved=saved, x_L=x, stem=stem, B=B, N=N)

    def _encoder_backward(self, ectx: Dict, d_feats: torch.Tensor, reducer) -> None:
        """From ``d_feats`` [B*N, d], the gradient of the encoder output (consumed), into self.flat_g: ln_post, the trained
        blocks from the last (the halves the decoder's blocks share: _mlp_bwd, _self_attn_bwd), then the stem under "all".  The
        walk stops after the first trained block.  Every finished segment goes to ``reducer`` like the decoder's."""
        dm = self.model.dims
        P, G = self.w, self.g
        saved, x_L, B, N = ectx["saved"], ectx["x_L"], ectx["B"], ectx["N"]
        d = dm.n_audio_state
        M, Mp = B * N, _ceil(B * N, 32)
        with on_stream():
            dx = torch.empty(M, d, dtype=torch.float32, device=d_feats.device)
            self._ln_bwd(x_L, d_feats, P("encoder.ln_post.weight"), dx, False, G("encoder.ln_post.weight"), G("encoder.ln_post.bias"), M, d)
            self._reduce_segment(reducer, "encoder.ln_post")
            for l in reversed(range(self._enc_first, dm.n_audio_layer)):
                pre = f"encoder.blocks.{l}"
                S = saved[l]
                self._mlp_bwd(pre, S, dx, M, d)
                # an f32_split trainer takes the split-product attention kernels here: faster at encoder shapes, the A/B against the
                # exact kernels is in profiles/encoder_train_bench.txt
                self._self_attn_bwd(pre, S, dx, B, M, Mp, d, split=self.f32_split)
                saved[l] = None
                del S
                self._reduce_segment(reducer, pre)
            if self._train_stem:
                self._stem_backward(ectx["stem"], dx, B, N)
                self._reduce_segment(reducer, "encoder.stem")

    def _stem_backward(self, stem: Dict, dx: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """conv2 and conv1 from ``dx`` [B*N, d], the gradient of the stem's output x = gelu(z2) + positional table (the table is
        no parameter).  Weight gradients: K-major GEMMs over the overlapping-row views of the padded inputs (_wgrad_rows), the
        dead rows of each clip carrying zero gradient; biases: wipa_colsum; conv2's input gradient: dz2 W2 as three taps per
        position, folded onto the 2N conv1 frames and through conv1's GELU by wipa_conv2_dx.  conv1 needs no input gradient.
        Returns dz1, the gradient of conv1's pre-activation in the rows of conv1's GEMM (frame s of clip b at row b*(2N + 2) + s)."""
        dm, L = self.model.dims, self.L
        P, G = self.w, self.g
        d, n_mels = dm.n_audio_state, dm.n_mels
        M = B * N
        rows = _stem_rows(B, N)
        R, M1, M2, Kc1, Kc2 = rows.R, rows.M1, rows.M2, rows.Kc1, rows.Kc2
        padded, z1, c1, z2 = stem["padded"], stem["z1"], stem["c1"], stem["z2"]
        with on_stream() as s:
            dev = dx.device
            dz2 = torch.empty(M, d, dtype=torch.float32, device=dev)
            _lib.check(L.wipa_gelu_bwd(ptr(z2), ptr(dx), ptr(dz2), dz2.numel(), sptr(s)), "wipa_gelu_bwd")
            self._colsum(dz2, M, d, G("encoder.conv2.bias"))
            # the rows of conv2's GEMM: N + 1 per clip, the last one dead (zero), zero rows up to the padded contraction length
            dz2p = torch.zeros(Kc2, d, dtype=torch.float32, device=dev)
            dz2p[:M2].view(B, N + 1, d)[:, :N].copy_(dz2.view(B, N, d))
            self._wgrad_rows(dz2p, c1, 2 * d, Kc2, d, 3 * d, G("encoder.conv2.weight").view(d, 3 * d))
            taps = torch.empty(M2, 3 * d, dtype=torch.float32, device=dev)
            self._mm(dz2p, P("encoder.conv2.weight").view(d, 3 * d), taps, M2, 3 * d, d, d, 3 * d, w_trans=True)
            # the rows of conv1's GEMM: R per clip (2N frames, two dead rows written as zero by the kernel), zero rows up to Kc1
            dz1 = torch.empty(Kc1, d, dtype=torch.float32, device=dev)
            if Kc1 > M1:
                dz1[M1:].zero_()
            _lib.check(L.wipa_conv2_dx(ptr(taps), (N + 1) * 3 * d, ptr(z1[1:]), R * d, ptr(dz1), R * d, B, N, d, 2, sptr(s)),
                       "wipa_conv2_dx")
            self._colsum(dz1, M1, d, G("encoder.conv1.bias"))
            self._wgrad_rows(dz1, padded, n_mels, Kc1, d, 3 * n_mels, G("encoder.conv1.weight").view(d, 3 * n_mels))
        return dz1

    def loss_and_grads_from_mel(self, mel: torch.Tensor, tokens: torch.Tensor, eot: int, group=None, clip_keys=None, n_frames=None):
        """The full path of a trainer that trains encoder layers: mel [B, 3000, n_mels] (or [B, 2N, n_mels] with
        ``model.audio_ctx`` = N), tokens [B, T+1] int.  Encoder forward that keeps its activations, decoder forward and backward
        (which also yields the gradient of the encoder output), encoder backward.  Fills every segment of self.flat_g like
        loss_and_grads; returns (loss, sum_ce, n_valid).  With train_encoder_layers=0 it is embed_audio + loss_and_grads.
        ``clip_keys`` / ``n_frames``: the streams and the time axes of a trainer with ``spec_augment`` (ignored without one)."""
        if not self.trains_encoder:
            if self._spec_augment is not None:
                return self._loss_and_grads(self._embed_audio_augmented(mel, clip_keys, n_frames), tokens, eot, group, None)
            return self.loss_and_grads(self.model.embed_audio(mel), tokens, eot, group)
        feats, ectx = self._encoder_forward(mel, clip_keys, n_frames)
        self.last_features = feats  # the encoder output of this step (before the update)
        return self._loss_and_grads(feats, tokens, eot, group, ectx)

    def loss_and_grads(self, audio_features: torch.Tensor, tokens: torch.Tensor, eot: int, group=None):
        """features [B, 1500, d] f32 (encoder output, no gradient), tokens [B, T+1] int.
        Fills self.flat_g (un-clipped, already divided by the global valid count and, under DP,
        all-reduced).  Returns (loss, sum_ce, n_valid) as device scalars.  The fused path of the fine-tune step: masked CE and
        its gradient run in place on the logits (wipa_masked_ce / _bwd), nothing of size [B*T, V] is kept twice.
        Features carry no gradient, so only the decoder segments could be filled: a trainer that trains encoder layers
        refuses the call (loss_and_grads_from_mel is its path)."""
        self._decoder_only("loss_and_grads(audio_features, ...)")
        if self._spec_augment is not None:
            raise _lib.WipaError("DecoderTrainer.loss_and_grads(audio_features, ...) on a trainer with spec_augment: the masks are "
                                 "drawn on the mel -- step from it (train_step / loss_and_grads_from_mel)")
        return self._loss_and_grads(audio_features, tokens, eot, group, None)

    def _embed_audio_augmented(self, mel: torch.Tensor, clip_keys, n_frames) -> torch.Tensor:
        """model.embed_audio with the mask stored into its padded copy of the mel, between the pad and the encoder"""
        if mel is None:
            raise _lib.WipaError("DecoderTrainer: a trainer with spec_augment steps from the mel of every clip")
        B = 1 if mel.dim() == 2 else mel.shape[0]
        return self.model.embed_audio(mel, _mask_padded=lambda padded, F: self._augment_padded(padded, B, F, clip_keys, n_frames))

    def _loss_and_grads(self, audio_features: torch.Tensor, tokens: torch.Tensor, eot: int, group, ectx: Optional[Dict]):
        m, dm, L = self.model, self.model.dims, self.L
        if getattr(m, "_bank", None) is not None:
            raise _lib.WipaError("DecoderTrainer: a step while the model has an adapter bank set: set_adapter_bank(None) first (a bank "
                                 "serves inference; its adapters are trained one at a time, without it)")
        if self.lora is not None and getattr(m, "_adapter", None) is not None:
            raise _lib.WipaError("DecoderTrainer: a step while the model has an adapter applied: its weights are base + adapter, and the "
                                 "step would add the adapter a second time -- set_adapter(None) (or leave adapter_applied()) first")
        B, T1 = tokens.shape
        T = T1 - 1
        V = dm.n_vocab
        M, Vp = B * T, _ceil(V, 32)
        with on_stream() as s:
            dev = m.device
            tok = tokens.to(device=dev, dtype=torch.int32).contiguous()
            tok_in = tok[:, :-1].contiguous()
            logits, ctx = self._forward(audio_features, tok_in)
            row_buf = torch.empty(2 * M, dtype=torch.float32, device=dev)
            stats = torch.empty(2, dtype=torch.float32, device=dev)
            _lib.check(L.wipa_masked_ce(ptr(logits), Vp, ptr(tok), T1, B, T, V, eot, ptr(row_buf), ptr(stats), sptr(s)),
                       "wipa_masked_ce")
            sum_ce, n_valid = parallel.allreduce_loss_stats(stats[0], stats[1], group)
            count = n_valid.reshape(1).contiguous()
            loss = sum_ce / torch.clamp(n_valid, min=1.0)
            _lib.check(L.wipa_masked_ce_bwd(ptr(logits), Vp, ptr(tok), T1, B, T, V, ptr(row_buf[M:]), ptr(count), sptr(s)),
                       "wipa_masked_ce_bwd")
            reducer = self._new_reducer(group)
            d_feats = None if ectx is None else torch.empty_like(ctx["feats"])
            self._backward(ctx, logits, reducer, d_feats)
            del ctx, logits
            if ectx is not None:
                self._encoder_backward(ectx, d_feats, reducer)
            self._join_reductions(reducer, s)
        return loss, sum_ce, n_valid

    # ---- torch.autograd surface: Whisper.logits differentiable w.r.t. the decoder tensors (train_whisper_ipa.py:232,284) ----
    def leaves(self) -> Dict[str, torch.Tensor]:
        """name -> leaf tensor (requires_grad) that VIEWS the flat parameter buffer: what ``Whisper.logits`` differentiates
        against under torch.enable_grad().  ``.grad`` is filled by ``loss.backward()``; apply_update() reads self.flat_g, so a
        custom training loop copies / accumulates the leaves' gradients there (value_and_grad in scripts/train_whisper_ipa.py)."""
        self._decoder_only("leaves")
        self._no_lora("leaves")
        if self._leaves is None:
            self._leaves = {n: self.p(n).detach().requires_grad_(True) for n in self.names}
        return self._leaves

    differentiable_scope = False  # True inside value_and_grad(model, loss_fn): Whisper.logits then returns differentiable logits

    def differentiable_logits(self, tokens: torch.Tensor, audio_features: torch.Tensor) -> torch.Tensor:
        """logits [B, T, V] f32 with a grad_fn: the HIP forward of loss_and_grads, its hand-written backward behind
        torch.autograd.Function, so ANY torch-written loss on the logits gets exact decoder gradients.  The backward WRITES
        self.flat_g (zeroed first: gradients accumulated there by loss_and_grads are lost) and returns clones of every decoder
        gradient as the leaves' .grad (one more copy of the decoder's size); it reduces over no process group."""
        self._decoder_only("differentiable_logits")
        self._no_lora("differentiable_logits")
        if parallel.world()[1] != 1:
            raise _lib.WipaError("differentiable_logits is single-process (its backward runs without the data-parallel group); "
                                 "use DecoderTrainer.train_step / loss_and_grads(group=...) under torch.distributed")
        leaves = self.leaves()
        return _DecoderLogits.apply(self, tokens, audio_features, *[leaves[n] for n in self.names])


    @property
    def last_allreduce_exposed_ms(self) -> float:
        """Exposed (not overlapped with the backward) gradient all-reduce time of the last step, from HIP events on the
        compute stream around the final waits; 0 for a single process.  Synchronises."""
        ev = self._ar_events
        if not ev:
            return 0.0
        ev[1].synchronize()
        return float(ev[0].elapsed_time(ev[1]))

    def apply_update(self) -> None:
        """per-tensor clip (of the tensors ``clip_scope`` reaches) + AdamW on the flat buffers (flat_g becomes the gradient
        after the clip; ``self.norms`` the un-clipped L2 norm of every tensor)."""
        with on_stream() as s:
            _lib.check(self.L.wipa_clip_adamw(ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_v), ptr(self.ch_off),
                                              ptr(self.ch_len), ptr(self.ch_seg), ptr(self.seg_first), self.n_chunks, self.n_seg,
                                              ptr(self.partial), ptr(self.coef), ptr(self.norms), ptr(self.seg_clip), self.max_grad_norm, self.lr,
                                              self.b1, self.b2, self.eps, self.wd, sptr(s)), "wipa_clip_adamw")
        if self.trains_encoder:
            # encoder tensors moved: the packed encoder tables die with _invalidate() below, and whatever is a function of the
            # encoder weights (a FrozenFeatureCache, cached features) watches this count
            self.model._enc_generation += 1
        if self.lora is None:  # a LoRA step moves no tensor of the model
            self.model._invalidate()  # fused inference tables are rebuilt lazily from the updated weights
        self.step_count += 1

    def train_step(self, mel: Optional[torch.Tensor], tokens: torch.Tensor, eot: int, group=None, clip_keys=None, n_frames=None):
        """train_whisper_ipa.py:266-311: encoder forward (frozen), loss + grads, clip, AdamW.
        Returns (loss as a device scalar, dict of clipped gradients).
        ``clip_keys`` (one hashable int per clip, e.g. the dataset index) with an enabled feature cache: ``mel`` holds only the
        clips ``feature_cache.missing(clip_keys)`` marks (or is None when every clip is cached); the others come from HBM.
        With ``spec_augment``: ``clip_keys`` name the clips' streams and ``n_frames`` (one per clip: its own length in log-mel
        frames; None: the whole time axis) the span of the time masks."""
        if self.trains_encoder or self._spec_augment is not None:
            # encoder forward that saves activations, decoder forward / backward, encoder backward (no feature cache: refused)
            loss, _, _ = self.loss_and_grads_from_mel(mel, tokens, eot, group, clip_keys, n_frames)
        else:
            cached = clip_keys is not None and self.feature_cache is not None
            feats = self.feature_cache.assemble(clip_keys, mel) if cached else self.model.embed_audio(mel)
            loss, _, _ = self.loss_and_grads(feats, tokens, eot, group)
        self.apply_update()
        return loss, self.grads()


FineTuneTrainer = DecoderTrainer  # the name for what it has become; the class keeps its own


class _DecoderLogits(torch.autograd.Function):
    """TextDecoder.__call__ of the fine-tune step as one autograd node: forward = DecoderTrainer._forward (libwipa kernels),
    backward = DecoderTrainer._backward.  Gradients flow to the decoder tensors only (the encoder is frozen,
    train_whisper_ipa.py:187; features and tokens get None)."""

    @staticmethod
    def forward(ctx, trainer, tokens, audio_features, *leaves):
        B, T = tokens.shape
        with on_stream():
            tok_in = tokens.to(device=trainer.model.device, dtype=torch.int32).contiguous()
        logits, saved = trainer._forward(audio_features, tok_in)
        ctx.trainer, ctx.saved_acts, ctx.shape = trainer, saved, (B, T, logits.shape[0], logits.shape[1])
        V = trainer.model.dims.n_vocab
        return logits[: B * T].view(B, T, logits.shape[1])[:, :, :V]

    @staticmethod
    def backward(ctx, dlogits):
        tr = ctx.trainer
        B, T, Mp, Vp = ctx.shape
        V = tr.model.dims.n_vocab
        with on_stream() as s:
            dl = torch.zeros(Mp, Vp, dtype=torch.float32, device=tr.model.device)
            dl[: B * T].view(B, T, Vp)[:, :, :V].copy_(dlogits)
            reducer = tr._new_reducer(None)  # single-process (differentiable_logits refuses anything else): nothing to reduce
            tr._backward(ctx.saved_acts, dl, reducer)
            tr._join_reductions(reducer, s)
            ctx.saved_acts = None
            grads = tuple(tr.g(n).clone() for n in tr.names)
        return (None, None, None) + grads


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= s
    return n
