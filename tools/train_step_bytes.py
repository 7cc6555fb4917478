#!/usr/bin/env python3
"""Bytes of the decoder-only fine-tune step, for comparing two commits: two train_step calls of DecoderTrainer(model) -- no
train_encoder_layers argument, so the script runs on commits that do not have it -- on the MICRO model of the tests (synthetic weights,
3 clips, exact and split products, both clip scopes), then the SHA-256 of every loss, of the flat parameter, gradient and moment buffers
and the list of tensor names and offsets.  Run it in both checkouts on the same GPU and diff the outputs
(profiles/encoder_train_k0_bytes.txt).
After those 16 lines, more_configurations() does the same for the other paths of the step -- encoder layers, audio_ctx, SpecAugment, the
feature cache, differentiable_logits, the tuned shape with its GEMM dispatch census -- through the trainer's public surface only
(profiles/train_step_refactor_bytes.txt); a commit older than those options stops there, after the 16 lines.
usage: python tools/train_step_bytes.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import whisper_ref as R  # noqa: E402
from whisper_ipa_amd.training import DecoderTrainer  # noqa: E402
from whisper_ipa_amd.whisper import ModelDimensions, Whisper  # noqa: E402

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
EOT = 50257


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def main():
    W = R.synthetic_weights(MICRO, seed=7)
    g = torch.Generator().manual_seed(3)
    mel = (torch.rand(3, 3000, 80, generator=g) * 2 - 1).cuda()
    rng = np.random.default_rng(5)
    sot = [50258, 50259, 50359, 50363]
    seqs = [sot + rng.integers(0, 50257, size=n).tolist() + [EOT] for n in (9, 5, 7)]
    T = max(len(s) for s in seqs)
    tokens = torch.tensor([s + [EOT] * (T - len(s)) for s in seqs], dtype=torch.int64).cuda()
    for split in (False, True):
        for scope in ("reference", "all"):
            m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=torch.float32, f32_split=split)
            m.load_weights(W)
            tr = DecoderTrainer(m, lr=1e-3, f32_split=split, clip_scope=scope)
            tag = f"{'split' if split else 'exact'} clip_scope={scope}"
            print(f"{tag}: {len(tr.names)} tensors, {tr.n_params} floats, layout "
                  f"{hashlib.sha256(repr(sorted(tr.offsets.items())).encode()).hexdigest()[:32]}")
            for step in (1, 2):
                loss, _ = tr.train_step(mel, tokens, EOT)
                torch.cuda.synchronize()
                print(f"{tag} step {step}: loss {float(loss):.9g} {sha(loss)}  p {sha(tr.flat_p)}  g {sha(tr.flat_g)}  m {sha(tr.flat_m)}  "
                      f"v {sha(tr.flat_v)}  norms {sha(tr.norms)}")
            print(f"{tag}: features after the steps {sha(m.embed_audio(mel))}")
    more_configurations(W, mel, tokens)


def micro_trainer(W, split=True, audio_ctx=None, **kw):
    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=torch.float32, f32_split=split)
    m.load_weights(W)
    if audio_ctx is not None:
        m.audio_ctx = audio_ctx
    return DecoderTrainer(m, lr=1e-3, f32_split=split, **kw)


def layout_line(tag, tr):
    print(f"{tag}: {len(tr.names)} tensors, {tr.n_params} floats, layout {hashlib.sha256(repr(sorted(tr.offsets.items())).encode()).hexdigest()[:32]}")


def state_line(tag, tr, loss, extra=""):
    torch.cuda.synchronize()
    feats = f"  features {sha(tr.last_features)}" if tr.trains_encoder else ""
    print(f"{tag}: loss {float(loss):.9g} {sha(loss)}  p {sha(tr.flat_p)}  g {sha(tr.flat_g)}  m {sha(tr.flat_m)}  v {sha(tr.flat_v)}  "
          f"norms {sha(tr.norms)}{feats}{extra}")


def two_steps(tag, tr, mel, tokens, **kw):
    layout_line(tag, tr)
    for step in (1, 2):
        loss, _ = tr.train_step(mel, tokens, EOT, **kw)
        state_line(f"{tag} step {step}", tr, loss)


def more_configurations(W, mel, tokens):
    """The paths the 16 lines above do not reach, same 3 clips and ragged token rows (B*T is odd: the transposing path of the linear
    backward): encoder training, the short audio context, SpecAugment, the feature cache, the autograd surface; then the tuned shape
    of tests/test_gpu_training.py (width 768, 32 clips x 64 targets: split-K, K-major operands, one [2d, d] cross projection) with
    the GEMM dispatch census of every step."""
    import bench
    from whisper_ipa_amd import audio, ops
    from whisper_ipa_amd.runtime import on_stream

    for layers in (1, "all"):
        for split in (False, True):
            two_steps(f"micro train_encoder_layers={layers} {'split' if split else 'exact'}", micro_trainer(W, split, train_encoder_layers=layers),
                      mel, tokens)
    for layers in (0, "all"):
        two_steps(f"micro audio_ctx=33 train_encoder_layers={layers}", micro_trainer(W, audio_ctx=33, train_encoder_layers=layers),
                  mel[:, :66].contiguous(), tokens)
    for layers in (0, "all"):
        aug = audio.SpecAugment(0.2, 10, 2, 0.2, 10, 2, fill=-3.0, seed=5)
        two_steps(f"micro spec_augment train_encoder_layers={layers}", micro_trainer(W, train_encoder_layers=layers, spec_augment=aug),
                  mel, tokens, clip_keys=[4242, 17, 5], n_frames=[137, 3000, 900])
    tr = micro_trainer(W)
    tr.enable_feature_cache(8)
    layout_line("micro feature cache", tr)
    for step, visit in ((1, mel), (2, None)):  # first visit from the mel, second one from the cache alone
        loss, _ = tr.train_step(visit, tokens, EOT, clip_keys=[4242, 17, 5])
        state_line(f"micro feature cache step {step}", tr, loss, f"  hits {tr.feature_cache.hits} misses {tr.feature_cache.misses}")
    tr = micro_trainer(W)
    feats = tr.model.embed_audio(mel)
    with torch.enable_grad(), on_stream():
        loss = (tr.differentiable_logits(tokens[:, :-1], feats) ** 2).sum()
        loss.backward()
    loss = loss.detach()
    torch.cuda.synchronize()
    leaves = tr.leaves()
    picked = ("decoder.token_embedding.weight", "decoder.blocks.1.cross_attn.key.weight")
    print(f"micro differentiable_logits: loss {float(loss):.9g} {sha(loss)}  g {sha(tr.flat_g)}  " + "  ".join(f"{n} {sha(leaves[n].grad)}" for n in picked))

    tuned = R.ModelDimensions(80, 1500, 768, 12, 1, 51865, 448, 768, 12, 2)
    Wt = R.synthetic_weights(tuned, seed=21)
    tmel, ttok, eot = bench.synthetic_train_batch(32, 64, tuned.n_mels)
    tmel, ttok = tmel.cuda(), ttok.cuda()
    for layers in (0, "all"):
        for split in (False, True):
            m = Whisper(ModelDimensions(**tuned.__dict__), dtype=torch.float32, f32_split=split)
            m.load_weights(Wt)
            tr = DecoderTrainer(m, lr=1e-3, f32_split=split, train_encoder_layers=layers)
            tag = f"tuned train_encoder_layers={layers} {'split' if split else 'exact'}"
            layout_line(tag, tr)
            for step in (1, 2):
                ops.gemm_dispatch_counts(reset=True)
                loss, _ = tr.train_step(tmel, ttok, eot)
                state_line(f"{tag} step {step}", tr, loss, f"  gemm dispatch {sorted(ops.gemm_dispatch_counts(reset=True).items())}")
            m._trainer = None  # the model and its trainer point at each other: break the cycle so the buffers go now
            del tr, m


if __name__ == "__main__":
    main()
