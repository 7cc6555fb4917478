#!/usr/bin/env python3
"""Bytes of the decoder-only fine-tune step, for comparing two commits: two train_step calls of DecoderTrainer(model) -- no
train_encoder_layers argument, so the script runs on commits that do not have it -- on the MICRO model of the tests (synthetic weights,
3 clips, exact and split products, both clip scopes), then the SHA-256 of every loss, of the flat parameter, gradient and moment buffers
and the list of tensor names and offsets.  Run it in both checkouts on the same GPU and diff the outputs
(profiles/encoder_train_k0_bytes.txt).
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


if __name__ == "__main__":
    main()
