#!/usr/bin/env python3
"""What SpecAugment costs on an MI355X.
1. The kernel alone (wipa_spec_augment, streams and frame counts already on the device): B = 32 and 64 clips x 3000 frames x 80 and 128
   bins in the padded layout the trainer masks, with the default settings over the whole window (n_frames = None) and over short clips
   (n_frames drawn from 100..600), next to ONE plain device-to-device copy of the same mel (torch's copy_), alternating.  Device
   events around --launches back-to-back launches; the bytes the kernel writes are counted from the host plan (4 bytes per masked
   element, overlaps counted once).
2. The whisper-small float32 fine-tune step of bench.py --mode train (32 clips x 64 target tokens, synthetic weights, split products, no
   feature cache) with and without an augmenter, at train_encoder_layers 0 and "all": ONE trainer per setting, the augmenter switched
   on and off from step to step, host wall clock around synchronised steps.
usage: python tools/spec_augment_bench.py [--launches 200] [--steps 4] [--skip-steps]"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib  # noqa: E402
from whisper_ipa_amd.audio import SpecAugment, padded_mel_rows  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, sptr  # noqa: E402
from whisper_ipa_amd.training import DecoderTrainer  # noqa: E402
from whisper_ipa_amd.whisper import Whisper  # noqa: E402

TRAIN_B, TRAIN_T, FRAMES = 32, 64, 3000


def masked_elements(plan: np.ndarray, aug: SpecAugment, n_frames, n_mels: int) -> int:
    """elements the kernel stores, from the host plan: the union of the time rows and the bin columns of every clip"""
    total = 0
    for b in range(plan.shape[0]):
        L = FRAMES if n_frames is None else min(int(n_frames[b]), FRAMES)
        rows, cols = np.zeros(FRAMES, dtype=bool), np.zeros(n_mels, dtype=bool)
        for s in plan[b, 0, 1:1 + plan[b, 0, 0]]:
            rows[s:s + min(aug.cfg.length[0], L)] = True
        for s in plan[b, 1, 1:1 + plan[b, 1, 0]]:
            cols[s:s + min(aug.cfg.length[1], n_mels)] = True
        r, c = int(rows.sum()), int(cols.sum())
        total += r * n_mels + (FRAMES - r) * c
    return total


def kernel_times(aug: SpecAugment, B: int, n_mels: int, short: bool, launches: int):
    L = _lib.lib()
    rng = np.random.default_rng(B * 1000 + n_mels)
    streams = np.stack([np.arange(B), np.zeros(B, dtype=np.int64)], axis=1)
    n_frames = rng.integers(100, 601, size=B) if short else None
    written = 4 * masked_elements(aug.plan(streams, n_frames, FRAMES, n_mels), aug, n_frames, n_mels)
    R = FRAMES + 2
    with on_stream() as s:
        dev = torch.device("cuda")
        padded = torch.rand(padded_mel_rows(B), n_mels, device=dev)
        other = torch.empty_like(padded)
        st = torch.from_numpy(streams.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
        nf = None if n_frames is None else torch.from_numpy(n_frames.astype(np.int32)).to(dev)

        def mask():
            _lib.check(L.wipa_spec_augment(padded.data_ptr() + 4 * n_mels, R * n_mels, n_mels, B, FRAMES, n_mels, C.byref(aug.cfg),
                                           st.data_ptr(), None if nf is None else nf.data_ptr(), aug.seed, sptr(s)), "wipa_spec_augment")

        def copy():
            other.copy_(padded)

        ms = {"mask": [], "copy": []}
        for fn in (mask, copy):  # warm-up
            fn()
        for _ in range(5):
            for name, fn in (("mask", mask), ("copy", copy)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(launches):
                    fn()
                e1.record(s)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / launches * 1e3)  # us per launch
    return {"B": B, "n_mels": n_mels, "short_clips": short, "mask_us": ms["mask"], "copy_us": ms["copy"], "bytes_written": written,
            "mel_bytes": B * FRAMES * n_mels * 4}


def step_times(k, aug: SpecAugment, steps: int):
    dims, W = bench.synthetic_weights_small(0, "small")
    m = Whisper(dims, dtype=torch.float32, f32_split=True)
    m.load_weights(W)
    del W
    tr = DecoderTrainer(m, lr=1e-5, f32_split=True, train_encoder_layers=k)
    mel, tok, eot = bench.synthetic_train_batch(TRAIN_B, TRAIN_T, dims.n_mels)
    mel, tok = mel.cuda(), tok.cuda()
    n_frames = np.random.default_rng(1).integers(100, 601, size=TRAIN_B).tolist()
    ms = {"plain": [], "augmented": []}
    for a in (None, aug):  # warm-up of both paths
        tr.spec_augment = a
        tr.train_step(mel, tok, eot, n_frames=n_frames)
    torch.cuda.synchronize()
    for _ in range(steps):
        for name, a in (("plain", None), ("augmented", aug)):
            tr.spec_augment = a
            t0 = time.perf_counter()
            loss, _ = tr.train_step(mel, tok, eot, n_frames=n_frames)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {"train_encoder_layers": k, "plain_ms": ms["plain"], "augmented_ms": ms["augmented"], "loss": float(loss)}
    tr.model._trainer = None
    del tr, mel, tok
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    aug = SpecAugment()
    print(f"# SpecAugment, default settings {aug.settings}, {torch.cuda.get_device_name(0)}")
    print(f"# kernel: padded layout, {args.launches} back-to-back launches per window, 5 windows, alternating with one plain copy of the mel")
    kernels = []
    for B in (32, 64):
        for n_mels in (80, 128):
            for short in (False, True):
                r = kernel_times(aug, B, n_mels, short, args.launches)
                kernels.append(r)
                mk, cp = min(r["mask_us"]), min(r["copy_us"])
                print(f"  B={B:<3} n_mels={n_mels:<4} {'n_frames 100..600' if short else 'n_frames None    '}: mask {mk:7.2f} us (mean "
                      f"{sum(r['mask_us']) / 5:7.2f}), writes {r['bytes_written'] / 1e6:6.3f} MB of a {r['mel_bytes'] / 1e6:6.1f} MB mel"
                      f" = {r['bytes_written'] / mk / 1e3:7.1f} GB/s   copy of the mel {cp:7.2f} us (mean {sum(r['copy_us']) / 5:7.2f})   "
                      f"mask / copy {mk / cp:.3f}")
    steps = []
    if not args.skip_steps:
        print(f"# step: whisper-small f32 split, {TRAIN_B} clips x {TRAIN_T} target tokens, no feature cache, n_frames 100..600, {args.steps} "
              f"steps each, alternating on one trainer")
        for k in (0, "all"):
            r = step_times(k, aug, args.steps)
            steps.append(r)
            p, a = sum(r["plain_ms"]) / len(r["plain_ms"]), sum(r["augmented_ms"]) / len(r["augmented_ms"])
            print(f"  train_encoder_layers={k!s:<4} plain {p:9.2f} ms (min {min(r['plain_ms']):9.2f})   augmented {a:9.2f} ms (min "
                  f"{min(r['augmented_ms']):9.2f})   augmented - plain {a - p:+.2f} ms ({(a / p - 1) * 100:+.2f} %)")
    print(json.dumps({"spec_augment_bench": {"kernel": kernels, "steps": steps}}))


if __name__ == "__main__":
    main()
