#!/usr/bin/env python3
"""Device-side audio ingest against the host path, per source rate: B clips x 30 s, s16 mono (default 64 clips at 16 / 44.1 / 48 kHz).
For every rate: the host-to-device copy of the packed PCM, the resample-and-pad kernel (csrc/resample.hip) and the two together
through audio.load_audio_batch (HIP events, mean of N calls after warm-up); the host's load_audio on the same box on a few of the
same clips (wall clock per clip, extrapolated to the batch); and, once, log-mel on the kernel's output for scale.
usage: python tools/ingest_bench.py [--batch 64] [--rates 16000 44100 48000] [--host-clips 2] [--iters 10]"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
from whisper_ipa_amd import _lib, audio  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402

PASS_MS = 72.0  # one 64-clip pass of log-mel -> encoder -> decode with four in flight


def timed(fn, s, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        fn()
    s.synchronize()
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 44100, 48000])
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--host-clips", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    rows = []
    print(f"# device ingest, {args.batch} clips x {args.seconds:g} s, s16 mono, {torch.cuda.get_device_name(dev)}")
    print(f"# {'rate':>6} {'MB':>7} {'pack ms':>8} {'H2D ms':>8} {'GB/s':>6} {'kernel ms':>10} {'copy+kernel':>12} {'host s/clip':>12} {'host s/batch':>13} {'speed-up':>9}")
    for rate in args.rates:
        n = int(rate * args.seconds)
        clips = [audio.PcmClip((0.3 * 32767 * rng.standard_normal(n)).clip(-32768, 32767).astype("<i2").tobytes(), n, 1, 2, rate)
                 for _ in range(args.batch)]
        t0 = time.perf_counter()
        batch = audio.PcmBatch(clips)
        pack_ms = (time.perf_counter() - t0) * 1e3
        with on_stream() as s:
            tables = audio._tables_for(dev, batch)
            pcm = torch.empty(batch.nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(batch.B, audio.N_SAMPLES, dtype=torch.float32, device=dev)
            copy_ms = timed(lambda: pcm.copy_(batch.buffer, non_blocking=True), s, args.iters)
            kernel_ms = timed(lambda: _lib.check(L.wipa_resample_pad(ptr(pcm), batch.nbytes, ptr(pcm), batch.descs, batch.B, ptr(tables),
                                                                     tables.numel(), ptr(out), sptr(s)), "wipa_resample_pad"), s, args.iters)
            both_ms = timed(lambda: audio.load_audio_batch(batch, out=out), s, args.iters)
        # the host path on the same box, on files holding the same samples
        host_s, worst = [], 0.0
        with tempfile.TemporaryDirectory() as d:
            for i in range(min(args.host_clips, args.batch)):
                p = os.path.join(d, f"c{i}.wav")
                with wave.open(p, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(rate)
                    w.writeframes(clips[i].data)
                t0 = time.perf_counter()
                ref = audio.pad_or_trim(audio.load_audio(p))
                host_s.append(time.perf_counter() - t0)
                worst = max(worst, float(np.abs(out[i].cpu().numpy() - ref).max()))
        per_clip = float(np.mean(host_s)) if host_s else float("nan")
        row = dict(rate=rate, batch=args.batch, pcm_mb=batch.nbytes / 1e6, pack_ms=pack_ms, h2d_ms=copy_ms, h2d_gb_s=batch.nbytes / copy_ms / 1e6,
                   kernel_ms=kernel_ms, copy_plus_kernel_ms=both_ms, host_s_per_clip=per_clip, host_s_per_batch=per_clip * args.batch,
                   speedup=per_clip * args.batch * 1e3 / both_ms, max_abs_diff_vs_host=worst)
        rows.append(row)
        print(f"  {rate:>6} {row['pcm_mb']:>7.1f} {pack_ms:>8.1f} {copy_ms:>8.2f} {row['h2d_gb_s']:>6.1f} {kernel_ms:>10.3f} {both_ms:>12.2f} "
              f"{per_clip:>12.3f} {row['host_s_per_batch']:>13.1f} {row['speedup']:>8.0f}x   (max |device - host| {worst:.1e})")
        del pcm, batch, clips
    with on_stream() as s:
        mel_ms = timed(lambda: audio.log_mel_padded(out, 80, torch.bfloat16), s, args.iters)
    print(f"# log-mel on the kernel's output ({args.batch} clips, 80 bins, bf16): {mel_ms:.3f} ms")
    print(f"# one pass of log-mel -> encoder -> decode with four in flight: {PASS_MS:.0f} ms; ingest (copy + kernel) must stay below it")
    print(json.dumps({"ingest_bench": rows, "logmel_ms": mel_ms, "pass_ms": PASS_MS}))


if __name__ == "__main__":
    main()
