#!/usr/bin/env python3
"""What training encoder layers costs on an MI355X: the whisper-small float32 fine-tune step of bench.py --mode train (32 clips x 64
target tokens, synthetic weights, no feature cache) with DecoderTrainer(train_encoder_layers=K) for K = 0, 2, 6, 12 and "all", exact
and split products.  Per (K, products): ms per step (host wall clock around synchronised steps, as bench.py), the peak of
torch.cuda.max_memory_allocated over a step, and both next to the K = 0 figure of the SAME run.
The split rows run the encoder's attention backward on the split-product kernels, as an f32_split trainer does.
Then the attention backward alone at encoder shapes -- B = 8, H = 12, Tq = Tk = 1500 and 300, non-causal, f32: the exact f32-MFMA
kernels against the split-product kernels (wipa_attention_bwd_ex, f32_split 0 / 1), alternating, HIP events, TF/s of the 5 matmuls
(10 * B * H * T^2 * 64 FLOP): the A/B behind the choice of what the trainer wires in.
--profile-step K runs one warm-up and two steps of one configuration and nothing else: the command to put behind
`rocprofv3 --kernel-trace --stats --output-format csv -d out --` for the per-kernel split of a step.
usage: python tools/encoder_train_bench.py [--steps 3] [--layers 0,2,6,12,all] [--f32 exact,split] [--profile-step all]"""
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
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402
from whisper_ipa_amd.training import QK_SCALE, DecoderTrainer  # noqa: E402
from whisper_ipa_amd.whisper import Whisper  # noqa: E402

TRAIN_B, TRAIN_T = 32, 64


def parse_k(text):
    return text if text == "all" else int(text)


def trainer_for(k, split):
    dims, W = bench.synthetic_weights_small(0, "small")
    m = Whisper(dims, dtype=torch.float32, f32_split=split)
    m.load_weights(W)
    del W
    return DecoderTrainer(m, lr=1e-5, f32_split=split, train_encoder_layers=k), dims


def step_times(k, split, steps):
    tr, dims = trainer_for(k, split)
    mel, tok, eot = bench.synthetic_train_batch(TRAIN_B, TRAIN_T, dims.n_mels)
    mel, tok = mel.cuda(), tok.cuda()
    tr.train_step(mel, tok, eot)  # warm-up: workspaces, slabs
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loss, _ = tr.train_step(mel, tok, eot)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated()
    out = {"train_encoder_layers": k, "f32": "split" if split else "exact", "step_ms": ms, "loss": float(loss),
           "held_GB": held / 1e9, "peak_GB": peak / 1e9, "trained_floats": tr.n_params}
    tr.model._trainer = None  # the model and its trainer point at each other: break the cycle so the buffers go now,
    del tr, mel, tok          # not at some later collection inside the next configuration's peak
    gc.collect()
    torch.cuda.empty_cache()
    return out


def attention_bwd(T, B=8, H=12, repeats=5):
    """ms of one wipa_attention_bwd_ex call (dQ kernel + dK/dV kernel) on [B*T, H*64] row-major q, k, v: exact and split, alternating"""
    L = _lib.lib()
    d = H * 64
    g = torch.Generator().manual_seed(T)
    with on_stream() as s:
        q, k, v, go = (torch.randn(B * T, d, generator=g).cuda() * sc for sc in (0.5, 0.5, 1.0, 1.0))
        out = torch.empty_like(q)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
        a = _lib.AttnDesc()
        a.q, a.k, a.v, a.out, a.lse = ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse)
        for n in ("q", "k", "v", "o"):
            setattr(a, f"{n}_bs", T * d), setattr(a, f"{n}_rs", d), setattr(a, f"{n}_hs", 64)
        a.B, a.H, a.Tq, a.Tk, a.causal, a.dtype = B, H, T, T, 0, 0
        _lib.check(L.wipa_attention(C.byref(a), sptr(s)), "wipa_attention")
        dq, dk, dv, dvec = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q), torch.empty_like(lse)

        def run(split):
            _lib.check(L.wipa_attention_bwd_ex(C.byref(a), ptr(out), ptr(go), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(dvec), QK_SCALE,
                                               split, sptr(s)), "wipa_attention_bwd_ex")

        grads = {}
        for split in (0, 1):
            run(split)
            grads[split] = [t.clone() for t in (dq, dk, dv)]
        apart = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(grads[1], grads[0]))
        ms = {0: [], 1: []}
        for _ in range(repeats):
            for split in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                run(split)
                e1.record(s)
                e1.synchronize()
                ms[split].append(e0.elapsed_time(e1))
    flop = 10.0 * B * H * T * T * 64
    return {"T": T, "B": B, "H": H, "exact_ms": ms[0], "split_ms": ms[1], "exact_tflops_at_min": flop / min(ms[0]) / 1e9,
            "split_tflops_at_min": flop / min(ms[1]) / 1e9, "split_vs_exact_max_rel": apart}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--layers", default="0,2,6,12,all")
    ap.add_argument("--f32", default="exact,split")
    ap.add_argument("--profile-step", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    if args.profile_step is not None:
        r = step_times(parse_k(args.profile_step), args.f32.split(",")[-1] == "split", 2)
        print(json.dumps({"encoder_train_profile_step": r}))
        return
    print(f"# encoder fine-tuning: whisper-small f32 synthetic weights, {TRAIN_B} clips x {TRAIN_T} target tokens, {args.steps} steps per "
          f"configuration after one warm-up, {torch.cuda.get_device_name(0)}")
    rows = []
    for mode in args.f32.split(","):
        base = None
        for k in (parse_k(x) for x in args.layers.split(",")):
            r = step_times(k, mode == "split", args.steps)
            rows.append(r)
            base = base or r
            mean, mean0 = sum(r["step_ms"]) / len(r["step_ms"]), sum(base["step_ms"]) / len(base["step_ms"])
            print(f"  {mode:<5} train_encoder_layers={k!s:<4} step {mean:9.2f} ms (min {min(r['step_ms']):9.2f}) = {mean / mean0:6.2f} x K=0 "
                  f"({mean0:.2f} ms)   peak {r['peak_GB']:6.2f} GB (K=0 {base['peak_GB']:.2f} GB; held between steps {r['held_GB']:.2f} GB)   "
                  f"trained {r['trained_floats'] / 1e6:.1f} M floats   loss {r['loss']:.6f}")
    attn = [attention_bwd(T) for T in (1500, 300)]
    for r in attn:
        print(f"  attention backward B={r['B']} H={r['H']} Tq=Tk={r['T']}: exact f32 MFMA {min(r['exact_ms']):8.3f} ms (mean "
              f"{sum(r['exact_ms']) / len(r['exact_ms']):.3f}, {r['exact_tflops_at_min']:.1f} TF/s of its five matmuls)   split bf16 MFMA "
              f"{min(r['split_ms']):8.3f} ms (mean {sum(r['split_ms']) / len(r['split_ms']):.3f}, {r['split_tflops_at_min']:.1f} TF/s)   "
              f"split / exact {min(r['split_ms']) / min(r['exact_ms']):.3f}   gradients {r['split_vs_exact_max_rel']:.1e} apart")
    print(json.dumps({"encoder_train_bench": {"steps": rows, "attention_bwd": attn}}))


if __name__ == "__main__":
    main()
