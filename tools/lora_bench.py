#!/usr/bin/env python3
"""What LoRA fine-tuning costs on an MI355X, against the full decoder step, and the adapter kernels against a composition of GEMMs.

(a) The fine-tune step: whisper-small dimensions, synthetic weights, f32, 32 clips x 64 target tokens, in ONE process: the full step
    (DecoderTrainer(model)) and the LoRA step at rank 16 on query,value and on all six targets.  Per configuration: host wall clock of
    train_step from the mel (synchronised steps, as bench.py's finetune_step -- the full step's figure is the one to hold against it),
    the decoder step on cached features by class from HIP events around DecoderTrainer._forward / ._backward / .apply_update (the
    rest of loss_and_grads -- masked CE and its gradient -- is listed as "loss"), the bytes of the four flat buffers and the bytes
    handed to the SegmentReducer per step.
(b) One adapted linear at rank 16, K = N = 768, M = 2048 (the tuned step's token rows) and M = 48 000 (32 clips of encoder rows):
    wipa_lora_fwd + wipa_lora_bwd against the same arithmetic composed from wipa_gemm / wipa_transpose / wipa_sum_slabs as the
    trainer composes its linears (DecoderTrainer._lin / ._lin_bwd on A and Bm padded to 32 columns: wipa_gemm takes K in whole
    32-float steps), exact f32 products on both sides, alternating, HIP events.
usage: python tools/lora_bench.py [--steps 5] [--repeats 10] [--f32 split]"""
import argparse
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
from whisper_ipa_amd.lora import LoRAConfig  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402
from whisper_ipa_amd.training import DecoderTrainer  # noqa: E402
from whisper_ipa_amd.whisper import Whisper  # noqa: E402

TRAIN_B, TRAIN_T = 32, 64
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")


def instrument(tr):
    """HIP events around the trainer's forward, backward and optimiser, on the library stream"""
    ev = {}
    for name in ("_forward", "_backward", "apply_update", "_loss_and_grads"):
        def wrapped(*a, _orig=getattr(tr, name), _name=name, **kw):
            with on_stream() as s:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                out = _orig(*a, **kw)
                e1.record(s)
            ev.setdefault(_name, []).append((e0, e1))
            return out
        setattr(tr, name, wrapped)
    return ev


def step_config(label, lora, split, steps):
    dims, W = bench.synthetic_weights_small(0, "small")
    m = Whisper(dims, dtype=torch.float32, f32_split=split)
    m.load_weights(W)
    del W
    tr = DecoderTrainer(m, lr=1e-5, f32_split=split, lora=lora)
    mel, tok, eot = bench.synthetic_train_batch(TRAIN_B, TRAIN_T, dims.n_mels)
    mel, tok = mel.cuda(), tok.cuda()
    tr.train_step(mel, tok, eot)  # warm-up: workspaces, slabs
    torch.cuda.synchronize()
    wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loss, _ = tr.train_step(mel, tok, eot)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    feats = m.embed_audio(mel)
    ev = instrument(tr)
    for _ in range(steps):
        tr.loss_and_grads(feats, tok, eot)
        tr.apply_update()
    torch.cuda.synchronize()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    mean = lambda v: sum(v) / len(v)
    fwd, bwd, opt, lg = mean(ms["_forward"]), mean(ms["_backward"]), mean(ms["apply_update"]), mean(ms["_loss_and_grads"])
    out = {"config": label, "f32": "split" if split else "exact", "train_step_from_mel_ms": wall, "forward_ms": fwd, "backward_ms": bwd,
           "loss_ms": lg - fwd - bwd, "optimiser_ms": opt, "decoder_step_ms": lg + opt, "trained_floats": tr.n_params,
           "flat_buffer_bytes": 4 * 4 * tr.n_params, "reducer_bytes_per_step": 4 * sum(hi - lo for _, lo, hi in tr.segments),
           "loss": float(loss)}
    m._trainer = None
    del tr, m, mel, tok, feats
    gc.collect()
    torch.cuda.empty_cache()
    return out


def linear_ab(M, K, N, r, repeats):
    """ms of wipa_lora_fwd + wipa_lora_bwd against the GEMM composition on the same operands (gain 1)"""
    L = _lib.lib()
    g = torch.Generator().manual_seed(M)
    rp = 32
    with on_stream() as s:
        x, dy, y0 = (torch.randn(M, c, generator=g).cuda() for c in (K, N, N))
        A = ((torch.rand(r, K, generator=g) * 2 - 1) * K ** -0.5).cuda()
        Bm = (0.1 * torch.randn(N, r, generator=g)).cuda()
        A_pad, B_pad = torch.zeros(rp, K, device="cuda"), torch.zeros(N, rp, device="cuda")
        A_pad[:r].copy_(A)
        B_pad[:, :r].copy_(Bm)
        y, u = y0.clone(), torch.empty(M, r, device="cuda")
        dA, dB, dx = torch.empty(r, K, device="cuda"), torch.empty(N, r, device="cuda"), torch.empty(M, K, device="cuda")
        ws_bytes = L.wipa_lora_workspace_bytes(M, K, N, r)
        ws = torch.empty(ws_bytes // 4, device="cuda")
        helper = object.__new__(DecoderTrainer)  # the trainer's GEMM helpers alone: no model, no flat buffers
        helper.L, helper.f32_split, helper._slabs = L, False, None
        dA_c, dB_c, dx_c, y_c = torch.empty(rp, K, device="cuda"), torch.empty(N, rp, device="cuda"), torch.empty(M, K, device="cuda"), y0.clone()

        def kernels():
            _lib.check(L.wipa_lora_fwd(ptr(x), K, ptr(A), ptr(Bm), ptr(y), N, ptr(u), M, K, N, r, 1.0, sptr(s)), "wipa_lora_fwd")
            _lib.check(L.wipa_lora_bwd(ptr(dy), N, ptr(x), K, ptr(u), ptr(A), ptr(Bm), ptr(dA), ptr(dB), ptr(dx), K, 0, M, K, N, r, 1.0,
                                       ptr(ws), ws_bytes, sptr(s)), "wipa_lora_bwd")

        def composed():
            u_pad = helper._lin(x, M, K, A_pad, rp)
            helper._lin(u_pad, M, rp, B_pad, N, residual=y_c, out=y_c)
            du = helper._lin_bwd(dy, M, N, u_pad, None, rp, B_pad, dB_c)
            helper._lin_bwd(du, M, rp, x, None, K, A_pad, dA_c, dx=dx_c)

        kernels()
        composed()
        apart = {"dA": float((dA - dA_c[:r]).abs().max() / dA.abs().max()), "dB": float((dB - dB_c[:, :r]).abs().max() / dB.abs().max()),
                 "dx": float((dx - dx_c).abs().max() / dx.abs().max())}
        ms = {"kernels": [], "composed": []}
        for _ in range(repeats):
            for name, fn in (("kernels", kernels), ("composed", composed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    return {"M": M, "K": K, "N": N, "r": r, "kernels_ms": ms["kernels"], "composed_ms": ms["composed"], "max_rel_apart": apart}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--f32", default="split", choices=["split", "exact"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    split = args.f32 == "split"
    print(f"# LoRA fine-tuning: whisper-small f32 synthetic weights ({args.f32} products), {TRAIN_B} clips x {TRAIN_T} target tokens, {args.steps} "
          f"steps per configuration after one warm-up, {torch.cuda.get_device_name(0)}")
    rows = []
    for label, lora in (("full decoder", None), ("lora r16 query,value", LoRAConfig(rank=16, targets=("query", "value"))),
                        ("lora r16 all six", LoRAConfig(rank=16, targets=ALL))):
        r = step_config(label, lora, split, args.steps)
        rows.append(r)
        w = r["train_step_from_mel_ms"]
        print(f"  {label:<22} train_step from the mel {sum(w) / len(w):8.2f} ms (min {min(w):8.2f})   decoder step on cached features "
              f"{r['decoder_step_ms']:8.2f} ms = forward {r['forward_ms']:7.2f} + loss {r['loss_ms']:6.2f} + backward {r['backward_ms']:7.2f} + "
              f"optimiser {r['optimiser_ms']:6.2f}   trained {r['trained_floats'] / 1e6:8.3f} M floats   flat buffers "
              f"{r['flat_buffer_bytes'] / 1e6:9.2f} MB   to the reducer {r['reducer_bytes_per_step'] / 1e6:8.2f} MB per step   loss {r['loss']:.6f}")
    lin = []
    for M in (2048, 48000):
        r = linear_ab(M, 768, 768, 16, args.repeats)
        lin.append(r)
        k, c = r["kernels_ms"], r["composed_ms"]
        print(f"  adapted linear M={M} K=N=768 r=16: wipa_lora_fwd + wipa_lora_bwd {min(k):7.3f} ms (mean {sum(k) / len(k):.3f})   composed from "
              f"wipa_gemm / wipa_sum_slabs {min(c):7.3f} ms (mean {sum(c) / len(c):.3f})   kernels / composed {min(k) / min(c):.3f}   "
              f"results {max(r['max_rel_apart'].values()):.1e} apart")
    print(json.dumps({"lora_bench": {"steps": rows, "adapted_linear": lin}}))


if __name__ == "__main__":
    main()
