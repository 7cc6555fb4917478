#!/usr/bin/env python3
"""What per-row adapters cost in a decode batch on an MI355X: whisper-small dimensions, synthetic weights, bf16, 64 rows, 7 adapters, r = 16.

(a) The decode step (64 new tokens behind a 4-token prompt pass, replayed step graphs, host wall clock of the synchronised decode,
    cross K / V projection included, also divided by its 67 steps):
    without a bank on the default path of each cross-attention form and on that form's separate-launch cross branch (the branch a
    bank takes: WIPA_ABS_FUSED_PROLOGUE=0 on the absorbed form, WIPA_DECODE_FUSED=0 on the cached one), and with a bank on
    query,value and on all six targets.  A bank on cross_attn.key / value decodes on the cached form, so the all-six row is held
    against the cached rows.  Launches added per step and layer: one wipa_lora_bank_apply per adapted GEMM (attn.query | key | value
    share one), 2 at query,value (q|k|v, cross query), 6 at all six (q|k|v, attn.out, cross query, cross out, mlp1, mlp2).
(b) A 64-token decode of 64 clips spread evenly over 7 languages: ONE batch through the bank, against 7 sub-batches with
    Whisper.set_adapter between them (merge launches, new packed tables, re-captured step graphs), host wall clock, synchronised.
(c) One wipa_lora_bank_apply at 64 x 768 -> 2304 (a layer's q|k|v, three segments) with 1 and with 7 distinct ids, HIP events.
usage: python tools/lora_bank_bench.py [--repeats 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib, lora  # noqa: E402
from whisper_ipa_amd.decoding import greedy_decode_tokens  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402
from whisper_ipa_amd.whisper import Whisper  # noqa: E402

B, NEW, N_ADAPTERS, RANK = 64, 64, 7, 16
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")
INIT, EOT = [50258, 50259, 50359, 50363], 50257
LANGS = [f"l{i}" for i in range(N_ADAPTERS)]


def adapters(dims, targets):
    out = {}
    for i, name in enumerate(LANGS):
        cfg = lora.LoRAConfig(rank=RANK, alpha=32.0, targets=targets, seed=100 + i)
        g = torch.Generator().manual_seed(100 + i)
        out[name] = ({n: (t if n.endswith("lora_A") else 0.02 * torch.randn(t.shape, generator=g)) for n, t in lora.init_adapter(dims, cfg).items()}, cfg)
    return out


def model(cross_attention):
    dims, W = bench.synthetic_weights_small(0, "small")
    m = Whisper(dims, dtype=torch.bfloat16, cross_attention=cross_attention)
    m.load_weights(W)
    return m


def decode_ms(m, feats, repeats, row_ids=None, env=None):
    """ms per decode of NEW tokens (set_audio and the prompt pass included), host wall clock, synchronised: (min, mean) after one warm-up"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ms = []
        for i in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            greedy_decode_tokens(m, feats, INIT, [], [], EOT, max_new_tokens=NEW, stop_on_eot=False, **({"row_ids": row_ids} if row_ids else {}))
            torch.cuda.synchronize()  # (the decode has brought its tokens to the host already)
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        return min(ms), sum(ms) / len(ms)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def part_a(repeats):
    feats = (torch.randn(B, 1500, 768, generator=torch.Generator().manual_seed(1)) * 0.7).to(torch.bfloat16).cuda()
    ids = [i % N_ADAPTERS for i in range(B)]
    rows = []
    for form, sep_env in (("absorbed", {"WIPA_ABS_FUSED_PROLOGUE": "0"}), ("cached", {"WIPA_DECODE_FUSED": "0"})):
        m = model(form)
        rows.append((f"{form}: no bank, default path", decode_ms(m, feats, repeats)))
        rows.append((f"{form}: no bank, separate-launch cross branch", decode_ms(m, feats, repeats, env=sep_env)))
        m.set_adapter_bank(lora.AdapterBank(m.dims, adapters(m.dims, ("attn.query", "attn.value", "cross_attn.query") if form == "absorbed"
                                                             else ("query", "value"))))
        label = "attn.query, attn.value, cross_attn.query (the query,value sites the absorbed form serves)" if form == "absorbed" else "query,value"
        rows.append((f"{form}: bank r{RANK} on {label}", decode_ms(m, feats, repeats, row_ids=ids)))
        if form == "cached":
            m.set_adapter_bank(lora.AdapterBank(m.dims, adapters(m.dims, ALL)))
            rows.append((f"{form}: bank r{RANK} on all six", decode_ms(m, feats, repeats, row_ids=ids)))
        del m
        torch.cuda.empty_cache()
    out = []
    for label, (lo, mean) in rows:
        print(f"  (a) {label:<100} {lo:8.2f} ms per {NEW}-token decode (mean {mean:8.2f}) = {1e3 * lo / (NEW + len(INIT) - 1):7.1f} us per step")
        out.append({"config": label, "decode_ms_min": lo, "decode_ms_mean": mean})
    return out


def part_b(repeats):
    m = model("cached")
    ad = adapters(m.dims, ("query", "value"))
    feats = (torch.randn(B, 1500, 768, generator=torch.Generator().manual_seed(2)) * 0.7).to(torch.bfloat16).cuda()
    ids = [i % N_ADAPTERS for i in range(B)]
    bank = lora.AdapterBank(m.dims, ad)
    res = {"bank": [], "set_adapter": []}
    for i in range(repeats + 1):
        m.set_adapter_bank(bank)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        greedy_decode_tokens(m, feats, INIT, [], [], EOT, max_new_tokens=NEW, stop_on_eot=False, row_ids=ids)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m.set_adapter_bank(None)
        t2 = time.perf_counter()
        for k, name in enumerate(LANGS):
            rows = [b for b in range(B) if ids[b] == k]
            m.set_adapter(*ad[name])
            greedy_decode_tokens(m, feats[rows], INIT, [], [], EOT, max_new_tokens=NEW, stop_on_eot=False)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        m.set_adapter(None)
        if i:
            res["bank"].append((t1 - t0) * 1e3)
            res["set_adapter"].append((t3 - t2) * 1e3)
    for k, v in res.items():
        print(f"  (b) 64 clips x {NEW} tokens over {N_ADAPTERS} languages, {k:<12} {min(v):9.2f} ms (mean {sum(v) / len(v):9.2f})")
    return res


def part_c(repeats):
    L = _lib.lib()
    M, K, N = 64, 768, 2304
    g = torch.Generator().manual_seed(3)
    out = []
    with on_stream() as s:
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
        y = torch.randn(M, N, generator=g).to(torch.bfloat16).cuda()
        A = ((torch.rand(3, N_ADAPTERS, RANK, K, generator=g) * 2 - 1) * K ** -0.5).cuda()
        Bm = (0.02 * torch.randn(3, N_ADAPTERS, N // 3, RANK, generator=g)).cuda()
        gain = torch.full((N_ADAPTERS,), 2.0).cuda()
        for distinct in (1, N_ADAPTERS):
            ids = torch.tensor([i % distinct for i in range(M)], dtype=torch.int32).cuda()
            d = _lib.LoraBankDesc(x=ptr(x), y=ptr(y), out=ptr(y), gain=ptr(gain), ids=ptr(ids), ldx=K, ld=N, M=M, K=K, N=N, r=RANK, n=N_ADAPTERS,
                                  rows_per_id=1, n_seg=3, x_dtype=_lib.WIPA_BF16, y_dtype=_lib.WIPA_BF16)
            for sg in range(3):
                d.A[sg], d.B[sg], d.col_scale[sg] = ptr(A[sg]), ptr(Bm[sg]), 1.0
            ms = []
            for i in range(20 * repeats + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                _lib.check(L.wipa_lora_bank_apply(C.byref(d), sptr(s)), "wipa_lora_bank_apply")
                e1.record(s)
                e1.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            print(f"  (c) wipa_lora_bank_apply {M} x {K} -> {N} bf16, r = {RANK}, {distinct} distinct id(s): {1e3 * min(ms):7.1f} us (mean {1e3 * sum(ms) / len(ms):7.1f})")
            out.append({"distinct_ids": distinct, "us_min": 1e3 * min(ms), "us_mean": 1e3 * sum(ms) / len(ms)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    print(f"# adapter bank: whisper-small bf16 synthetic weights, {B} rows, {N_ADAPTERS} adapters, r = {RANK}, {args.repeats} repeats after one "
          f"warm-up, {torch.cuda.get_device_name(0)}")
    c = part_c(args.repeats)
    a = part_a(args.repeats)
    b = part_b(args.repeats)
    print(json.dumps({"lora_bank_bench": {"step": a, "mixed_batch": b, "apply": c}}))


if __name__ == "__main__":
    main()
