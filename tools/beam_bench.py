#!/usr/bin/env python3
"""Cost of beam search on the device against the grouped best-of-5 sampling decode on the same rows: whisper-small
bf16, synthetic weights, W windows x beam 5 = best_of 5, 64 new tokens, timestamp rules on, absorbed cross-attention with 4 frame splits.
  step         (a decode of 64 new tokens - one of 16) / 48: one replayed decode step, for beams (patience 1) and for best-of
  decode       the whole decode of 64 new tokens, ranking / finalize and the read-back of W rows included
  self_attn    the self-attention launch alone at 224 keys on W x 5 rows: wipa_decode_attn, wipa_decode_attn_beam with the identity
               table and with a random table (every key from another row of the clip); mean over 20 back-to-back launches
  tail         wipa_beam_step alone (its two launches, beam_topk + beam_select, without the embedding) against wipa_sample_step, the
               one-launch tail of the sampling decode; mean over 20 back-to-back calls
  beam_bytes   wipa_beam_bytes of the shape
HIP events on the library stream, one untimed warm-up of every variant, then --repeats repeats with the variants alternating.
The alternative to the ancestor table, a physical gather of the KV cache, would move n_layer x 2 x rows x p x d elements per step each
way: printed as ARITHMETIC from the sizes, not measured.
usage: python tools/beam_bench.py [--windows 64] [--repeats 5]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib  # noqa: E402
from whisper_ipa_amd.decoding import Beams, Sampling, _suppress_lists, greedy_decode_tokens, timestamp_rules  # noqa: E402
from whisper_ipa_amd.ops import dt_code  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402

G, NEW, KEYS, LAUNCHES = 5, 64, 224, 20


def _stats(t):
    t = sorted(t)
    return {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import warnings

    from whisper_ipa_amd.tokenizer import get_tokenizer

    L = _lib.lib()
    model = bench.build_model("small")
    model.cross_attention, model.cross_splits = "absorbed", 4
    dims = model.dims
    d, H, Ta, V, n_ctx = dims.n_text_state, dims.n_text_head, dims.n_audio_ctx, dims.n_vocab, dims.n_text_ctx
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    sot = list(tok.sot_sequence)
    always, first = _suppress_lists(wipa.DecodingOptions(language="en", without_timestamps=False), tok)
    rules = timestamp_rules(tok)
    W = args.windows
    B = W * G
    dev = model.device
    gen = torch.Generator().manual_seed(0)
    feats = torch.randn(W, Ta, d, generator=gen).to(device=dev, dtype=model.dtype)
    streams = [(3000 * (w % 7), w) for w in range(W)]

    def decode(beams, new):
        if beams:
            return lambda: greedy_decode_tokens(model, feats, sot, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False, rules=rules,
                                                n_group=G, beams=Beams(G))
        return lambda: greedy_decode_tokens(model, feats, sot, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False, rules=rules,
                                            sample=Sampling(1, 0.8, streams, 1), n_group=G, rank=True)

    # ---- the self-attention launch at KEYS keys
    q = torch.randn(B, n_ctx, H, 64, generator=gen).to(device=dev, dtype=model.dtype)
    k = torch.randn(B, n_ctx, H, 64, generator=gen).to(device=dev, dtype=model.dtype)
    v = torch.randn(B, n_ctx, H, 64, generator=gen).to(device=dev, dtype=model.dtype)
    o = torch.empty(B, H, 64, device=dev, dtype=model.dtype)
    ld_tok = n_ctx + 8
    identity = (torch.arange(B) % G)[:, None].expand(B, ld_tok).contiguous().to(torch.uint8).to(dev)
    random_table = torch.randint(0, G, (B, ld_tok), generator=gen).to(torch.uint8).to(dev)
    desc = _lib.AttnDesc()
    desc.q, desc.k, desc.v, desc.out = ptr(q), ptr(k), ptr(v), ptr(o)
    desc.q_bs, desc.q_rs, desc.q_hs = q.stride(0), q.stride(1), q.stride(2)
    desc.k_bs, desc.k_rs, desc.k_hs = k.stride(0), k.stride(1), k.stride(2)
    desc.v_bs, desc.v_rs, desc.v_hs = v.stride(0), v.stride(1), v.stride(2)
    desc.o_bs, desc.o_rs, desc.o_hs = o.stride(0), o.stride(0), o.stride(1)
    desc.B, desc.H, desc.Tq, desc.Tk, desc.causal, desc.dtype = B, H, 1, KEYS, 0, dt_code(model.dtype)

    def attn(table):
        def run():
            with on_stream() as s:
                for _ in range(LAUNCHES):
                    if table is None:
                        _lib.check(L.wipa_decode_attn(C.byref(desc), sptr(s)), "wipa_decode_attn")
                    else:
                        _lib.check(L.wipa_decode_attn_beam(C.byref(desc), ptr(table), ld_tok, G, sptr(s)), "wipa_decode_attn_beam")
        return run

    # ---- the tails on written logits
    ldl = (V + 7) // 8 * 8
    logits = torch.randn(B, ldl, generator=gen).to(dev)
    mask = torch.zeros(V, device=dev)
    tokens = torch.zeros(B, ld_tok, dtype=torch.int32, device=dev)
    tokens[:, :3] = torch.tensor(sot, dtype=torch.int32)
    tokens[:, 3:40] = torch.randint(1000, 40000, (B, 37), generator=gen).to(torch.int32).to(dev)
    pos = torch.tensor([39], dtype=torch.int32, device=dev)
    sums = torch.zeros(B, dtype=torch.float32, device=dev)
    nd = torch.zeros(1, dtype=torch.int32, device=dev)
    beam_bytes = int(L.wipa_beam_bytes(B, G, G, ld_tok))
    buf = torch.zeros(beam_bytes, dtype=torch.uint8, device=dev)
    rec_host = torch.zeros(int(L.wipa_sample_record_bytes(B)), dtype=torch.uint8)
    flat = (C.c_uint32 * (2 * B))(*[x for b in range(B) for x in (b, 0)])
    _lib.check(L.wipa_sample_record_fill(rec_host.numpy().ctypes.data, rec_host.numel(), 1, 1, 0.8, flat, B), "wipa_sample_record_fill")
    rec = rec_host.to(dev)
    with on_stream() as s:
        _lib.check(L.wipa_beam_begin(ptr(buf), beam_bytes, B, G, G, ld_tok, sptr(s)), "wipa_beam_begin")

    def beam_tail():
        with on_stream() as s:
            for _ in range(LAUNCHES):
                _lib.check(L.wipa_beam_step(ptr(logits), ldl, B, V, ptr(mask), ptr(mask), ptr(tokens), ld_tok, ptr(pos), 3, tok.eot, C.byref(rules),
                                            ptr(buf), G, G, ptr(sums), ptr(nd), sptr(s)), "wipa_beam_step")

    def sample_tail():
        with on_stream() as s:
            for _ in range(LAUNCHES):
                _lib.check(L.wipa_sample_step(ptr(logits), ldl, B, V, ptr(mask), ptr(mask), ptr(tokens), ld_tok, ptr(pos), 3, tok.eot, C.byref(rules),
                                              ptr(rec), ptr(sums), ptr(nd), sptr(s)), "wipa_sample_step")

    variants = {"beam_16": decode(True, 16), "beam_64": decode(True, NEW), "best_of_16": decode(False, 16), "best_of_64": decode(False, NEW),
                "attn_plain": attn(None), "attn_beam_identity": attn(identity), "attn_beam_random": attn(random_table),
                "tail_beam": beam_tail, "tail_sample": sample_tail}
    times = {name: [] for name in variants}
    with on_stream() as s:
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, fn in variants.items():
                times[name].append(timed(fn, s))
    r = {name + "_ms": _stats(t) for name, t in times.items()}
    r.update(windows=W, rows=B, beam_size=G, new_tokens=NEW, keys=KEYS, repeats=args.repeats, beam_bytes=beam_bytes)
    for kind in ("beam", "best_of"):
        r[f"step_{kind}_ms"] = (r[f"{kind}_64_ms"]["mean"] - r[f"{kind}_16_ms"]["mean"]) / (NEW - 16)
    e = 2  # bf16
    gather_bytes = dims.n_text_layer * 2 * B * KEYS * d * e
    print(f"# beam search against grouped best-of-{G} sampling, whisper-small bf16 synthetic weights, {W} windows x {G} = {B} rows, {NEW} new "
          f"tokens, absorbed cross-attention with 4 splits, rules on, {args.repeats} repeats, {torch.cuda.get_device_name(0)}")
    print(f"  step         beam {r['step_beam_ms']:8.4f} ms   best-of {r['step_best_of_ms']:8.4f} ms")
    for kind, label in (("beam", "beam   "), ("best_of", "best-of")):
        m = r[f"{kind}_64_ms"]
        print(f"  decode of {NEW} {label} {m['mean']:8.2f} ms (min {m['min']:.2f} max {m['max']:.2f})")
    for name, label in (("attn_plain", "wipa_decode_attn               "), ("attn_beam_identity", "wipa_decode_attn_beam, identity"),
                        ("attn_beam_random", "wipa_decode_attn_beam, random  ")):
        print(f"  self_attn    {label} {1e3 * r[name + '_ms']['mean'] / LAUNCHES:8.1f} us at {KEYS} keys (per layer)")
    print(f"  tail         wipa_beam_step (beam_topk + beam_select) {1e3 * r['tail_beam_ms']['mean'] / LAUNCHES:8.1f} us   "
          f"wipa_sample_step {1e3 * r['tail_sample_ms']['mean'] / LAUNCHES:8.1f} us")
    print(f"  beam_bytes   {beam_bytes} ({beam_bytes / 1e6:.2f} MB)")
    print(f"  a physical gather of the KV cache at {KEYS} positions would read {gather_bytes / 1e9:.2f} GB and write as much per step "
          "(arithmetic from the sizes, not a measurement)")
    print(json.dumps({"beam_bench": r}))


if __name__ == "__main__":
    main()
