#!/usr/bin/env python3
"""Cost of best-of-N sampling with candidate groups (cfg.dec_n_group: the decode state holds a clip's audio once, every candidate row
reads clip b / G) against the replicated-features decode the library could already run (repeat_interleave + explicit streams):
whisper-small bf16, synthetic weights, W windows x best_of 5, 64 new tokens; absorbed cross-attention with 2 and 4 frame splits, and
cached K / V.  Per shape and form, for both:
  blob_bytes   wipa_decoder_layout(...).total_bytes of the decode state
  set_audio    wipa_decoder_set_audio alone (copy of xa, or the K / V projection of every layer), HIP events around the host call
  step         (a sampling decode of 64 new tokens - one of 16) / 48: one replayed decode step, timestamp rules on
  stream       the launch that reads the audio, alone: the absorbed streaming kernel (WIPA_ABS_STAGES=2 on a scratch a full call
               has filled), or the cached cross-attention launch (wipa_decode_cross_attn[_grouped]); mean over 20 back-to-back launches
  rank         wipa_rank_groups over the W x 5 rows (grouped only: the replicated decode ranks on the host)
HIP events on the library stream, one untimed warm-up of every variant, then --repeats repeats with the variants alternating.
usage: python tools/best_of_bench.py [--windows 16,64] [--repeats 5]"""
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
from whisper_ipa_amd.decoding import (Sampling, _grouped, _packed_for, _rank_groups, _state_for, _suppress_lists, candidate_streams,  # noqa: E402
                                      greedy_decode_tokens, timestamp_rules)
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402

G, NEW = 5, 64


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
    ap.add_argument("--windows", default="16,64")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import warnings

    from whisper_ipa_amd.tokenizer import get_tokenizer

    L = _lib.lib()
    model = bench.build_model("small")
    dims = model.dims
    d, H, Ta = dims.n_text_state, dims.n_text_head, dims.n_audio_ctx
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    sot = list(tok.sot_sequence)
    always, first = _suppress_lists(wipa.DecodingOptions(language="en", without_timestamps=False), tok)
    rules = timestamp_rules(tok)
    out = {"best_of": G, "new_tokens": NEW, "repeats": args.repeats, "shapes": []}
    print(f"# best-of-{G} candidate groups against replicated features, whisper-small bf16 synthetic weights, {NEW} new tokens, "
          f"{args.repeats} repeats, {torch.cuda.get_device_name(0)}")
    for W in [int(w) for w in args.windows.split(",")]:
        B = W * G
        gen = torch.Generator().manual_seed(0)
        feats = torch.randn(W, Ta, d, generator=gen).to(device=model.device, dtype=model.dtype)
        feats_rep = feats.repeat_interleave(G, dim=0).contiguous()
        streams = [(3000 * (w % 7), w) for w in range(W)]
        for form, splits in (("absorbed", 2), ("absorbed", 4), ("cached", 0)):
            model.cross_attention = form
            if form == "absorbed":
                model.cross_splits = splits
            absorbed = form == "absorbed"

            def decode(grouped, new):
                if grouped:
                    return lambda: greedy_decode_tokens(model, feats, sot, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False, rules=rules,
                                                        sample=Sampling(1, 0.8, streams, 1), n_group=G)
                return lambda: greedy_decode_tokens(model, feats_rep, sot, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False,
                                                    rules=rules, sample=Sampling(1, 0.8, candidate_streams(streams, G), 1))

            def set_audio(grouped):
                pk = _packed_for(model, B, NEW)
                pk = _grouped(pk, G) if grouped else pk
                st = _state_for(model, B, pk)
                f = feats if grouped else feats_rep

                def run():
                    with on_stream() as s:
                        _lib.check(L.wipa_decoder_set_audio(C.byref(pk["cfg"]), pk["dec_tab"], ptr(f), ptr(st.blob), st.blob.numel(), B, sptr(s)),
                                   "wipa_decoder_set_audio")
                return run, int(st.layout.total_bytes)

            def stream_launch(grouped):
                """20 back-to-back launches of the kernel that reads the audio"""
                f = feats if grouped else feats_rep
                q = torch.randn(B, d, device=model.device, dtype=model.dtype)
                o = torch.empty_like(q)
                if absorbed:
                    n = int(L.wipa_cross_absorbed_scratch_bytes(B, d, Ta))
                    sc = torch.empty(n, dtype=torch.uint8, device=model.device)
                    w = torch.randn(d, d, device=model.device, dtype=model.dtype) * 0.03
                    bv = torch.zeros(d, device=model.device, dtype=torch.float32)

                    def call(s):
                        _lib.check(L.wipa_cross_absorbed_attention_grouped(ptr(q), d, ptr(w), ptr(f), ptr(w), ptr(bv), ptr(o), d, ptr(sc), n, B, H, d,
                                                                           Ta, 0.35355339, splits, G if grouped else 1, sptr(s)), "absorbed")
                    with on_stream() as s:
                        call(s)  # fills Qp
                else:
                    kv = torch.randn((W if grouped else B) * 2 * H * Ta * 64, device=model.device, dtype=model.dtype)

                    def call(s):
                        _lib.check(L.wipa_decode_cross_attn_grouped(ptr(q), ptr(kv), ptr(o), B, H, Ta, 1, G if grouped else 1, 1, sptr(s)), "cached")

                def run():
                    if absorbed:
                        os.environ["WIPA_ABS_STAGES"] = "2"  # the streaming launch alone
                    try:
                        with on_stream() as s:
                            for _ in range(20):
                                call(s)
                    finally:
                        os.environ.pop("WIPA_ABS_STAGES", None)
                return run

            def rank():
                pk = _grouped(_packed_for(model, B, NEW), G)
                st = _state_for(model, B, pk)

                def run():
                    with on_stream() as s:
                        _rank_groups(st, G, len(sot), NEW, tok.eot, None, s)
                return run

            sa_g, bytes_g = set_audio(True)
            sa_r, bytes_r = set_audio(False)
            variants = {"grouped_16": decode(True, 16), "grouped_64": decode(True, NEW), "replicated_16": decode(False, 16),
                        "replicated_64": decode(False, NEW), "set_audio_grouped": sa_g, "set_audio_replicated": sa_r,
                        "stream_grouped": stream_launch(True), "stream_replicated": stream_launch(False), "rank": rank()}
            times = {k: [] for k in variants}
            with on_stream() as s:
                for fn in variants.values():
                    fn()
                torch.cuda.synchronize()
                for _ in range(args.repeats):
                    for name, fn in variants.items():
                        times[name].append(timed(fn, s))
            r = {"windows": W, "rows": B, "form": form, "cross_splits": splits, "blob_bytes_grouped": bytes_g, "blob_bytes_replicated": bytes_r}
            for k in variants:
                r[f"{k}_ms"] = _stats(times[k])
            for k in ("grouped", "replicated"):
                r[f"step_{k}_ms"] = (r[f"{k}_64_ms"]["mean"] - r[f"{k}_16_ms"]["mean"]) / (NEW - 16)
                r[f"stream_{k}_us"] = 1e3 * r[f"stream_{k}_ms"]["mean"] / 20
            out["shapes"].append(r)
            name = f"{form}" + (f" {splits} splits" if absorbed else "")
            print(f"{W} windows x {G} = {B} rows, {name}")
            print(f"  blob         grouped {bytes_g / 1e9:8.3f} GB   replicated {bytes_r / 1e9:8.3f} GB")
            print(f"  set_audio    grouped {r['set_audio_grouped_ms']['mean']:8.3f} ms   replicated {r['set_audio_replicated_ms']['mean']:8.3f} ms")
            print(f"  step         grouped {r['step_grouped_ms']:8.4f} ms   replicated {r['step_replicated_ms']:8.4f} ms")
            print(f"  stream       grouped {r['stream_grouped_us']:8.1f} us   replicated {r['stream_replicated_us']:8.1f} us   (per layer)")
            print(f"  decode of {NEW} grouped {r['grouped_64_ms']['mean']:8.2f} ms (min {r['grouped_64_ms']['min']:.2f} max {r['grouped_64_ms']['max']:.2f})   "
                  f"replicated {r['replicated_64_ms']['mean']:8.2f} ms (min {r['replicated_64_ms']['min']:.2f} max {r['replicated_64_ms']['max']:.2f})")
            print(f"  rank         {1e3 * r['rank_ms']['mean']:8.1f} us (host call with the read-back of {W} rows)")
            for st in list(model.__dict__.get("_dec_states", {}).values()):  # the 17 GB blobs of the cached form do not pile up
                st.release()
            model.__dict__["_dec_states"] = {}
            torch.cuda.empty_cache()
    print(json.dumps({"best_of_bench": out}))


if __name__ == "__main__":
    main()
