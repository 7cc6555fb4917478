#!/usr/bin/env python3
"""Cost of temperature sampling in the replayed decode step: whisper-small bf16, synthetic weights, B clips (default 64), one pass in
flight, the timestamp rules on in both variants.  Per repeat and variant: prompt prefill, two warm steps, then N steps replayed from
the captured graph between two HIP events; the variants alternate within a repeat so that drift hits both.  Temperature 0 is
the call with rules alone, unchanged by the sampling work; the sampled step adds wipa_decode_call.sample to the same rules: the same
logits GEMM and written logits, and a tail that adds one Philox4x32-10 call per alive quad, two logf per alive column and a third
(max, lowest column) reduction.  A second table times the two tails ALONE on B x 51 865 random logits (wipa_timestamp_step against
wipa_sample_step, no embedding), which is what to hold against the step's logits GEMM.  Prints means and run-to-run spreads in us
and one JSON line.
usage: python tools/sample_step_bench.py [--batch 64] [--steps 48] [--repeats 7] [--temperature 0.6]"""
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
from whisper_ipa_amd.decoding import Sampling, _mask, _packed_for, _state_for, decode_call  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402


def _stats(t):
    t = sorted(t)
    return {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--temperature", type=float, default=0.6)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a step time is a device measurement"
    L = _lib.lib()
    B = args.batch
    model = bench.build_model("small")
    init4, always, first, eot = bench.decode_setup()
    init = init4[:3]  # sot, language, task: the timestamp path's prompt
    rules = _lib.DecodeRules(init4[3] + 1, init4[3], 50)
    n_init = len(init)
    V = model.dims.n_vocab
    pk = _packed_for(model, B, args.steps + 4)
    st = _state_for(model, B, pk)
    m_always, m_first = _mask(model, always), _mask(model, list(always) + list(first))
    host_init = (C.c_int32 * n_init)(*init)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(B, model.dims.n_audio_ctx, model.dims.n_audio_state, generator=g).to(device=model.device, dtype=model.dtype)
    cfg, tab, blob, nb = C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel()

    def one(sampled: bool, s, rec) -> float:
        call = decode_call(n_init, eot, m_first, m_always, rules, rec if sampled else None)
        head = (cfg, tab, blob, nb, B, C.byref(call))
        _lib.check(L.wipa_decoder_begin(cfg, blob, nb, B, host_init, n_init, sptr(s)), "wipa_decoder_begin")
        _lib.check(L.wipa_decoder_prefill_ex(*head, 1, sptr(s)), "prefill")
        _lib.check(L.wipa_decoder_run_ex(*head, 2, 1, sptr(s)), "warm steps")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _lib.check(L.wipa_decoder_run_ex(*head, args.steps, 1, sptr(s)), "timed steps")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.steps

    def tail_alone(sampled: bool, s, rec, lg, tk, pos, slp, nd, n=50) -> float:
        ldl, ld_tok = lg.shape[1], tk.shape[1]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(n + 3):
            if i == 3:
                e0.record(s)
            if sampled:
                _lib.check(L.wipa_sample_step(ptr(lg), ldl, B, V, ptr(m_first), ptr(m_always), ptr(tk), ld_tok, ptr(pos), n_init, eot, C.byref(rules),
                                              ptr(rec), ptr(slp), ptr(nd), sptr(s)), "wipa_sample_step")
            else:
                _lib.check(L.wipa_timestamp_step(ptr(lg), ldl, B, V, ptr(m_first), ptr(m_always), ptr(tk), ld_tok, ptr(pos), n_init, eot,
                                                 C.byref(rules), ptr(slp), ptr(nd), sptr(s)), "wipa_timestamp_step")
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    variants = [False, True]
    times = {v: [] for v in variants}
    tails = {v: [] for v in variants}
    with on_stream() as s:
        rec = st.sample_record(Sampling(1, args.temperature))
        _lib.check(L.wipa_decoder_set_audio(cfg, tab, ptr(feats), blob, nb, B, sptr(s)), "wipa_decoder_set_audio")
        for v in variants:  # graph capture and first launches, untimed
            one(v, s, rec)
        for _ in range(args.repeats):
            for v in variants:
                times[v].append(one(v, s, rec))
        # the tails alone: text after text (history a, b after an opening pair), every text column and the later timestamps alive
        ldl = (V + 3) // 4 * 4
        lg = (torch.randn(B, ldl, generator=g) * 2.0).to(model.device)
        hist = list(init) + [rules.timestamp_begin, rules.timestamp_begin, 1200, 2400]
        tk = torch.zeros(B, 16, dtype=torch.int32, device=model.device)
        tk[:, : len(hist)] = torch.tensor(hist, dtype=torch.int32, device=model.device)
        pos = torch.tensor([len(hist) - 1], dtype=torch.int32, device=model.device)
        slp = torch.zeros(B, dtype=torch.float32, device=model.device)
        nd = torch.zeros(1, dtype=torch.int32, device=model.device)
        for _ in range(args.repeats):
            for v in variants:
                tails[v].append(tail_alone(v, s, rec, lg, tk, pos, slp, nd))
    print(f"# replayed decode step with the timestamp rules, whisper-small bf16 synthetic weights, B = {B}, {args.steps} steps x "
          f"{args.repeats} repeats, temperature {args.temperature}, {torch.cuda.get_device_name(0)}")
    out = {"batch": B, "steps": args.steps, "repeats": args.repeats, "temperature": args.temperature}
    for table, label in ((times, "step"), (tails, "tail_alone")):
        for v in variants:
            name = f"{label}_{'sampled' if v else 'temperature0'}_us"
            out[name] = _stats(table[v])
            print(f"  {name:<28} {out[name]['mean']:8.1f} us   (min {out[name]['min']:.1f}, max {out[name]['max']:.1f} over {len(table[v])} repeats)")
        a, b = out[f"{label}_temperature0_us"]["mean"], out[f"{label}_sampled_us"]["mean"]
        out[f"{label}_ratio"] = b / a
        print(f"  {label}: sampled / temperature 0 = {b / a:.3f} ({b - a:+.1f} us)")
    print(json.dumps({"sample_step_bench": out}))


if __name__ == "__main__":
    main()
