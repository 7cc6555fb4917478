#!/usr/bin/env python3
"""Cost of the timestamp rules in the replayed decode step: whisper-small bf16, synthetic weights, B clips (default 64), one pass in
flight.  Per repeat and variant: prompt prefill, two warm steps, then N steps replayed from the captured graph between two HIP events;
the variants alternate within a repeat so that drift hits both.  Rules off is the plain step (the logits projection carries the greedy
partials and no step but the last writes its logits); rules on is a call with wipa_decode_call.rules: every step writes its logits (B x 51 865 f32)
and the row-scan tail reads them back, scans the row's history and makes two reductions.  Both variants use the same three-token
prompt, so they time the same positions.  Prints the mean and the run-to-run spread in us per step and one JSON line.
usage: python tools/timestamp_step_bench.py [--batch 64] [--steps 48] [--repeats 7]"""
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
from whisper_ipa_amd.decoding import _mask, _packed_for, _state_for, decode_call  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a step time is a device measurement"
    L = _lib.lib()
    B = args.batch
    model = bench.build_model("small")
    init4, always, first, eot = bench.decode_setup()
    init = init4[:3]  # sot, language, task: the timestamp path's prompt, used for both variants
    rules = _lib.DecodeRules(init4[3] + 1, init4[3], 50)
    n_init = len(init)
    pk = _packed_for(model, B, args.steps + 4)
    st = _state_for(model, B, pk)
    m_always, m_first = _mask(model, always), _mask(model, list(always) + list(first))
    host_init = (C.c_int32 * n_init)(*init)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(B, model.dims.n_audio_ctx, model.dims.n_audio_state, generator=g).to(device=model.device, dtype=model.dtype)
    cfg, tab, blob, nb = C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel()

    def one(with_rules: bool, s) -> float:
        call = decode_call(n_init, eot, m_first, m_always, rules if with_rules else None)
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

    variants = [False, True]
    times = {v: [] for v in variants}
    with on_stream() as s:
        _lib.check(L.wipa_decoder_set_audio(cfg, tab, ptr(feats), blob, nb, B, sptr(s)), "wipa_decoder_set_audio")
        for v in variants:  # graph capture and first launches, untimed
            one(v, s)
        for _ in range(args.repeats):
            for v in variants:
                times[v].append(one(v, s))
    print(f"# replayed decode step, whisper-small bf16 synthetic weights, B = {B}, {args.steps} steps x {args.repeats} repeats, "
          f"{torch.cuda.get_device_name(0)}")
    out = {"batch": B, "steps": args.steps, "repeats": args.repeats}
    for v in variants:
        t = sorted(times[v])
        name = "rules_on" if v else "rules_off"
        out[name + "_us"] = {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}
        print(f"  {name:<9} {sum(t) / len(t):8.1f} us per step   (min {t[0]:.1f}, max {t[-1]:.1f} over {len(t)} repeats)")
    out["rules_cost_us"] = out["rules_on_us"]["mean"] - out["rules_off_us"]["mean"]
    print(f"  the rules cost {out['rules_cost_us']:+.1f} us per step ({100.0 * out['rules_cost_us'] / out['rules_off_us']['mean']:+.1f} %)")
    print(json.dumps({"timestamp_step_bench": out}))


if __name__ == "__main__":
    main()
