#!/usr/bin/env python3
"""Cost of prompt conditioning in one transcribe round: whisper-small bf16, synthetic weights, B windows (default 64), histories of
random text ids with a timestamp every ninth token.  Between HIP events on the library stream, after warm-up, per repeat (every figure
is a whole host call: cross-attention set-up + begin + what is named):
  pass_full     the batched prompt pass (wipa_decoder_prefill_ragged) alone, every row with a 223-token history: P = 227
  pass_mixed    the same with histories of 0 .. 223 tokens spread over the rows (P = 227 as well: the longest row sets it)
  walk_full / walk_mixed   the same prompts walked column by column by the decode step (WIPA_NO_PREFILL=1)
  step_ragged   one decode step with starts at columns 235 .. 266: (round of 40 new tokens - round of 8) / 32, timestamp rules on
  step_plain    the same columns without starts (the parent commit's step: a 3-token prompt generating up to the same columns), rules on
  round_cond    decode(prompts=...) of the mixed batch, 64 new tokens: a conditioned transcribe round after the encoder
  round_plain   decode() without prompts, 64 new tokens: the unconditioned round
Prints means and run-to-run spreads and one JSON line.
usage: python tools/prompt_bench.py [--batch 64] [--repeats 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd.decoding import _suppress_lists, greedy_decode_tokens, ragged_decode_tokens, timestamp_rules  # noqa: E402
from whisper_ipa_amd.runtime import on_stream  # noqa: E402


def _stats(t):
    t = sorted(t)
    return {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import warnings

    from whisper_ipa_amd.tokenizer import get_tokenizer

    B = args.batch
    model = bench.build_model("small")
    dims = model.dims
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    sot = list(tok.sot_sequence)
    tb = int(tok.timestamp_begin)
    rng = np.random.default_rng(0)

    def history(n):
        body = [int(t) for t in rng.integers(1000, 50000, size=n)]
        for j in range(3, n, 9):
            body[j] = tb + 5 * j
        return body

    full = [history(223) for _ in range(B)]
    mixed = [history(int(round(223 * b / max(B - 1, 1)))) for b in range(B)]
    rows_of = lambda hs: [([tok.sot_prev] + h if h else []) + sot for h in hs]  # noqa: E731
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(B, dims.n_audio_ctx, dims.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, sample_len=64)
    always, first = _suppress_lists(opts, tok)
    rules = timestamp_rules(tok)

    def ragged(rows, new):
        return lambda: ragged_decode_tokens(model, feats, rows, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False, rules=rules,
                                            pad_to=227, sot_back=len(sot))

    def plain(new):
        return lambda: greedy_decode_tokens(model, feats, sot, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False, rules=rules)

    def walked(fn):
        def run():
            os.environ["WIPA_NO_PREFILL"] = "1"
            try:
                fn()
            finally:
                del os.environ["WIPA_NO_PREFILL"]
        return run

    variants = {
        "pass_full": ragged(rows_of(full), 1), "pass_mixed": ragged(rows_of(mixed), 1),
        "walk_full": walked(ragged(rows_of(full), 1)), "walk_mixed": walked(ragged(rows_of(mixed), 1)),
        "ragged_8": ragged(rows_of(mixed), 8), "ragged_40": ragged(rows_of(mixed), 40),
        "plain_232": plain(224 + 8), "plain_264": plain(224 + 40),  # a 3-token prompt reaching the same columns 235 .. 266
        "round_cond": lambda: wipa.decode(model, feats, opts, prompts=mixed),
        "round_plain": lambda: wipa.decode(model, feats, opts),
    }
    times = {k: [] for k in variants}

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with on_stream() as s:
        for fn in variants.values():  # first launches, code objects, graph capture: untimed
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):  # the variants alternate within a repeat so that drift hits all of them
            for name, fn in variants.items():
                times[name].append(timed(fn, s))
    out = {"batch": B, "repeats": args.repeats, "P": 227, "mixed_histories": [len(h) for h in mixed][:: max(B // 8, 1)]}
    print(f"# prompt conditioning, whisper-small bf16 synthetic weights, {B} windows, {args.repeats} repeats, {torch.cuda.get_device_name(0)}")
    for name in variants:
        out[f"{name}_ms"] = r = _stats(times[name])
        print(f"  {name:<12} {r['mean']:9.3f} ms   (min {r['min']:.3f}, max {r['max']:.3f})")
    out["step_ragged_ms"] = (out["ragged_40_ms"]["mean"] - out["ragged_8_ms"]["mean"]) / 32
    out["step_plain_ms"] = (out["plain_264_ms"]["mean"] - out["plain_232_ms"]["mean"]) / 32
    print(f"  step_ragged  {out['step_ragged_ms']:9.4f} ms   step_plain {out['step_plain_ms']:9.4f} ms   "
          f"delta {1e3 * (out['step_ragged_ms'] - out['step_plain_ms']):+.1f} us per step at columns 235 .. 266")
    print(f"  prompt pass / walked prompt: full {out['pass_full_ms']['mean'] / out['walk_full_ms']['mean']:.3f}, "
          f"mixed {out['pass_mixed_ms']['mean'] / out['walk_mixed_ms']['mean']:.3f}")
    print(f"  conditioned round / unconditioned round = {out['round_cond_ms']['mean'] / out['round_plain_ms']['mean']:.3f}")
    print(json.dumps({"prompt_bench": out}))


if __name__ == "__main__":
    main()
