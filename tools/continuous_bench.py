#!/usr/bin/env python3
"""Continuous-batching decode against lockstep decode on ragged output lengths: whisper-small bf16, synthetic weights, 256 clips
(random features), 64 slots.  Clip i generates exactly as many tokens as transcript i of tests/golden/combined_test_ipa.json has in this
process's tokenizer (clamped to n_text_ctx // 2); EOT is suppressed in both decodes so that synthetic weights cannot end a row early.
  lockstep     wipa.decode over the clips in file order, four batches of 64, each run to its longest row (sample_len = that length)
  continuous   wipa.decode_continuous(slots=64, sample_lens=lengths, check_every=8)
Recorded: the generating steps both ways, the lower bound on the continuous steps and on the ratio that follows from the lengths alone
(computable without a GPU: --lengths-only), wall time of both after a warm-up, and the per-step time of the continuous step against the
plain step (the step of greedy_decode_tokens, whose kernels this change leaves as they were: profiles/continuous_kernel_diff.txt),
both over columns 8 .. 72 of 64 rows, between HIP events.  Prints a report and one JSON line.
usage: python tools/continuous_bench.py [--clips 256] [--slots 64] [--repeats 3] [--lengths-only]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
from whisper_ipa_amd.continuous import (DeviceStepper, ScheduleStats, continuous_steps_bound, lockstep_steps, run_schedule)  # noqa: E402
from whisper_ipa_amd.tokenizer import get_tokenizer  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "combined_test_ipa.json")
N_INIT = 4  # <|startoftranscript|> <|en|> <|transcribe|> <|notimestamps|>


def lengths(tok, n_clips: int, cap: int):
    items = json.load(open(GOLDEN))[:n_clips]
    return [max(1, min(cap, len(tok.encode(" " + it["ipa_transcription"].strip())))) for it in items]


class _Dry:
    """run_schedule's stepper with rows that never say EOT: the schedule of forced lengths without a GPU"""

    def __init__(self, slots):
        self.slots = slots

    def admit(self, pairs): pass
    def run(self, n): pass
    def last_tokens(self): return [0] * self.slots
    def retire(self, *a): pass
    def shift(self, n): pass


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lengths-only", action="store_true", help="the step counts and the bound only: no GPU")
    args = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    n_ctx = 448
    lens = lengths(tok, args.clips, n_ctx // 2)
    N, S, ce = len(lens), args.slots, args.check_every
    lock = lockstep_steps(lens, S)
    bound = continuous_steps_bound(lens, S, N_INIT, ce)
    dry = run_schedule(_Dry(S), N, S, N_INIT, lens, -1, n_ctx, ce)
    out = {"clips": N, "slots": S, "check_every": ce, "tokenizer": "byte-fallback" if tok.byte_fallback else "tiktoken",
           "lengths": {"min": min(lens), "max": max(lens), "mean": sum(lens) / N, "sum": sum(lens)},
           "lockstep_generating_steps": lock, "lockstep_steps_with_prompt": lock + (N_INIT - 1) * -(-N // S),
           "continuous_steps_lower_bound": bound, "continuous_steps": dry.steps, "continuous_shifts": dry.shifts,
           "ratio_lower_bound": bound / lock, "ratio_steps": dry.steps / lock}
    print(f"# {N} clips, {S} slots, check every {ce}: lengths {min(lens)} .. {max(lens)}, mean {sum(lens) / N:.1f}")
    print(f"  lockstep generating steps   {lock}   (+ {N_INIT - 1} prompt columns per batch, taken by one prompt pass each)")
    print(f"  continuous steps            {dry.steps}   (lower bound from the lengths {bound}; shifts {dry.shifts})")
    print(f"  steps continuous / lockstep {dry.steps / lock:.3f}   (bound {bound / lock:.3f})")
    if args.lengths_only:
        print(json.dumps({"continuous_bench": out}))
        return
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import bench
    from whisper_ipa_amd.decoding import _suppress_lists, greedy_decode_tokens
    from whisper_ipa_amd.runtime import on_stream

    model = bench.build_model("small")
    d = model.dims
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(N, d.n_audio_ctx, d.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    opts = wipa.DecodingOptions(language="en", without_timestamps=True, suppress_tokens=[-1, int(tok.eot)])

    def lockstep():
        res = []
        for i in range(0, N, S):
            res += wipa.decode(model, feats[i:i + S], opts, sample_len=max(lens[i:i + S]))
        return res

    stats = []

    def continuous():
        stats.clear()
        return wipa.decode_continuous(model, feats, opts, slots=S, sample_lens=lens, check_every=ce, stats_out=stats)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), res

    _, a = wall(lockstep)  # first launches, code objects, graph capture: untimed
    _, b = wall(continuous)
    full = sum(len(r.tokens) == n for r, n in zip(b, lens))
    same = sum(r.tokens[:n] == q.tokens[:n] for r, q, n in zip(b, a, lens))
    t_lock, t_cont = [], []
    for _ in range(args.repeats):  # alternating, so that drift hits both
        t_lock.append(wall(lockstep)[0])
        t_cont.append(wall(continuous)[0])
    st: ScheduleStats = stats[0]
    out.update(lockstep_ms=sorted(t_lock), continuous_ms=sorted(t_cont), continuous_steps_run=st.steps, continuous_shifts_run=st.shifts,
               admissions=len(st.admissions), rows_at_full_length=full, rows_equal_to_lockstep=same,
               lockstep_forms=["absorbed" if model.use_absorbed(S, max(lens[i:i + S])) else "cached" for i in range(0, N, S)],
               continuous_form="absorbed" if model.use_absorbed() else "cached")
    # per-step time over columns 8 .. 72 of 64 rows: (a call of 72 steps - a call of 8 steps) / 64, as tools/prompt_bench.py does
    always, first = _suppress_lists(opts, tok)
    init = list(tok.sot_sequence_including_notimestamps)

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def plain(n):
        return lambda: greedy_decode_tokens(model, feats[:S], init, always, first, tok.eot, max_new_tokens=n, stop_on_eot=False)

    with on_stream() as s:
        def cont(n):
            def run():
                stp = DeviceStepper(model, S, lambda c: feats[c], lambda c: init, len(init), [200] * S, tok.eot, always, first, None, s)
                stp.admit([(b, b) for b in range(S)])
                stp.run(n + len(init) - 1)
            return run

        variants = {"plain_8": plain(8), "plain_72": plain(72), "cont_8": cont(8), "cont_72": cont(72)}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(max(args.repeats, 3)):
            for k, fn in variants.items():
                times[k].append(timed(fn, s))
    mean = {k: sum(v) / len(v) for k, v in times.items()}
    out["step_plain_ms"] = (mean["plain_72"] - mean["plain_8"]) / 64
    out["step_continuous_ms"] = (mean["cont_72"] - mean["cont_8"]) / 64
    out["admit_64_rows_plus_8_steps_ms"] = mean["cont_8"]
    ml, mc = sum(t_lock) / len(t_lock), sum(t_cont) / len(t_cont)
    print(f"# whisper-small bf16 synthetic weights, {torch.cuda.get_device_name(0)}, {args.repeats} repeats")
    print(f"  lockstep    {ml:9.1f} ms wall   (min {min(t_lock):.1f}, max {max(t_lock):.1f}); forms {out['lockstep_forms']}")
    print(f"  continuous  {mc:9.1f} ms wall   (min {min(t_cont):.1f}, max {max(t_cont):.1f}); form {out['continuous_form']}; "
          f"{st.steps} steps, {len(st.admissions)} admissions, shifts {st.shifts}")
    print(f"  wall continuous / lockstep = {mc / ml:.3f}")
    print(f"  rows that generated their full length {full} / {N}; rows whose ids equal lockstep's {same} / {N} (bf16, lively synthetic "
          f"weights: margins are not gated here, the parity claims live in tests/test_gpu_continuous.py)")
    print(f"  step_continuous {out['step_continuous_ms']:.4f} ms   step_plain {out['step_plain_ms']:.4f} ms   "
          f"delta {1e3 * (out['step_continuous_ms'] - out['step_plain_ms']):+.1f} us per step (columns 8 .. 72, 64 rows)")
    print(json.dumps({"continuous_bench": out}))


if __name__ == "__main__":
    main()
