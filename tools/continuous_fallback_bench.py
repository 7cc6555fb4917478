#!/usr/bin/env python3
"""The temperature fallback on the continuous schedule: whisper-small bf16, synthetic weights, the setting of
tools/continuous_rules_bench.py.
  step       one continuous step with rules over 64 rows, columns 8 .. 72: (a call of 72 steps - a call of 8 steps) / 64 between HIP
             events, median of the repeats, the variants alternating --
               rules       a continuous call with rules, the tail without a sampling record (what a decode without per-row
                           temperatures launches)
               sample_0.6  the same call with the one-temperature sampling record at 0.6 (the existing sampling tail)
               rows_0      the call with wipa_decode_call.sample_rows, every row greedy
               rows_0.6    the same call, every row at temperature 0.6
               rows_half   the same call, every second row at 0.6, the others greedy
  schedules  wipa.transcribe(seed=3) on the 24 files of tools/continuous_rules_bench.py (sample_len 32): schedule="rounds" against
             schedule="continuous" with 24 and with 8 slots -- wall time, decoder steps, retries per window.  With random weights the
             average log-probability of nearly every window lies far below the threshold, so nearly every window runs the whole
             schedule: this is the bookkeeping's worst case, not a speed claim.
Prints a report and one JSON line.
usage: python tools/continuous_fallback_bench.py [--repeats 5] [--files 24]"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
from whisper_ipa_amd.continuous import DeviceStepper  # noqa: E402
from whisper_ipa_amd.decoding import Sampling  # noqa: E402
from whisper_ipa_amd.tokenizer import get_tokenizer  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from continuous_rules_bench import mixed_files, wall  # noqa: E402

SEED = 3


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--files", type=int, default=24)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import bench
    from whisper_ipa_amd.decoding import _suppress_lists, timestamp_rules
    from whisper_ipa_amd.runtime import on_stream
    from whisper_ipa_amd.transcribe import _model_decoder

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    model = bench.build_model("small")
    d = model.dims
    S, ce, reps = args.slots, args.check_every, max(args.repeats, 5)
    out = {"slots": S, "check_every": ce, "repeats": reps, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(S, d.n_audio_ctx, d.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, suppress_tokens=[-1, int(tok.eot)])

    # ---- step: (72 steps - 8 steps) / 64, 64 rows, with rules
    always, first = _suppress_lists(opts, tok)
    rules = timestamp_rules(tok, opts.max_initial_timestamp)
    init = list(tok.sot_sequence)

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with on_stream() as s:
        def cont(n, temperature_of):
            """temperature_of: None -- the entry point without a record; a number -- the same entry point with the one-temperature
            record; else slot -> temperature, through the entry point with a temperature per row"""
            def run():
                rows = callable(temperature_of)
                one = Sampling(SEED, float(temperature_of), None, 0) if temperature_of is not None and not rows else None
                stp = DeviceStepper(model, S, lambda c: feats[c], lambda c: init, len(init), [200] * S, tok.eot, always, first, one, s,
                                    rules=rules, no_speech_token=tok.no_speech, row_seed=SEED if rows else None,
                                    draws=(lambda c: (temperature_of(c), 0, (c, 0)) if temperature_of(c) else None) if rows else None)
                stp.admit([(b, b) for b in range(S)])
                stp.run(n + len(init) - 1)
            return run

        kinds = {"rules": None, "sample_0.6": 0.6, "rows_0": lambda c: 0.0, "rows_0.6": lambda c: 0.6, "rows_half": lambda c: 0.6 if c % 2 else 0.0}
        variants = {f"{k}_{n}": cont(n, t) for n in (8, 72) for k, t in kinds.items()}
        for fn in variants.values():  # first launches, code objects, graph capture: untimed
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(reps):  # alternating, so that drift hits all
            for k, fn in variants.items():
                times[k].append(timed(fn, s))
    per_repeat = {k: [(b - a) / 64 for a, b in zip(times[f"{k}_8"], times[f"{k}_72"])] for k in kinds}
    step = {k: (median(times[f"{k}_72"]) - median(times[f"{k}_8"])) / 64 for k in kinds}
    out["step_ms"] = step
    out["step_ms_per_repeat"] = per_repeat
    print(f"# one continuous step with rules, {S} rows, columns 8 .. 72 (median of {reps} calls each, HIP events); whisper-small bf16 "
          f"synthetic weights, {out['device']}")
    for k in kinds:
        v = per_repeat[k]
        print(f"  {k:10s} {1e3 * step[k]:8.1f} us   (per repeat: min {1e3 * min(v):.1f}, max {1e3 * max(v):.1f})")
    spread = 1e3 * (max(per_repeat["rules"]) - min(per_repeat["rules"]))
    print(f"  over the tail without a record: the one-temperature tail at 0.6 {1e3 * (step['sample_0.6'] - step['rules']):+.1f} us; a temperature "
          f"per row: every row greedy {1e3 * (step['rows_0'] - step['rules']):+.1f} us, every row at 0.6 "
          f"{1e3 * (step['rows_0.6'] - step['rules']):+.1f} us, half the rows at 0.6 {1e3 * (step['rows_half'] - step['rules']):+.1f} us; "
          f"spread between the repeats of the tail without a record {spread:.1f} us")
    print(f"  every row at 0.6, a temperature per row over the one-temperature tail: {1e3 * (step['rows_0.6'] - step['sample_0.6']):+.1f} us")

    # ---- schedules: transcribe(seed=3) on files of mixed lengths
    files, secs = mixed_files(args.files)
    kw = dict(language="en", sample_len=32, suppress_tokens=[-1], seed=SEED)
    log = {}

    def rounds():
        log.clear()
        log.update(windows=0, retried_rows=0, steps=0)
        inner = _model_decoder(model, dict(sample_len=32, suppress_tokens=[-1]))

        def decode_fn(windows, languages):
            res = inner(windows, languages)
            log["windows"] += len(windows)
            log["steps"] += max(len(r.tokens) for r in res)
            return res

        def fallback_fn(results, languages, **more):
            res = inner.retry(results, languages, **more)
            log["retried_rows"] += len(results)
            log["steps"] += max(len(r.tokens) for r in res)
            return res

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return wipa.transcribe(model, files, decode_fn=decode_fn, fallback_fn=fallback_fn, **kw)

    cstats = []

    def cont_files(slots):
        def run():
            cstats.clear()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return wipa.transcribe(model, files, schedule="continuous", slots=slots, check_every=ce, stats_out=cstats, **kw)
        return run

    runs = {"rounds": rounds, f"continuous_{args.files}": cont_files(args.files), "continuous_8": cont_files(8)}
    results, facts = {}, {}
    for k, fn in runs.items():  # warm-up, and what each run did
        _, results[k] = wall(fn)
        if k == "rounds":
            facts[k] = dict(windows=log["windows"], retries=log["retried_rows"], steps_upper=log["steps"])
        else:
            cs = cstats[0]
            facts[k] = dict(windows=sum(len(x) for x in cs.groups), retries=len(cs.retries), steps=cs.schedule.steps, rows=cs.rows,
                            encoder_groups=len(cs.groups), admissions=len(cs.schedule.admissions))
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(wall(fn)[0])
    same = {k: sum(x["text"] == y["text"] for x, y in zip(results[k], results["rounds"])) for k in runs if k != "rounds"}
    kept = {k: sorted({s["temperature"] for r in results[k] for s in r["segments"]}) for k in runs}
    out["schedules"] = dict(files=len(files), seconds=secs, facts=facts, wall_ms={k: sorted(v) for k, v in t.items()}, files_with_equal_text=same,
                            kept_temperatures=kept)
    print(f"# transcribe(seed={SEED}): {len(files)} files of {min(secs)} .. {max(secs)} s, sample_len 32 (median wall of {reps} calls, alternating)")
    f = facts["rounds"]
    print(f"  rounds         {f['windows']} windows, {f['retries']} retries ({f['retries'] / max(f['windows'], 1):.2f} per window); "
          f"{f['steps_upper']} generating steps (the longest row of every decode and retry call)   {median(t['rounds']):9.1f} ms wall "
          f"(min {min(t['rounds']):.1f}, max {max(t['rounds']):.1f})")
    for k in runs:
        if k == "rounds":
            continue
        f = facts[k]
        print(f"  {k:14s} {f['rows']} rows; {f['windows']} windows, {f['retries']} retries ({f['retries'] / max(f['windows'], 1):.2f} per window); "
              f"{f['steps']} steps; {f['encoder_groups']} encoder groups, {f['admissions']} admissions   {median(t[k]):9.1f} ms wall "
              f"(min {min(t[k]):.1f}, max {max(t[k]):.1f}); wall / rounds = {median(t[k]) / median(t['rounds']):.3f}; files with the text of "
              f"rounds {same[k]} / {len(files)} (bf16, margins are not gated here)")
    print(f"  temperatures of the kept segments: {kept}")
    print("  random weights: nearly every window fails the log-probability threshold at every temperature and runs the whole schedule -- the "
          "bookkeeping's worst case, not a speed claim")
    print(json.dumps({"continuous_fallback_bench": out}))


if __name__ == "__main__":
    main()
