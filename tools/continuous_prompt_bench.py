#!/usr/bin/env python3
"""Prompts on the continuous schedule: whisper-small bf16, synthetic weights, the setting of tools/continuous_rules_bench.py and
tools/prompt_bench.py.  HIP events on the library stream, after warm-up, the variants alternating within every repeat.
  step        one continuous step with rules over 64 rows: (a call of 72 steps - a call of 8 steps) / 64, median of the repeats --
                rules           a continuous call with rules, columns 8 .. 72 (the unprompted step, unchanged kernels)
                prompted_empty  the same call with wipa_decode_call.prompted on the same columns: prompt room 0, no row has a prompt -- the
                                PROMPTED tail against the CONTINUOUS one and nothing else
                prompted_197    the same prompted call, every row behind a 197-column prompt (prompt room 197): the steps stand at columns
                                205 .. 269 and every row's self-attention sees 197 more keys -- what a conditioned row pays per step
  admission   one wipa_decoder_admit_rows_prompted call (cross-attention input + tokens + the prompt pass + the K / V scatter) for 1, 4
              and 16 rows x W = 32 and 197 prompt columns, against wipa_decoder_admit_rows of the same rows; the difference is the pass.
              For scale: the W - 1 steps that walking the prompt column by column would take, at the measured step
  schedules   wipa.transcribe(condition_on_previous_text=True) on the 24 files of tools/continuous_rules_bench.py (sample_len 32):
              schedule="rounds" against schedule="continuous" with 24 and with 8 slots -- wall time, decoder steps, admissions
whisper-small bf16 runs the ABSORBED cross form, where an admission copies the clip's features.  In the cached form an admission projects
every layer's cross K / V into the state AND the prompt pass projects them again into its workspace: not measured here.
Not measured here either: a pretrained checkpoint (random weights never say EOT early, so every window runs to sample_len and a window's
history is as long as it can be), and more than one GPU.  Prints a report and one JSON line.
usage: python tools/continuous_prompt_bench.py [--repeats 5] [--files 24]"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from whisper_ipa_amd.continuous import DeviceStepper  # noqa: E402
from whisper_ipa_amd.tokenizer import get_tokenizer  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from continuous_rules_bench import mixed_files, wall  # noqa: E402


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

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    model = bench.build_model("small")
    d = model.dims
    S, ce, reps = args.slots, args.check_every, max(args.repeats, 3)
    out = {"slots": S, "check_every": ce, "repeats": reps, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(S, d.n_audio_ctx, d.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, suppress_tokens=[-1, int(tok.eot)])
    always, first = _suppress_lists(opts, tok)
    rules = timestamp_rules(tok, opts.max_initial_timestamp)
    init = list(tok.sot_sequence)
    tb = int(tok.timestamp_begin)
    rng = np.random.default_rng(0)

    def history(n):
        body = [int(t) for t in rng.integers(1000, 50000, size=n)]
        for j in range(3, n, 9):
            body[j] = tb + 5 * j
        return body

    def prompt(W):  # W prompt columns: sot_prev and W - 1 history tokens
        return ([int(tok.sot_prev)] + history(W - 1)) if W else []

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stepper(s, room, prompts):
        return DeviceStepper(model, S, lambda c: feats[c], lambda c: init, len(init), [200] * S, tok.eot, always, first, None, s, rules=rules,
                             no_speech_token=tok.no_speech, prompts=(lambda c: prompts[c]) if room is not None else None, prompt_room=room)

    with on_stream() as s:
        # ---- step: (72 steps - 8 steps) / 64, 64 rows, with rules
        p197 = [prompt(197) for _ in range(S)]
        kinds = {"rules": (None, None), "prompted_empty": (0, [[]] * S), "prompted_197": (197, p197)}

        def cont(n, room, prompts):
            def run():
                stp = stepper(s, room, prompts)
                stp.admit([(b, b) for b in range(S)])
                stp.run(n + len(init) - 1)
                stp._keep.clear()
            return run

        variants = {f"{k}_{n}": cont(n, *kinds[k]) for n in (8, 72) for k in kinds}
        for fn in variants.values():  # first launches, code objects, graph capture: untimed
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, s))
        per_repeat = {k: [(b - a) / 64 for a, b in zip(times[f"{k}_8"], times[f"{k}_72"])] for k in kinds}
        step = {k: (median(times[f"{k}_72"]) - median(times[f"{k}_8"])) / 64 for k in kinds}
        out["step_ms"], out["step_ms_per_repeat"] = step, per_repeat
        print(f"# one continuous step with rules, {S} rows (median of {reps} calls each, HIP events); whisper-small bf16 synthetic weights, "
              f"{out['device']}")
        for k in kinds:
            v = per_repeat[k]
            print(f"  {k:15s} {1e3 * step[k]:8.1f} us   (per repeat: min {1e3 * min(v):.1f}, max {1e3 * max(v):.1f})")
        spread = 1e3 * (max(per_repeat["rules"]) - min(per_repeat["rules"]))
        print(f"  the PROMPTED tail over the CONTINUOUS tail, same columns: {1e3 * (step['prompted_empty'] - step['rules']):+.1f} us per step; "
              f"behind 197 prompt columns: {1e3 * (step['prompted_197'] - step['rules']):+.1f} us per step; spread between the repeats of "
              f"the unprompted step {spread:.1f} us")

        # ---- admission: n rows x W prompt columns, against the unprompted admission of the same rows
        adm = {}
        cases = [(n, W) for n in (1, 4, 16) for W in (0, 32, 197)]
        steppers = {}
        for n, W in cases:
            prompts = [prompt(W) for _ in range(S)]
            steppers[(n, W)] = stepper(s, W if W else None, prompts)  # W = 0: wipa_decoder_admit_rows
        # the steppers of one model, stream and slot count share ONE decode state: open it once more at the widest prompt, so that every
        # case admits at column 197 -- over and over, without steps in between, which is all an admission's cost depends on
        steppers[(16, 197)]._begin()

        def admission(n, W):
            stp = steppers[(n, W)]

            def run():
                stp.admit([(b, b) for b in range(n)])
                del stp._keep[:]  # the workspace goes back to the allocator of this stream: reused in stream order
            return run

        runs = {c: admission(*c) for c in cases}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        t_adm = {c: [] for c in cases}
        for _ in range(reps):
            for c, fn in runs.items():
                t_adm[c].append(timed(fn, s))
        print(f"# one admission call (median of {reps}, HIP events): rows x prompt columns W; W = 0 is wipa_decoder_admit_rows")
        for n in (1, 4, 16):
            base = median(t_adm[(n, 0)])
            for W in (32, 197):
                m = median(t_adm[(n, W)])
                adm[f"{n}x{W}"] = dict(ms=m, plain_ms=base, pass_ms=m - base, min=min(t_adm[(n, W)]), max=max(t_adm[(n, W)]),
                                       walked_ms=(W - 1) * step["rules"])
                print(f"  {n:2d} rows x W = {W:3d}: {m:8.3f} ms (min {min(t_adm[(n, W)]):.3f}, max {max(t_adm[(n, W)]):.3f}); without prompts "
                      f"{base:.3f} ms; the pass {m - base:+.3f} ms = {(m - base) / step['rules']:.1f} steps of {S} rows; walking W - 1 columns "
                      f"would take {(W - 1) * step['rules']:.1f} ms")
        out["admission"] = adm

    # ---- schedules: transcribe(condition_on_previous_text=True) on files of mixed lengths
    files, secs = mixed_files(args.files)
    kw = dict(language="en", sample_len=32, suppress_tokens=[-1], condition_on_previous_text=True)
    cstats = []

    def rounds():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return wipa.transcribe(model, files, **kw)

    def cont_files(slots):
        def run():
            cstats.clear()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return wipa.transcribe(model, files, schedule="continuous", slots=slots, check_every=ce, stats_out=cstats, **kw)
        return run

    def plain_files(slots):  # the same files without conditioning: what the prompts add to the continuous schedule
        def run():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return wipa.transcribe(model, files, schedule="continuous", slots=slots, check_every=ce, language="en", sample_len=32,
                                       suppress_tokens=[-1])
        return run

    runs = {"rounds": rounds, f"continuous_{args.files}": cont_files(args.files), "continuous_8": cont_files(8),
            f"unconditioned_{args.files}": plain_files(args.files), "unconditioned_8": plain_files(8)}
    results, facts = {}, {}
    for k, fn in runs.items():  # warm-up, and what each run did
        _, results[k] = wall(fn)
        if k.startswith("continuous"):
            cs = cstats[0]
            facts[k] = dict(rows=cs.rows, windows=sum(len(x) for x in cs.groups), steps=cs.schedule.steps, admissions=len(cs.schedule.groups),
                            shifts=len(cs.schedule.shifts), prompt_budget=cs.prompt_budget,
                            prompted_windows=sum(1 for _, _, _, kept in cs.prompts if kept), longest_prompt=max(kept for _, _, _, kept in cs.prompts))
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(wall(fn)[0])
    same = {k: sum(x["text"] == y["text"] for x, y in zip(results[k], results["rounds"])) for k in runs if k.startswith("continuous")}
    out["schedules"] = dict(files=len(files), seconds=secs, facts=facts, wall_ms={k: sorted(v) for k, v in t.items()}, files_with_equal_text=same)
    print(f"# transcribe(condition_on_previous_text=True): {len(files)} files of {min(secs)} .. {max(secs)} s, sample_len 32 (median wall of "
          f"{reps} calls, alternating)")
    print(f"  rounds            {median(t['rounds']):9.1f} ms wall (min {min(t['rounds']):.1f}, max {max(t['rounds']):.1f})")
    for k in runs:
        if k == "rounds":
            continue
        line = f"  {k:17s} {median(t[k]):9.1f} ms wall (min {min(t[k]):.1f}, max {max(t[k]):.1f}); wall / rounds = {median(t[k]) / median(t['rounds']):.3f}"
        if k in facts:
            f = facts[k]
            line += (f"; {f['rows']} rows, {f['windows']} windows ({f['prompted_windows']} with a prompt, the longest {f['longest_prompt']} tokens, "
                     f"budget {f['prompt_budget']}), {f['steps']} steps, {f['admissions']} admission calls, {f['shifts']} shifts; files with the "
                     f"text of rounds {same[k]} / {len(files)} (bf16, margins are not gated here)")
        print(line)
    print(json.dumps({"continuous_prompt_bench": out}))


if __name__ == "__main__":
    main()
