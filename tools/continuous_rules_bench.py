#!/usr/bin/env python3
"""Continuous batching under the timestamp rules: whisper-small bf16, synthetic weights, the setting of tools/continuous_bench.py (256
clips of random features through 64 slots, clip i forced to the token count of transcript i of tests/golden/combined_test_ipa.json, EOT
suppressed in both decodes).
  decode     wipa.decode_continuous(without_timestamps=False) against four lockstep wipa.decode(without_timestamps=False) batches, each
             run to its longest row: steps and wall time after a warm-up, repeats alternating
  step       one continuous step with rules against one without and against the plain step: (a call of 72 steps - a call of 8 steps) / 64
             over 64 rows, between HIP events, as tools/continuous_bench.py measures the continuous step
  transcribe wipa.transcribe(schedule="continuous") against schedule="rounds" on a list of files of mixed lengths (synthetic audio,
             sample_len 32): decoder steps, the number and sizes of the encoder groups, wall time, and the tail of the continuous run -- the
             steps at which fewer files than slots were live
Prints a report and one JSON line.
usage: python tools/continuous_rules_bench.py [--clips 256] [--slots 64] [--repeats 3] [--files 24] [--file-slots 8]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from whisper_ipa_amd.continuous import DeviceStepper, lockstep_steps  # noqa: E402
from whisper_ipa_amd.tokenizer import get_tokenizer  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from continuous_bench import lengths  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def mixed_files(n: int, seed: int = 0):
    """n files of 4 .. 100 s of noise bursts at 16 kHz (a seeded draw): 1 .. 4 windows each"""
    rng = np.random.default_rng(seed)
    secs = rng.integers(4, 101, size=n)
    return [(0.1 * rng.standard_normal(int(s) * 16000)).astype(np.float32) for s in secs], [int(s) for s in secs]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--file-slots", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import bench
    from whisper_ipa_amd.decoding import _suppress_lists, greedy_decode_tokens, timestamp_rules
    from whisper_ipa_amd.runtime import on_stream
    from whisper_ipa_amd.transcribe import _model_decoder

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    model = bench.build_model("small")
    d = model.dims
    lens = lengths(tok, args.clips, d.n_text_ctx // 2)
    N, S, ce = len(lens), args.slots, args.check_every
    out = {"clips": N, "slots": S, "check_every": ce, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(N, d.n_audio_ctx, d.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, suppress_tokens=[-1, int(tok.eot)])

    # ---- decode: continuous with rules against four lockstep batches with rules
    def lockstep():
        res = []
        for i in range(0, N, S):
            res += wipa.decode(model, feats[i:i + S], opts, sample_len=max(lens[i:i + S]))
        return res

    stats = []

    def continuous():
        stats.clear()
        return wipa.decode_continuous(model, feats, opts, slots=S, sample_lens=lens, check_every=ce, stats_out=stats)

    _, a = wall(lockstep)  # first launches, code objects, graph capture: untimed
    _, b = wall(continuous)
    full = sum(len(r.tokens) == n for r, n in zip(b, lens))
    same = sum(r.tokens[:n] == q.tokens[:n] for r, q, n in zip(b, a, lens))
    t_lock, t_cont = [], []
    for _ in range(args.repeats):  # alternating, so that drift hits both
        t_lock.append(wall(lockstep)[0])
        t_cont.append(wall(continuous)[0])
    st = stats[0]
    lock = lockstep_steps(lens, S)
    out["decode"] = dict(lockstep_generating_steps=lock, continuous_steps=st.steps, shifts=st.shifts, lockstep_ms=sorted(t_lock),
                         continuous_ms=sorted(t_cont), rows_at_full_length=full, rows_equal_to_lockstep=same)
    ml, mc = sum(t_lock) / len(t_lock), sum(t_cont) / len(t_cont)
    print(f"# decode with timestamps: {N} clips, {S} slots, check every {ce}; whisper-small bf16 synthetic weights, {out['device']}")
    print(f"  lockstep    {lock} generating steps (+ one prompt pass and one no-speech pass per batch)   {ml:9.1f} ms wall "
          f"(min {min(t_lock):.1f}, max {max(t_lock):.1f})")
    print(f"  continuous  {st.steps} steps, shifts {st.shifts}   {mc:9.1f} ms wall (min {min(t_cont):.1f}, max {max(t_cont):.1f})")
    print(f"  steps continuous / lockstep = {st.steps / lock:.3f}; wall continuous / lockstep = {mc / ml:.3f}")
    print(f"  rows at their full length {full} / {N}; rows whose ids equal lockstep's {same} / {N} (bf16, margins are not gated here)")

    # ---- step: (72 steps - 8 steps) / 64, 64 rows
    always, first = _suppress_lists(opts, tok)
    rules = timestamp_rules(tok, opts.max_initial_timestamp)
    init3, init4 = list(tok.sot_sequence), list(tok.sot_sequence_including_notimestamps)

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def plain(n, init, r):
        return lambda: greedy_decode_tokens(model, feats[:S], init, always, first, tok.eot, max_new_tokens=n, stop_on_eot=False, rules=r)

    with on_stream() as s:
        def cont(n, init, r):
            def run():
                stp = DeviceStepper(model, S, lambda c: feats[c], lambda c: init, len(init), [200] * S, tok.eot, always, first, None, s, rules=r,
                                    no_speech_token=tok.no_speech if r is not None else None)
                stp.admit([(b, b) for b in range(S)])
                stp.run(n + len(init) - 1)
            return run

        variants = {}
        for n in (8, 72):
            variants[f"plain_{n}"] = plain(n, init4, None)
            variants[f"plain_rules_{n}"] = plain(n, init3, rules)
            variants[f"cont_{n}"] = cont(n, init4, None)
            variants[f"cont_rules_{n}"] = cont(n, init3, rules)
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(max(args.repeats, 5)):
            for k, fn in variants.items():
                times[k].append(timed(fn, s))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    step = {k: (med[f"{k}_72"] - med[f"{k}_8"]) / 64 for k in ("plain", "plain_rules", "cont", "cont_rules")}
    out["step_ms"] = step
    out["step_calls_ms"] = {k: sorted(v) for k, v in times.items()}
    print(f"# one step, 64 rows, columns 8 .. 72 (median of {max(args.repeats, 5)} calls each, HIP events)")
    for k in ("plain", "plain_rules", "cont", "cont_rules"):
        print(f"  {k:12s} {1e3 * step[k]:8.1f} us")
    print(f"  rules in lockstep {1e3 * (step['plain_rules'] - step['plain']):+.1f} us; continuous without rules over plain "
          f"{1e3 * (step['cont'] - step['plain']):+.1f} us; continuous with rules over continuous without "
          f"{1e3 * (step['cont_rules'] - step['cont']):+.1f} us")

    # ---- transcribe: both schedules on files of mixed lengths
    files, secs = mixed_files(args.files)
    FS = args.file_slots
    kw = dict(language="en", sample_len=32, suppress_tokens=[-1])
    rounds_log = []

    def rounds():
        rounds_log.clear()
        inner = _model_decoder(model, dict(sample_len=32, suppress_tokens=[-1]))

        def decode_fn(windows, languages):
            res = inner(windows, languages)
            rounds_log.append((len(windows), max(len(r.tokens) for r in res)))
            return res

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return wipa.transcribe(model, files, decode_fn=decode_fn, **kw)

    cstats = []

    def cont_files():
        cstats.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return wipa.transcribe(model, files, schedule="continuous", slots=FS, check_every=ce, stats_out=cstats, **kw)

    _, ra = wall(rounds)
    _, rb = wall(cont_files)
    t_r, t_c = [], []
    for _ in range(args.repeats):
        t_r.append(wall(rounds)[0])
        t_c.append(wall(cont_files)[0])
    cs = cstats[0]
    sched = cs.schedule
    tail_steps = ce * sum(1 for n in sched.live_rows if n < cs.rows)
    same_text = sum(x["text"] == y["text"] for x, y in zip(ra, rb))
    out["transcribe"] = dict(files=len(files), seconds=secs, slots=FS, rounds=[list(r) for r in rounds_log],
                             rounds_steps_upper=sum(m for _, m in rounds_log), continuous_steps=sched.steps,
                             continuous_groups=[len(x) for x in cs.groups], continuous_live_rows=sched.live_rows, tail_steps=tail_steps,
                             waited=cs.waited, rounds_ms=sorted(t_r), continuous_ms=sorted(t_c), files_with_equal_text=same_text)
    mr, mcc = sum(t_r) / len(t_r), sum(t_c) / len(t_c)
    print(f"# transcribe: {len(files)} files of {min(secs)} .. {max(secs)} s ({sum(-(-x // 30) for x in secs)} windows if every window is "
          f"consumed whole), sample_len 32")
    print(f"  rounds      {len(rounds_log)} rounds = encoder groups of {[n for n, _ in rounds_log]} windows in states of as many rows; longest row "
          f"per round {[m for _, m in rounds_log]} tokens ({sum(m for _, m in rounds_log)} generating steps)   {mr:9.1f} ms wall "
          f"(min {min(t_r):.1f}, max {max(t_r):.1f})")
    print(f"  continuous  {cs.rows} rows; {sched.steps} steps; {len(cs.groups)} encoder groups of {[len(x) for x in cs.groups]} windows; "
          f"{len(cs.waited)} files waited for a slot   {mcc:9.1f} ms wall (min {min(t_c):.1f}, max {max(t_c):.1f})")
    print(f"  the tail: {tail_steps} of {sched.steps} steps ran with fewer than {cs.rows} live rows (live rows per interval of {ce}: "
          f"{sched.live_rows})")
    print(f"  wall continuous / rounds = {mcc / mr:.3f}; files with equal text {same_text} / {len(files)} (bf16, margins are not gated here)")
    print(json.dumps({"continuous_rules_bench": out}))


if __name__ == "__main__":
    main()
