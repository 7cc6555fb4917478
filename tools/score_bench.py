#!/usr/bin/env python3
"""Device-side PER / PFER scoring against the host path: P seeded (reference, hypothesis) pairs over a seeded synthetic 24-feature
table (default 256 pairs, reference lengths 20-110 phones, about 15 % errors -- one transcribe_batches pass of 256 clips).
(a) the host's evaluate_batch on the first --host-pairs pairs (wall clock, SCALED to P pairs by pair count);
(b) evaluate_batch(scoring="device") end to end (wall clock around a call that ends in a stream synchronise; median and min of N
    calls after warm-up), split into: host tokenise + feature lookups + pack (wall clock), copy + kernel and kernel alone (HIP
    events on the library stream, mean of N), collect (the copy back on an idle stream + synchronise); the remainder is the
    closed-form diagnostic counts and the final divisions.
The two result dicts of the host subset are compared as tests/test_gpu_scoring.py compares them.  Writes --out.
usage: python tools/score_bench.py [--pairs 256] [--min-len 20] [--max-len 110] [--error-rate 0.15] [--phones 90] [--host-pairs 32]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
import evaluate_ipa as ev  # noqa: E402
from whisper_ipa_amd import scoring  # noqa: E402
from whisper_ipa_amd.runtime import device, on_stream  # noqa: E402

PASS_MS = 72.2  # 256 clips through transcribe_batches: log-mel -> encoder -> decode, four passes in flight (README)


class SyntheticTable:
    """seeded features in {-1, 0, +1} for ``phones``; any other phone is unknown (zero vector), as in the reference"""

    def __init__(self, phones, seed):
        rng = np.random.default_rng(seed)
        self.v = {p: rng.integers(-1, 2, ev.NUM_FEATURES).tolist() for p in phones}

    def word_to_vector_list(self, word, numeric=True):
        return [self.v[word]] if word in self.v else []


def make_pairs(rng, alphabet, n_pairs, lo, hi, error_rate):
    """references of lo..hi phones; hypotheses with error_rate of the phones substituted, deleted or followed by an insertion"""
    refs, hyps = [], []
    for _ in range(n_pairs):
        ref = rng.choice(alphabet, int(rng.integers(lo, hi + 1))).tolist()
        hyp = []
        for p in ref:
            u = rng.random()
            if u < error_rate / 3:
                continue
            hyp.append(str(rng.choice(alphabet)) if u < 2 * error_rate / 3 else p)
            if u > 1 - error_rate / 3:
                hyp.append(str(rng.choice(alphabet)))
        refs.append("".join(ref))
        hyps.append("".join(hyp))
    return refs, hyps


def wall(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def events(fn, s, iters, warmup=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    s.synchronize()
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def agree(dev, host):
    assert dev["per_scores"] == host["per_scores"] and dev["per"] == host["per"] and dev["per_std"] == host["per_std"]
    assert np.abs(np.array(dev["pfer_scores"]) - np.array(host["pfer_scores"])).max() < 1e-9
    assert abs(dev["pfer"] - host["pfer"]) < 1e-9 and abs(dev["pfer_std"] - host["pfer_std"]) < 1e-9
    for key in ("num_samples", "pfer_is_per_fallback", "pfer_unknown_phones", "pfer_base_fallback_phones"):
        assert dev[key] == host[key], key


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=110)
    ap.add_argument("--error-rate", type=float, default=0.15)
    ap.add_argument("--phones", type=int, default=90, help="phones the synthetic table knows")
    ap.add_argument("--unknown", type=int, default=4, help="further phones in the data that the table does not know")
    ap.add_argument("--host-pairs", type=int, default=32, help="pairs the host path is timed on (its time is scaled to --pairs)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    args = ap.parse_args()
    dev = device()
    rng = np.random.default_rng(args.seed)
    alphabet = np.array([chr(0x100 + i) for i in range(args.phones + args.unknown)])  # single-codepoint letters: one phone each
    ev.set_feature_table(SyntheticTable(alphabet[: args.phones].tolist(), args.seed))
    refs, hyps = make_pairs(rng, alphabet, args.pairs, args.min_len, args.max_len, args.error_rate)
    calc = ev.get_pfer_calculator()
    n_host = min(args.host_pairs, args.pairs)

    t0 = time.perf_counter()
    host = ev.evaluate_batch(refs[:n_host], hyps[:n_host])
    host_ms = (time.perf_counter() - t0) * 1e3
    host_cells = sum(len(r) * len(h) for r, h in zip(refs[:n_host], hyps[:n_host]))
    cells = sum(len(r) * len(h) for r, h in zip(refs, hyps))
    agree(ev.evaluate_batch(refs[:n_host], hyps[:n_host], scoring="device"), host)

    e2e_med, e2e_min = wall(lambda: ev.evaluate_batch(refs, hyps, scoring="device"), args.iters)
    tok = lambda: ([ev.tokenize_ipa(r) for r in refs], [ev.tokenize_ipa(h) for h in hyps])  # noqa: E731
    tok_med, _ = wall(tok, args.iters)
    ref_t, hyp_t = tok()
    pack_med, _ = wall(lambda: scoring.ScorePack(ref_t, hyp_t, calc.get_phone_features), args.iters)
    pack = scoring.ScorePack(ref_t, hyp_t, calc.get_phone_features)
    with on_stream() as s:
        buf = torch.empty(pack.nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(2, pack.P, dtype=torch.int32, device=dev)

        def copy_and_kernel():
            buf.copy_(pack.buffer, non_blocking=True)
            scoring.launch_packed(pack, buf, out, s)

        both_ms = events(copy_and_kernel, s, args.iters)
        kernel_ms = events(lambda: scoring.launch_packed(pack, buf, out, s), s, args.iters)
        s.synchronize()
        handle = scoring.ScoreHandle(pack, buf, out, s)
        collect_med, _ = wall(lambda: scoring.score_collect(handle), args.iters)
    rest = e2e_med - tok_med - pack_med - both_ms - collect_med
    scaled = host_ms * args.pairs / n_host
    row = dict(pairs=args.pairs, ref_len=[args.min_len, args.max_len], error_rate=args.error_rate, phones=args.phones, unknown=args.unknown,
               dp_cells=cells, host_pairs=n_host, host_ms=host_ms, host_us_per_cell=host_ms * 1e3 / max(host_cells, 1),
               host_ms_scaled_to_all_pairs=scaled, device_end_to_end_ms_median=e2e_med, device_end_to_end_ms_min=e2e_min,
               tokenise_ms=tok_med, lookup_pack_ms=pack_med, copy_plus_kernel_ms=both_ms, kernel_ms=kernel_ms, collect_ms=collect_med,
               counts_and_divisions_ms=rest, packed_bytes=pack.nbytes, pass_ms=PASS_MS, speedup_vs_scaled_host=scaled / e2e_med)
    lines = [
        f"# device-side PER / PFER scoring, {args.pairs} pairs, reference lengths {args.min_len}-{args.max_len}, ~{args.error_rate:.0%} errors, "
        f"{args.phones} + {args.unknown} phones, {cells} DP cells, {torch.cuda.get_device_name(dev)}",
        f"host evaluate_batch, {n_host} pairs ({host_cells} cells):   {host_ms:10.1f} ms   ({row['host_us_per_cell']:.1f} us per cell, PER + PFER)",
        f"  SCALED to {args.pairs} pairs by pair count:          {scaled:10.1f} ms",
        f"device evaluate_batch end to end, {args.pairs} pairs:  {e2e_med:10.3f} ms median, {e2e_min:.3f} ms min of {args.iters} calls",
        f"  host tokenise:                              {tok_med:10.3f} ms",
        f"  feature lookups + pack:                     {pack_med:10.3f} ms   ({pack.nbytes} bytes packed, {len(pack.vocab)} distinct phones)",
        f"  copy + kernel (HIP events):                 {both_ms:10.3f} ms   (kernel alone {kernel_ms:.3f} ms)",
        f"  collect (copy back + synchronise):          {collect_med:10.3f} ms",
        f"  diagnostic counts, divisions, means (rest): {rest:10.3f} ms",
        f"one pass of {args.pairs} clips (transcribe_batches):  {PASS_MS:10.1f} ms   -> scoring is {e2e_med / PASS_MS:.2f} of the pass it follows "
        f"({'below' if e2e_med < PASS_MS else 'ABOVE'} the target), {row['speedup_vs_scaled_host']:.0f}x the scaled host time",
        f"host subset: PER bit-equal, PFER within 1e-9, diagnostic dicts equal ({n_host} pairs)",
    ]
    text = "\n".join(lines) + "\n" + json.dumps({"score_bench": row}) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
