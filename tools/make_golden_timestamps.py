#!/usr/bin/env python
"""Record tests/golden/timestamp_rules.json from transformers' WhisperTimeStampLogitsProcessor -- the same algorithm as
ApplyTimestampRules of openai-whisper's decoding.py, which mlx_whisper.transcribe runs on every step (the reference's
scripts/evaluate_model.py:112-119; mlx_whisper's own port is [UPSTREAM-UNVERIFIED]).

Per case the fixture holds what regenerates the logits (an rng seed, a scale, a few boosted columns), the history (prompt +
sampled tokens), begin_index, max_initial_timestamp_index (null: no cap) and what the processor gave: the arg-max, the number of
finite columns and the log-probability of the arg-max.  tests/test_timestamps_host.py replays the cases through the numpy
restatement (tests/timestamp_ref.py).  CPU only:  python tools/make_golden_timestamps.py
"""
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "timestamp_rules.json")

V, EOT, SOT = 51865, 50257, 50258
NT = 50363          # <|notimestamps|>
TB = NT + 1         # <|0.00|>
PROMPT = [SOT, 50259, 50359]  # sot, <|en|>, <|transcribe|>

sys.path.insert(0, os.path.join(ROOT, "tests"))
from timestamp_ref import case_logits  # noqa: E402  (what the test regenerates the logits with)


def histories():
    a, b, c = 1200, 3400, 5600  # text ids
    T = TB
    return {
        "first": [],
        "one_text": [a],
        "one_timestamp": [T + 10],                       # len(seq) == 1: last and pen (pen by length)
        "two_text": [a, b],
        "text_then_timestamp": [a, T + 30],              # len(seq) == 2: a single timestamp
        "two_timestamps": [T + 0, T + 0],
        "timestamp_then_text": [T + 0, a],
        "single_after_text": [T + 0, a, b, T + 120],     # only EOT or a timestamp >= T+120 may follow
        "closed_pair": [T + 0, a, T + 120, T + 120],     # text next, later timestamps > T+120
        "text_after_pair": [T + 0, a, T + 120, T + 120, c],
        "non_monotone_forced": [T + 200, T + 200, a, T + 50, T + 50, b],  # the LAST stamp in order is T+50, not the maximum
        "non_monotone_single": [T + 200, T + 200, a, T + 50],
    }


def boosts():
    return {
        "plain": [],
        "text_peak": [[700, 14.0]],
        "timestamp_peak": [[TB + 300, 14.0]],
        "last_column": [[V - 1, 16.0]],
        "timestamp_mass": [["ts", 2.5]],                 # no single timestamp on top, the mass is
        "eot_peak": [[EOT, 14.0]],
    }


def main():
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor

    cases = []
    seed = 1000
    for (hn, seq), (bn, bo) in itertools.product(histories().items(), boosts().items()):
        for cap in ([50, None, 0] if hn == "first" else [50]):
            seed += 1
            cfg = SimpleNamespace(no_timestamps_token_id=NT, eos_token_id=EOT, bos_token_id=EOT, max_initial_timestamp_index=cap,
                                  _detect_timestamp_from_logprob=True)
            proc = WhisperTimeStampLogitsProcessor(cfg, begin_index=len(PROMPT))
            logits = case_logits(seed, 2.0, bo, V, TB)
            ids = torch.tensor([PROMPT + seq], dtype=torch.long)
            out = proc(ids, torch.from_numpy(logits)[None].clone())[0]
            lp = torch.log_softmax(out.double(), dim=-1)
            am = int(out.argmax())
            cases.append({"name": f"{hn}/{bn}/cap={cap}", "seed": seed, "scale": 2.0, "boosts": bo, "history": PROMPT + seq,
                          "begin_index": len(PROMPT), "max_initial_timestamp_index": cap,
                          "expected": {"argmax": am, "n_finite": int(torch.isfinite(out).sum()), "logprob": float(lp[am])}})
    doc = {"source": "transformers.generation.logits_process.WhisperTimeStampLogitsProcessor",
           "transformers_version": __import__("transformers").__version__,
           "vocab": {"n_vocab": V, "eot": EOT, "no_timestamps": NT, "timestamp_begin": TB}, "cases": cases}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {len(cases)} cases, {os.path.getsize(OUT)} bytes -> {OUT}")
    wins = sum(c["expected"]["argmax"] == V - 1 for c in cases)
    print(f"last column wins in {wins} cases")


if __name__ == "__main__":
    sys.exit(main())
