#!/usr/bin/env python3
"""Every decode path of the runtime once, on seeded inputs, with a SHA-256 per output array: what two builds of libwipa.so (and two
versions of decoding.py) must agree on bit for bit when a change only moves host code.  Models: the micro f32 model and the wide
(whisper-small width, one layer) bf16 model of tests/golden/ -- the oracle's synthetic weights behind micro_model.npz / wide_model.npz,
whose token rows feed the teacher-forced paths -- the wide one with cached and with absorbed cross-attention.  Paths:
  greedy_graph / greedy_eager   plain greedy on all three models (tokens, sum_logprobs, last-step logits)
  greedy_rules, sampled         timestamp rules; temperature 0.6 with rules
  ragged_pass / ragged_walk     per-row prompts through the batched prompt pass / walked by the step (WIPA_NO_PREFILL=1), with sot_logits
  best_of_cached / _absorbed    best_of = 2 with ranking (winners, lengths), plain and ragged
  forced                        forced_decode_logits (step logits, chosen ids)
  logits                        Whisper.logits (teacher-forced)
  align                         the alignment pass (matrix, DTW paths, token probabilities)
  beam_cached / _absorbed       beam search, beam_size 3 and patience 2, with the rules (winners, sums, lengths); micro on both
  continuous_plain              decode_continuous: five clips of unequal length through two slots, without timestamps
  continuous_rules              the same with the timestamp rules and the no-speech probabilities
  continuous_rows               the same with a temperature and an attempt per clip
  continuous_prompts            the same with a prompt per clip (two of the five without one)
and, unless --no-switches, greedy_graph again in a fresh child process under each A/B switch (the switches are read per call, the
init passes run once per process).  A torch.flip launch separates the paths in a kernel trace.
usage: python tools/decode_paths.py [--no-switches] [--only PATH]     prints "<path> <array> <sha256>" lines
       python tools/decode_paths.py --launches kernel_trace.csv       the ordered launches of a rocprofv3 --kernel-trace run of this
                                                                       driver (name, grid, workgroup, LDS) and the count per path"""
import argparse
import csv
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ["WIPA_DECODE_FUSED=0", "WIPA_DECODE_FUSED=1", "WIPA_DECODE_TAIL=0", "WIPA_LOGITS_FUSED=0", "WIPA_ABS_FUSED_PROLOGUE=0",
            "WIPA_ABS_MERGE_OUT=1"]
PATHS = ["greedy_graph", "greedy_eager", "greedy_rules", "sampled", "ragged_pass", "ragged_walk", "best_of_cached", "best_of_absorbed",
         "forced", "logits", "align", "beam_cached", "beam_absorbed", "continuous_plain", "continuous_rules", "continuous_rows",
         "continuous_prompts"]
MARKER = "flip"  # in the name of the kernel torch.flip launches; no path launches it


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    names, counts = ["(before the first path)"] + PATHS, {}
    seg = 0
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name.lower():
            seg += 1
            continue
        where = names[seg] if seg < len(names) else f"(segment {seg})"
        counts[where] = counts.get(where, 0) + 1
        print(f'{where} {name} grid={r["Grid_Size_X"]}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]} '
              f'wg={r["Workgroup_Size_X"]}x{r["Workgroup_Size_Y"]}x{r["Workgroup_Size_Z"]} lds={r.get("LDS_Block_Size", "?")}')
    for where, n in counts.items():
        print(f"# launches {where}: {n}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--no-switches", action="store_true", help="skip the child processes under the A/B switches")
    ap.add_argument("--only", choices=PATHS, help="this path alone (what the child processes run)")
    ap.add_argument("--launches", metavar="CSV", help="reduce a kernel trace of this driver instead of running")
    args = ap.parse_args()
    if args.launches:
        return launches(args.launches)

    sys.path.insert(0, ROOT)
    import whisper_ipa_amd as wipa  # before the first torch.cuda call: the package asks for its hardware queues at import
    import numpy as np
    import torch
    from oracle import whisper_ref as R
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import Beams, DecodingOptions, Sampling, forced_decode_logits, greedy_decode_tokens, ragged_decode_tokens
    from whisper_ipa_amd.timing import align_tokens
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    assert torch.cuda.is_available(), "needs a GPU"
    tag = os.environ.get("DECODE_PATHS_TAG", "")

    def sha(path, name, a):
        if torch.is_tensor(a):
            a = a.detach().float().cpu().numpy() if a.dtype == torch.bfloat16 else a.detach().cpu().numpy()
        a = np.ascontiguousarray(a)
        print(f"{tag}{path} {name} {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)

    sp = R.SpecialTokens.multilingual()
    always, first = R.suppress_lists(sp)
    init4 = list(sp.sot_sequence_including_notimestamps(0))
    init3 = init4[:3]
    rules = _lib.DecodeRules(sp.timestamp_begin, sp.no_timestamps, 50)
    golden = os.path.join(ROOT, "tests", "golden")
    tf_tokens = {"micro": np.load(os.path.join(golden, "micro_model.npz"))["tokens"],
                 "wide": np.load(os.path.join(golden, "wide_model.npz"))["small1_tokens"]}
    clips = np.stack([R.synthetic_clip(2, 30.0), R.synthetic_clip(3, 7.0)])
    mel = wipa.log_mel_spectrogram(clips, n_mels=80)
    rng = np.random.default_rng(5)
    history = [int(t) for t in rng.integers(1000, 50000, size=21)]
    rows = [[sp.sot_prev] + history + init3, list(init3)]  # a 25-token row and a bare sot_sequence: P = 32

    def build(dims, seed, dtype, cross):
        m = Whisper(ModelDimensions(**dims.__dict__), dtype=dtype, cross_attention=cross)
        m.load_weights(R.synthetic_weights(dims, seed=seed))
        return m, m.embed_audio(mel)

    micro = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
    wide = R.ModelDimensions(80, 1500, 768, 12, 1, 51865, 448, 768, 12, 1)
    models = {"micro": build(micro, 7, torch.float32, "auto"), "wide_cached": build(wide, 41, torch.bfloat16, "cached"),
              "wide_absorbed": build(wide, 41, torch.bfloat16, "absorbed")}
    for k, (_, f) in models.items():
        sha("inputs", f"features_{k}", f)

    def tokens_out(path, k, g):
        sha(path, f"{k}_tokens", g.tokens)
        sha(path, f"{k}_sum_logprobs", g.sum_logprobs)
        sha(path, f"{k}_last_logits", g.last_logits)
        for name in ("sot_logits", "winner", "lengths", "starts"):
            if getattr(g, name) is not None:
                sha(path, f"{k}_{name}", getattr(g, name))

    def greedy(path, init=init4, **kw):
        for k, (m, f) in models.items():
            tokens_out(path, k, greedy_decode_tokens(m, f, init, always, first, sp.eot, max_new_tokens=20, stop_on_eot=False, **kw))

    def sampled(path):
        for k, (m, f) in models.items():
            tokens_out(path, k, greedy_decode_tokens(m, f, init3, always, first, sp.eot, max_new_tokens=20, stop_on_eot=False, rules=rules,
                                                     sample=Sampling(11, 0.6, [(0, 0), (1, 0)])))

    def ragged(path, walk):
        if walk:
            os.environ["WIPA_NO_PREFILL"] = "1"
        try:
            for k, (m, f) in models.items():
                tokens_out(path, k, ragged_decode_tokens(m, f, rows, always, first, sp.eot, max_new_tokens=20, stop_on_eot=False, rules=rules,
                                                         sot_back=3))
        finally:
            os.environ.pop("WIPA_NO_PREFILL", None)

    def best_of(path, k):
        m, f = models[k]
        kw = dict(max_new_tokens=20, stop_on_eot=False, rules=rules, sample=Sampling(3, 0.8, [(0, 0), (1, 0)]), n_group=2, rank=True)
        tokens_out(path, k, greedy_decode_tokens(m, f, init3, always, first, sp.eot, **kw))
        tokens_out(path, k + "_ragged", ragged_decode_tokens(m, f, rows, always, first, sp.eot, sot_back=3, **kw))

    def forced(path):
        for k, (m, f) in models.items():
            hist = np.tile(np.array(init4 + history[:12], dtype=np.int64), (2, 1))
            trace, chosen = forced_decode_logits(m, f, hist, len(init4), always, first, sp.eot)
            sha(path, f"{k}_step_logits", trace)
            sha(path, f"{k}_chosen", chosen)

    def logits(path):
        for k, (m, f) in models.items():
            sha(path, f"{k}_logits", m.logits(torch.from_numpy(tf_tokens[k.split("_")[0]][:, :-1]).cuda(), f))

    def align(path):
        for k, (m, f) in models.items():
            text = [history[:14], history[14:19]]
            toks = [[*init3, sp.no_timestamps, *t, sp.eot] for t in text]
            matrix, paths, probs = align_tokens(m, toks, [len(t) + 1 for t in text], 3, sp.eot, f, [1500, 350])
            sha(path, f"{k}_matrix", matrix)
            sha(path, f"{k}_token_probs", probs)
            for b, (ti, tj) in enumerate(paths):
                sha(path, f"{k}_path{b}", np.stack([ti, tj]))

    def beam(path, wide):
        for k in ("micro", wide):
            m, f = models[k]
            tokens_out(path, k, greedy_decode_tokens(m, f, init3, always, first, sp.eot, max_new_tokens=20, stop_on_eot=False, rules=rules,
                                                     n_group=3, beams=Beams(6), length_penalty=None))

    lens5 = [9, 4, 12, 6, 8]

    def backwards(x, dim):  # torch.flip's values by a gather: the flip kernel is the marker between the paths
        return x.index_select(dim, torch.arange(x.shape[dim] - 1, -1, -1, device=x.device))

    def continuous(path, timestamps=True, **kw):
        for k, (m, f) in models.items():
            five = torch.cat([f, backwards(f, 1), backwards(f[:1], 2)]).contiguous()  # five clips from the two: frames, then channels backwards
            opts = DecodingOptions(language="en", without_timestamps=not timestamps, fp16=False, **({"seed": 5} if "temperatures" in kw else {}))
            res = decode_continuous(m, five, opts, slots=2, sample_lens=lens5, check_every=4, **kw)
            width = max(len(r.tokens) for r in res)
            sha(path, f"{k}_tokens", np.array([list(r.tokens) + [-1] * (width - len(r.tokens)) for r in res], dtype=np.int64))
            sha(path, f"{k}_lengths", np.array([len(r.tokens) for r in res], dtype=np.int64))
            sha(path, f"{k}_avg_logprob", np.array([r.avg_logprob for r in res], dtype=np.float64))
            sha(path, f"{k}_no_speech_prob", np.array([r.no_speech_prob for r in res], dtype=np.float64))

    run = {"beam_cached": lambda p: beam(p, "wide_cached"), "beam_absorbed": lambda p: beam(p, "wide_absorbed"),
           "continuous_plain": lambda p: continuous(p, timestamps=False), "continuous_rules": continuous,
           "continuous_rows": lambda p: continuous(p, temperatures=[0.0, 0.6, 0.8, 0.0, 0.6], attempts=[0, 1, 2, 0, 1]),
           "continuous_prompts": lambda p: continuous(p, prompts=[history[:9], [], history[5:21], [], history[:3]]),
           "greedy_graph": lambda p: greedy(p), "greedy_eager": lambda p: greedy(p, use_graph=False), "greedy_rules": lambda p: greedy(p, init3, rules=rules),
           "sampled": sampled, "ragged_pass": lambda p: ragged(p, False), "ragged_walk": lambda p: ragged(p, True),
           "best_of_cached": lambda p: best_of(p, "wide_cached"), "best_of_absorbed": lambda p: best_of(p, "wide_absorbed"),
           "forced": forced, "logits": logits, "align": align}
    marker = torch.arange(8, device="cuda")
    for path in ([args.only] if args.only else PATHS):
        torch.cuda.synchronize()
        torch.flip(marker, [0])
        torch.cuda.synchronize()
        run[path](path)
    torch.cuda.synchronize()
    if args.only or args.no_switches:
        return 0
    rc = 0
    for switch in SWITCHES:  # one fresh process at a time
        name, value = switch.split("=")
        env = dict(os.environ, DECODE_PATHS_TAG=switch + " ", **{name: value})
        rc |= subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "greedy_graph"], env=env).returncode
    return rc


if __name__ == "__main__":
    sys.exit(main())
