#!/usr/bin/env python3
"""Cost of the word-timestamp alignment of one transcribe round: whisper-small bf16, synthetic weights, B windows (default 64) of
60 text tokens and 1 500 frames each, default alignment heads (6 layers x 12 heads).  Between HIP events, after warm-up, per repeat:
  align      the whole wipa_decoder_align call (teacher-forced pass, weights launches, DTW, final projection in row blocks, token
             probabilities)
  weights    wipa_align_weights alone, once per decoder layer with alignment heads, on q / k buffers of the call's shapes
  dtw        wipa_dtw_batch alone on the matrix the call left
  pass       align - weights - dtw: the teacher-forced pass and what follows it (a remainder, not a measurement of its own)
  decode     one decode round of the same windows with timestamps and without word timestamps (``decode`` from features, 64 new
             tokens): what a transcribe round costs before the alignment; this code path is the parent commit's
By wall clock on the host: the word assembly (split_to_word_tokens + jumps + probabilities for all windows), and the float32
numpy / torch restatement of tests/alignment_ref.py (softmax chain over 72 heads + DTW) for ``--ref-windows`` windows, scaled to B.
Prints means and run-to-run spreads and one JSON line.
usage: python tools/align_bench.py [--batch 64] [--tokens 60] [--repeats 7] [--ref-windows 2]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib, timing  # noqa: E402
from whisper_ipa_amd.runtime import dt_code, on_stream, ptr, sptr  # noqa: E402


def _stats(t):
    t = sorted(t)
    return {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ref-windows", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import warnings

    from whisper_ipa_amd.tokenizer import get_tokenizer

    L = _lib.lib()
    B, n_text = args.batch, args.tokens
    model = bench.build_model("small")
    dims = model.dims
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    sot = list(tok.sot_sequence)
    rng = np.random.default_rng(0)
    # text a tokenizer can cut into words: blank + two letters, twenty words a window in the byte vocabulary
    text = [[t for _ in range(n_text // 3) for t in (220, int(rng.integers(64, 90)), int(rng.integers(64, 90)))] for _ in range(B)]
    rows = [[*sot, tok.no_timestamps, *t, tok.eot] for t in text]
    T = len(rows[0])
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(B, dims.n_audio_ctx, dims.n_text_state, generator=g).to(device=model.device, dtype=model.dtype)
    heads = model.alignment_heads
    by_layer = {}
    for l, h in heads:
        by_layer.setdefault(l, []).append(h)
    pk = model.packed(teacher_forced=True, absorbed=False)
    i32p = C.POINTER(C.c_int32)
    n_tok = np.full(B, T, dtype=np.int32)
    n_fr = np.full(B, dims.n_audio_ctx, dtype=np.int32)
    n_row = np.full(B, len(text[0]) + 1, dtype=np.int32)
    heads_arr = np.asarray(heads, dtype=np.int32).reshape(-1)
    ld_path = T + dims.n_audio_ctx
    times = {k: [] for k in ("align", "weights", "dtw", "decode")}

    def timed(fn, s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with on_stream() as s:
        dev = model.device
        d_tok = torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(dev)
        d_sizes = torch.from_numpy(np.stack([n_tok, n_fr, n_row])).to(dev)
        need = L.wipa_decoder_align_workspace_bytes(C.byref(pk["cfg"]), B, T, len(heads), 0)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        matrix = torch.empty(B, T, dims.n_audio_ctx, dtype=torch.float32, device=dev)
        path = torch.zeros(2, B, ld_path, dtype=torch.int32, device=dev)
        path_len = torch.zeros(B, dtype=torch.int32, device=dev)
        probs = torch.zeros(B, T, dtype=torch.float32, device=dev)

        def align():
            _lib.check(L.wipa_decoder_align(C.byref(pk["cfg"]), pk["dec_tab"], ptr(d_tok), ptr(feats), heads_arr.ctypes.data_as(i32p), len(heads),
                                            ptr(d_sizes[0]), ptr(d_sizes[1]), ptr(d_sizes[2]), n_tok.ctypes.data_as(i32p), n_fr.ctypes.data_as(i32p),
                                            n_row.ctypes.data_as(i32p), len(sot), tok.eot, ptr(matrix), ptr(path[0]), ptr(path[1]), ld_path,
                                            ptr(path_len), ptr(probs), 0, ptr(ws), ws.numel(), B, T, sptr(s)), "wipa_decoder_align")

        H, Ta, d = dims.n_text_head, dims.n_audio_ctx, dims.n_text_state
        q = (torch.randn(B, T, d, generator=g) * 64 ** -0.25).to(device=dev, dtype=model.dtype)
        k = (torch.randn(B, 2 * H, Ta, 64, generator=g) * 64 ** -0.25).to(device=dev, dtype=model.dtype)
        per_layer = max(len(v) for v in by_layer.values())
        st_need = L.wipa_align_weights_scratch_bytes(B, T, per_layer, Ta)
        st = torch.empty(st_need, dtype=torch.uint8, device=dev)
        acc = torch.zeros(B, T, Ta, dtype=torch.float32, device=dev)

        def weights():
            for l, hs in by_layer.items():
                hh = np.asarray(hs, dtype=np.int32)
                _lib.check(L.wipa_align_weights(ptr(q), ptr(k), 2 * H * Ta * 64, Ta * 64, dt_code(model.dtype), B, T, d, Ta, hh.ctypes.data_as(i32p),
                                                len(hh), ptr(d_sizes[0]), ptr(d_sizes[1]), ptr(st), st_need, ptr(acc), Ta, 0.0, sptr(s)),
                           "wipa_align_weights")

        tr_need = L.wipa_dtw_scratch_bytes(B, T)
        tr = torch.empty(tr_need, dtype=torch.uint8, device=dev)

        def dtw():
            _lib.check(L.wipa_dtw_batch(ptr(matrix), T * Ta, Ta, len(sot), T, ptr(d_sizes[2]), ptr(d_sizes[1]), n_row.ctypes.data_as(i32p),
                                        n_fr.ctypes.data_as(i32p), B, ptr(tr), tr_need, ptr(path[0]), ptr(path[1]), ld_path, ptr(path_len),
                                        sptr(s)), "wipa_dtw_batch")

        opts = wipa.DecodingOptions(language="en", without_timestamps=False, sample_len=64)

        def decode():
            wipa.decode(model, feats, opts)

        for fn in (align, weights, dtw, decode, align):  # first launches, code objects, graph capture: untimed
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):  # the variants alternate within a repeat so that drift hits all of them
            for name, fn in (("align", align), ("weights", weights), ("dtw", dtw), ("decode", decode)):
                times[name].append(timed(fn, s))
        align()
        path_h, len_h, probs_h = path.cpu().numpy(), path_len.cpu().numpy(), probs.cpu().numpy()
        matrix_h = matrix[: args.ref_windows].cpu().numpy()
    t0 = time.perf_counter()
    n_words = 0
    for b in range(B):
        ti, tj = path_h[0, b, :len_h[b]], path_h[1, b, :len_h[b]]
        n_words += len(timing.words_from_path(tok, text[b], ti, tj, probs_h[b, len(sot):len(sot) + len(text[b])]))
    host_ms = (time.perf_counter() - t0) * 1e3
    import alignment_ref as AR

    t0 = time.perf_counter()
    for b in range(args.ref_windows):
        qk = rng.standard_normal((len(heads), T, Ta)).astype(np.float32)
        m = AR.weights_chain(qk, Ta, np.float32)
        AR.dtw_f32(-m[len(sot):-1])
    ref_ms = (time.perf_counter() - t0) * 1e3 / max(args.ref_windows, 1) * B
    # the kernel's path is the restatement's on the kernel's own matrix
    for b in range(args.ref_windows):
        wi, wj, _, _ = AR.dtw_f32(-matrix_h[b, len(sot):len(sot) + int(n_row[b])])
        assert np.array_equal(wi, path_h[0, b, :len_h[b]]) and np.array_equal(wj, path_h[1, b, :len_h[b]]), b

    out = {"batch": B, "text_tokens": len(text[0]), "rows": T, "heads": len(heads), "repeats": args.repeats, "words": n_words}
    print(f"# word-timestamp alignment of one round, whisper-small bf16 synthetic weights, {B} windows x {len(text[0])} text tokens x "
          f"{Ta} frames, {len(heads)} alignment heads in {len(by_layer)} layers, {args.repeats} repeats, {torch.cuda.get_device_name(0)}")
    for name in ("align", "weights", "dtw", "decode"):
        out[f"{name}_ms"] = _stats(times[name])
        r = out[f"{name}_ms"]
        print(f"  {name:<8} {r['mean']:9.3f} ms   (min {r['min']:.3f}, max {r['max']:.3f})")
    out["pass_remainder_ms"] = out["align_ms"]["mean"] - out["weights_ms"]["mean"] - out["dtw_ms"]["mean"]
    out["host_words_ms"], out["restatement_f32_ms"] = host_ms, ref_ms
    print(f"  pass     {out['pass_remainder_ms']:9.3f} ms   (align - weights - dtw)")
    print(f"  host word assembly, {n_words} words: {host_ms:.2f} ms by wall clock")
    print(f"  float32 restatement on this host's CPU: {ref_ms:.0f} ms for {B} windows (from {args.ref_windows})")
    print(f"  align / decode round = {out['align_ms']['mean'] / out['decode_ms']['mean']:.3f}")
    print(json.dumps({"align_bench": out}))


if __name__ == "__main__":
    main()
