#!/usr/bin/env python3
"""What a short audio context (Whisper.audio_ctx = N: the model runs on the first N of its 1500 audio positions) buys on an MI355X:
whisper-small, synthetic weights, 64 clips, N in {None (1500), 750, 300}.  Per N, every figure next to the N = None figure of the SAME
run and next to what the size arithmetic predicts (N / 1500 for GEMM rows and cross-attention bytes, (N / 1500)^2 for the encoder's
self-attention):
  encoder      mel [64, 3000, 80] -> features, bf16: wipa_mel_pad_cast[_frames] + wipa_encoder_forward, ms per batch; and its split
               into GEMM / attention / LayerNorm time from the stage profiler (wipa_profile_begin / _end)
  step         one replayed decode step in us, absorbed (cross_splits 4 and 2) and cached: (a greedy decode of 64 new tokens - one of
               16) / 48, stop_on_eot off
  pass64       one lone pass: mel -> features -> 64 new tokens (cross_attention="auto": absorbed at this size), ms
  set_audio    wipa_decoder_set_audio alone: the copy of the features (absorbed) or the K / V projection of every layer (cached), ms
  blob         wipa_decoder_layout(...).total_bytes of the decode state, absorbed and cached
  pipelined    transcribe_batches' schedule, 4 passes (256 clips) in flight, mel -> 64 new tokens: ms per 64-clip pass, absorbed (2 frame
               splits, the several-passes setting) and cached -- the regime cross_attention="auto" was tuned in at 1500 keys
  train        the f32 fine-tune step of bench.py --mode train (32 clips x 64 target tokens, split products), uncached: encoder +
               loss_and_grads + update, ms per step, and its stages
HIP events on the library stream (host wall clock for the training step, as bench.py), one untimed warm-up of every variant, then
--repeats repeats with the three N alternating inside every repeat.
usage: python tools/audio_ctx_bench.py [--repeats 5] [--ctx 750,300] [--no-train]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import whisper_ipa_amd as wipa  # noqa: E402,F401  (before the first torch.cuda call: the package asks for its hardware queues at import)
import torch  # noqa: E402
import bench  # noqa: E402
from whisper_ipa_amd import _lib  # noqa: E402
from whisper_ipa_amd.decoding import _packed_for, _state_for, _suppress_lists, greedy_decode_tokens  # noqa: E402
from whisper_ipa_amd.runtime import on_stream, ptr, sptr  # noqa: E402

B, NEW, SHORT = 64, 64, 16
TRAIN_B, TRAIN_T = 32, 64


def _stats(t):
    t = sorted(t)
    return {"mean": sum(t) / len(t), "min": t[0], "max": t[-1]}


def timed(fn, s):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def release_states(model):
    for st in list(model.__dict__.get("_dec_states", {}).values()):
        st.release()
    model.__dict__["_dec_states"] = {}
    torch.cuda.empty_cache()


def stage_profile(model, mel):
    """GEMM / attention / LayerNorm / other ms of one encoder pass (events around every launch: slower than the untimed pass)"""
    L = _lib.lib()
    with on_stream() as s:
        _lib.check(L.wipa_profile_begin(sptr(s)), "wipa_profile_begin")
        model.embed_audio(mel)
        ms = (C.c_float * 4)()
        n = (C.c_int * 4)()
        _lib.check(L.wipa_profile_end(ms, n), "wipa_profile_end")
    return {k: round(float(ms[i]), 3) for i, k in enumerate(("gemm", "attention", "layernorm", "other"))}


def pipelined(model, mel, opts, form, passes=12, in_flight=4):
    """ms per pass with ``in_flight`` passes in flight (whisper_ipa_amd.pipeline.TranscribePipeline, as bench.py's timed region)"""
    from whisper_ipa_amd.pipeline import TranscribePipeline

    model.cross_attention = form
    kw = dict(cross_splits=2) if form == "absorbed" else {}
    with TranscribePipeline(model, opts, in_flight, max_new_tokens=NEW, stop_on_eot=False, **kw) as pipe:
        for _ in range(in_flight):
            pipe.submit(mel)
        for _ in pipe.drain():
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            pipe.submit(mel)
        for _ in pipe.drain():
            pass
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / passes
    release_states(model)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ctx", default="750,300")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: these are device measurements"
    import warnings

    from whisper_ipa_amd.tokenizer import get_tokenizer

    ctxs = [None] + [int(n) for n in args.ctx.split(",")]
    L = _lib.lib()
    model = bench.build_model("small")
    dims = model.dims
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    init = list(tok.sot_sequence_including_notimestamps)
    always, first = _suppress_lists(wipa.DecodingOptions(language="en", without_timestamps=True), tok)
    gen = torch.Generator().manual_seed(0)
    mel = (torch.randn(B, 3000, dims.n_mels, generator=gen) * 0.5).to(model.device)
    print(f"# audio_ctx: whisper-small bf16 synthetic weights, {B} clips, {NEW} new tokens, {args.repeats} repeats, {torch.cuda.get_device_name(0)}")
    forms = (("absorbed4", "absorbed", 4), ("absorbed2", "absorbed", 2), ("cached", "cached", 0))
    times = {n: {} for n in ctxs}
    extra = {n: {} for n in ctxs}

    def variants_for(n):
        model.audio_ctx = n
        model.cross_attention = "auto"
        feats = model.embed_audio(mel)
        v = {"encoder": lambda: model.embed_audio(mel)}

        def decode(form, splits, new):
            def run():
                model.cross_attention = form
                if form == "absorbed":
                    model.cross_splits = splits
                greedy_decode_tokens(model, feats, init, always, first, tok.eot, max_new_tokens=new, stop_on_eot=False)
            return run

        def set_audio(form, splits):
            def run():
                model.cross_attention = form
                if form == "absorbed":
                    model.cross_splits = splits
                pk = _packed_for(model, B, NEW)
                st = _state_for(model, B, pk)
                with on_stream() as s:
                    _lib.check(L.wipa_decoder_set_audio(C.byref(pk["cfg"]), pk["dec_tab"], ptr(feats), ptr(st.blob), st.blob.numel(), B, sptr(s)),
                               "wipa_decoder_set_audio")
                extra[n][f"blob_{form}"] = int(st.layout.total_bytes)
            return run

        for name, form, splits in forms:
            v[f"{name}_{SHORT}"] = decode(form, splits, SHORT)
            v[f"{name}_{NEW}"] = decode(form, splits, NEW)
        v["set_audio_absorbed"] = set_audio("absorbed", 4)
        v["set_audio_cached"] = set_audio("cached", 0)

        def lone_pass():
            model.cross_attention = "auto"
            model.cross_splits = 0
            greedy_decode_tokens(model, model.embed_audio(mel), init, always, first, tok.eot, max_new_tokens=NEW, stop_on_eot=False)
        v["pass64"] = lone_pass
        return v

    with on_stream() as s:
        for n in ctxs:  # warm-up: every variant once, untimed (graph capture, workspaces)
            for fn in variants_for(n).values():
                fn()
            torch.cuda.synchronize()
            model.cross_attention = "auto"
            extra[n]["encoder_stages_ms"] = stage_profile(model, mel)
            release_states(model)
        for _ in range(args.repeats):
            for n in ctxs:
                v = variants_for(n)
                for fn in v.values():  # the states and graphs of this N were dropped by the switch: not part of what is timed
                    fn()
                torch.cuda.synchronize()
                for name, fn in v.items():
                    times[n].setdefault(name, []).append(timed(fn, s))
                release_states(model)
    opts = wipa.DecodingOptions(language="en", without_timestamps=True)
    piped = {n: {"absorbed": [], "cached": []} for n in ctxs}
    for rep in range(3):
        for n in ctxs:
            model.audio_ctx = n
            for form in ("absorbed", "cached"):
                piped[n][form].append(pipelined(model, mel, opts, form))
    model.cross_attention = "auto"
    model.audio_ctx = None
    del model
    torch.cuda.empty_cache()

    train = {}
    if not args.no_train:
        from whisper_ipa_amd.training import DecoderTrainer
        from whisper_ipa_amd.whisper import Whisper

        tdims, W = bench.synthetic_weights_small(0, "small")
        tm = Whisper(tdims, dtype=torch.float32, f32_split=True)
        tm.load_weights(W)
        del W
        tr = DecoderTrainer(tm, lr=1e-5)
        tmel, ttok, eot = bench.synthetic_train_batch(TRAIN_B, TRAIN_T, tdims.n_mels)
        tmel, ttok = tmel.cuda(), ttok.cuda()
        train = {n: {"step": [], "encoder": [], "loss_and_grads": [], "update": []} for n in ctxs}
        for rep in range(args.repeats + 1):  # repeat 0 is the warm-up
            for n in ctxs:
                tm.audio_ctx = n
                tr.train_step(tmel, ttok, eot)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    tr.train_step(tmel, ttok, eot)
                torch.cuda.synchronize()
                step = (time.perf_counter() - t0) * 1e3 / 3
                stages = {}
                for name in ("encoder", "loss_and_grads", "update"):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if name == "encoder":
                        feats = tm.embed_audio(tmel)
                    elif name == "loss_and_grads":
                        tr.loss_and_grads(feats, ttok, eot)
                    else:
                        tr.apply_update()
                    torch.cuda.synchronize()
                    stages[name] = (time.perf_counter() - t1) * 1e3
                if rep:
                    train[n]["step"].append(step)
                    for k, x in stages.items():
                        train[n][k].append(x)

    out = {"clips": B, "new_tokens": NEW, "repeats": args.repeats, "ctx": []}
    base = None
    for n in ctxs:
        N = 1500 if n is None else n
        r = {"audio_ctx": n, "positions": N, "encoder_ms": _stats(times[n]["encoder"]), "pass64_ms": _stats(times[n]["pass64"]),
             "encoder_stages_ms": extra[n]["encoder_stages_ms"]}
        for name, form, _ in forms:
            r[f"step_{name}_us"] = 1e3 * (_stats(times[n][f"{name}_{NEW}"])["mean"] - _stats(times[n][f"{name}_{SHORT}"])["mean"]) / (NEW - SHORT)
        for form in ("absorbed", "cached"):
            r[f"pipelined_{form}_ms"] = _stats(piped[n][form])
            r[f"set_audio_{form}_ms"] = _stats(times[n][f"set_audio_{form}"])
            r[f"blob_{form}_bytes"] = extra[n][f"blob_{form}"]
        if train:
            for k in ("step", "encoder", "loss_and_grads", "update"):
                r[f"train_{k}_ms"] = _stats(train[n][k])
        out["ctx"].append(r)
        base = base or r
        lin, quad = N / 1500.0, (N / 1500.0) ** 2

        def line(label, now, ref, unit, predicted=None):
            ratio = now / ref
            p = "" if predicted is None else f"   size arithmetic {predicted:5.3f}"
            print(f"  {label:<34}{now:10.3f} {unit:<3} = {ratio:5.3f} of N=None ({ref:.3f} {unit}){p}")

        print(f"audio_ctx = {n} ({N} positions, {N * 0.02:.1f} s)")
        line("encoder, 64 clips", r["encoder_ms"]["mean"], base["encoder_ms"]["mean"], "ms")
        for k, pred in (("gemm", lin), ("attention", quad), ("layernorm", lin)):
            line(f"  {k} (profiled launches)", r["encoder_stages_ms"][k], base["encoder_stages_ms"][k], "ms", pred)
        for name, _, _ in forms:
            line(f"decode step, {name}", r[f"step_{name}_us"], base[f"step_{name}_us"], "us")
        line("lone pass, 64 new tokens", r["pass64_ms"]["mean"], base["pass64_ms"]["mean"], "ms")
        for form in ("absorbed", "cached"):
            line(f"pass, 4 in flight, {form}", r[f"pipelined_{form}_ms"]["mean"], base[f"pipelined_{form}_ms"]["mean"], "ms")
        for form in ("absorbed", "cached"):
            line(f"set_audio, {form}", r[f"set_audio_{form}_ms"]["mean"], base[f"set_audio_{form}_ms"]["mean"], "ms", lin)
            line(f"decode state, {form}", r[f"blob_{form}_bytes"] / 1e6, base[f"blob_{form}_bytes"] / 1e6, "MB")
        if train:
            line(f"fine-tune step, {TRAIN_B} x {TRAIN_T}, f32 split", r["train_step_ms"]["mean"], base["train_step_ms"]["mean"], "ms")
            line("  encoder", r["train_encoder_ms"]["mean"], base["train_encoder_ms"]["mean"], "ms")
            line("  loss_and_grads", r["train_loss_and_grads_ms"]["mean"], base["train_loss_and_grads_ms"]["mean"], "ms")
            line("  update", r["train_update_ms"]["mean"], base["train_update_ms"]["mean"], "ms")
            line("  feature-cache row", N * 768 * 4 / 1e6, 1500 * 768 * 4 / 1e6, "MB", lin)
    print(json.dumps({"audio_ctx_bench": out}))


if __name__ == "__main__":
    main()
