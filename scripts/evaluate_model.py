"""Offline evaluation with the behaviour of the reference's scripts/evaluate_model.py: transcribe a
test JSON (``audio_path`` / ``ipa_transcription`` records) with the base model and with a fine-tuned
checkpoint, print the first three examples, PER / PFER (mean ± std), the comparison table and the
target thresholds (reference :127-268), same CLI flags (:272-308).

Differences that the hardware asks for:
  * clips are decoded in batches of ``--batch-size`` (the reference is batch 1, :181-212), ``--passes-in-flight`` batches
    at a time on one GPU (whisper_ipa_amd.pipeline.transcribe_batches -- the schedule bench.py times); the result per clip is
    the same because every kernel on the path is batch-invariant and passes share no state
    (tests/test_gpu_model.py::test_full_size_bench_workload_properties, ::test_transcribe_batches_*);
  * under ``torchrun`` every rank takes a contiguous slice of the test list with a full weight
    replica and no collective on the data path; the hypotheses are gathered once at the end;
  * PER / PFER of the whole list are scored in one GPU launch (``--scoring device``, whisper_ipa_amd.scoring; ``host`` keeps the
    reference's Python loops): the same integers, so the same PER and, to float64 rounding, the same PFER;
  * the base model is a local directory (no hub access).  The reference's base leg goes through
    ``mlx_whisper.transcribe(audio_path, path_or_hf_repo=..., language=..., word_timestamps=False)`` (:112-119), which is NOT the
    checkpoint leg's ``decode(language="en", without_timestamps=True)``: it decodes with timestamps on (a three-token prompt),
    applies the timestamp rules on every step, cuts segments, skips silent windows and walks files longer than 30 s window by
    window.  ``--base-decode transcribe`` sends the base leg through ``whisper_ipa_amd.transcribe``, which does all of that
    (without conditioning on previous text unless ``--condition-on-previous-text`` asks for upstream's default, ``--initial-prompt``
    for a prompt before every file's first window; see that module for what it refuses); ``--base-decode decode``, the
    default, keeps the base leg on the checkpoint leg's path as before, which gives a different token stream than the
    reference's base leg.
All compute runs in libwipa.so on the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evaluate_ipa import SCORING_MODES, evaluate_batch  # noqa: E402
from whisper_ipa_amd import parallel  # noqa: E402
from whisper_ipa_amd.audio import PcmBatch, count_longer_than_audio_ctx, load_audio, pad_or_trim, read_pcm  # noqa: E402
from whisper_ipa_amd.decoding import DecodingOptions  # noqa: E402
from whisper_ipa_amd.load_models import load_model, overlay_decoder_weights, resolve_audio_ctx  # noqa: E402
from whisper_ipa_amd.pipeline import transcribe_batches  # noqa: E402


def load_checkpoint_model(checkpoint_path: str, base_model: str = "mlx-community/whisper-small-mlx", audio_ctx: Optional[int] = None):
    """reference :20-79: base architecture in fp32 + the checkpoint's ``decoder.*`` tensors.  ``audio_ctx``: --audio-ctx; without
    one the value the checkpoint's training_config.json recorded is used, and a different one is used with a warning."""
    print(f"Loading base model architecture: {base_model}")
    audio_ctx, warning = resolve_audio_ctx(audio_ctx, checkpoint_path)
    if warning:
        print(warning)
    model = load_model(base_model, audio_ctx=audio_ctx)
    model.set_dtype(torch.float32)
    if checkpoint_path and os.path.exists(os.path.join(checkpoint_path, "adapter_config.json")):
        # a LoRA run's checkpoint (or --adapter DIR): adapter files instead of a decoder overlay, merged into the base weights
        from whisper_ipa_amd.lora import load_adapter

        tensors, lora_cfg, _ = load_adapter(checkpoint_path)
        model.set_adapter(tensors, lora_cfg)
        print(f"✓ LoRA adapter applied: rank {lora_cfg.rank}, alpha {lora_cfg.alpha:g}, targets {','.join(lora_cfg.targets)} ({len(tensors)} tensors)")
        return model
    try:
        n = overlay_decoder_weights(model, checkpoint_path)
    except FileNotFoundError:
        print(f"WARNING: No weights found at {checkpoint_path}, using base model")
        return model
    print(f"Found {n} decoder parameters to load")
    print("✓ Decoder weights loaded successfully")
    return model


def parse_adapter_bank(spec: str) -> Dict[str, str]:
    """``--adapter-bank lang=DIR[,lang=DIR...]`` -> {language: adapter directory}, in the order given (the order of the bank's ids)"""
    out: Dict[str, str] = {}
    for part in [p for p in spec.split(",") if p.strip()]:
        lang, sep, directory = part.partition("=")
        if not sep or not lang.strip() or not directory.strip():
            raise ValueError(f"--adapter-bank: {part!r} is not lang=DIR")
        if lang.strip() in out:
            raise ValueError(f"--adapter-bank: language {lang.strip()!r} is given twice")
        out[lang.strip()] = directory.strip()
    if not out:
        raise ValueError("--adapter-bank: no lang=DIR pair")
    return out


def sample_adapters(samples: List[Dict], languages) -> List[Optional[str]]:
    """every sample's adapter: its language field (``locale``, else ``language``) where the bank holds that language, else None (the base)"""
    names = set(languages)
    return [(s.get("locale") or s.get("language")) if (s.get("locale") or s.get("language")) in names else None for s in samples]


def set_adapter_bank_from(model, bank_dirs: Dict[str, str]):
    """load the adapters of ``bank_dirs`` and keep them beside the base weights, unmerged (Whisper.set_adapter_bank)"""
    from whisper_ipa_amd.lora import AdapterBank, load_adapter

    loaded = {lang: load_adapter(directory)[:2] for lang, directory in bank_dirs.items()}
    model.set_adapter_bank(AdapterBank(model.dims, loaded))
    print(f"✓ adapter bank: {len(loaded)} adapters ({', '.join(loaded)}), rank {model.adapter_bank.rank}, sites {', '.join(model.adapter_bank.sites)}")
    return model


INGEST_MODES = ("device", "host")


def load_clips(audio_paths: List[str], ingest: str = "device", audio_ctx: Optional[int] = None):
    """host side of reference :184-189 for a list of clips: (batch or None, positions of the readable clips); a clip that cannot
    be read is reported and yields "" (:202-204).  ``ingest="device"``: the batch is a ``PcmBatch`` -- the files' PCM bytes packed
    for one copy; conversion, resampling and the 30 s pad run on the GPU (whisper_ipa_amd.audio.load_audio_batch).
    ``ingest="host"``: audio [n_ok, 480000] f32 from ``pad_or_trim(load_audio(path))`` in numpy, as before.
    ``audio_ctx`` (the model's): the clips longer than audio_ctx * 20 ms are counted and reported on one warning line."""
    if ingest not in INGEST_MODES:
        raise ValueError(f"ingest must be one of {INGEST_MODES}, got {ingest!r}")
    clips, slots, over = [], [], 0
    for i, path in enumerate(audio_paths):
        try:
            if ingest == "device":
                clips.append(read_pcm(path))
            else:
                a = load_audio(path)
                over += count_longer_than_audio_ctx([len(a)], audio_ctx)
                clips.append(np.asarray(pad_or_trim(a), dtype=np.float32))
            slots.append(i)
        except Exception as e:
            print(f"\nError transcribing {path}: {e}")
    if not clips:
        return None, slots
    batch = PcmBatch(clips) if ingest == "device" else torch.from_numpy(np.stack(clips))
    if ingest == "device":
        over = count_longer_than_audio_ctx(batch.sample_counts(), audio_ctx)
    if over:
        print(f"\nWARNING: {over} of {len(clips)} clips are longer than audio_ctx {audio_ctx} ({audio_ctx * 0.02:.2f} s) and are cut")
    return batch, slots


def transcribe_clips(model, audio_paths: List[str], options: DecodingOptions, batch_size: int = 64,
                     passes_in_flight: int = 4, progress=None, ingest: str = "device") -> List[str]:
    """reference :181-212 for the whole list: ``batch_size`` clips per batch, ``passes_in_flight`` batches in flight on one GPU
    (whisper_ipa_amd.pipeline.transcribe_batches: (ingest ->) log-mel -> encoder -> greedy decode per batch on its own stream
    set, the files of the next batches read on a helper thread meanwhile).  One text per path, "" where the file could not be
    read.  ``ingest``: where the samples are converted and resampled (``load_clips``); 16 kHz files give the same bits either way."""
    texts = [""] * len(audio_paths)
    metas = []  # (first clip of the batch, positions of its readable clips), in submission order

    def batches():
        for b in range(0, len(audio_paths), batch_size):
            audio, slots = load_clips(audio_paths[b:b + batch_size], ingest, audio_ctx=getattr(model, "audio_ctx", None))
            if audio is None:
                continue
            metas.append((b, slots))
            yield audio

    for r in transcribe_batches(model, batches(), options, passes_in_flight=passes_in_flight, prefetch=passes_in_flight):
        b, slots = metas[r.index]
        for i, text in zip(slots, r.texts):
            texts[b + i] = text.strip()
        if progress is not None:
            progress(min(b + batch_size, len(audio_paths)))
    return texts


DECODE_MODES = ("lockstep", "continuous")


def transcribe_clips_continuous(model, audio_paths: List[str], options: DecodingOptions, slots: int = 64, progress=None,
                                ingest: str = "device", row_adapters: Optional[List[Optional[str]]] = None) -> List[str]:
    """``transcribe_clips`` through whisper_ipa_amd.decode_continuous: the clips' log-mels, ``slots`` files at a time, then ONE
    continuous decode of all of them -- ``slots`` rows, and a row whose clip has reached EOT takes the next pending clip (the encoder runs
    in chunks of ``slots`` clips ahead of need).  One text per path, "" where the file could not be read."""
    from whisper_ipa_amd import decode_continuous
    from whisper_ipa_amd.audio import load_audio_batch, log_mel_spectrogram

    texts = [""] * len(audio_paths)
    mels, where = [], []
    for b in range(0, len(audio_paths), slots):
        audio, ok = load_clips(audio_paths[b:b + slots], ingest, audio_ctx=getattr(model, "audio_ctx", None))
        if audio is None:
            continue
        audio = load_audio_batch(audio) if ingest == "device" else audio.to(model.device)
        mels.append(log_mel_spectrogram(audio, n_mels=model.dims.n_mels))
        where += [b + i for i in ok]
        if progress is not None:
            progress(min(b + slots, len(audio_paths)))
    if mels:
        adapters = {"row_adapters": [row_adapters[i] for i in where]} if row_adapters is not None else {}  # per clip that could be read
        for i, r in zip(where, decode_continuous(model, torch.cat(mels), options, slots=slots, **adapters)):
            texts[i] = r.text.strip()
    return texts


BASE_DECODE_MODES = ("decode", "transcribe")


def transcribe_files(model, audio_paths: List[str], batch_size: int = 64, progress=None, seed: Optional[int] = None,
                     condition_on_previous_text: bool = False, initial_prompt: Optional[str] = None, schedule: str = "rounds",
                     beams: Optional[dict] = None) -> List[str]:
    """reference :112-119 for the whole list: ``mlx_whisper.transcribe(path, language="en", word_timestamps=False)["text"]`` per
    file through whisper_ipa_amd.transcribe, ``batch_size`` files per call (their windows decode as one batch per round).  One
    text per path, "" where the file could not be read.  ``seed``: run mlx_whisper.transcribe's temperature schedule on the windows
    that fail its thresholds (None: temperature 0 only, such windows are flagged).  ``condition_on_previous_text`` / ``initial_prompt``:
    mlx_whisper.transcribe's options of those names (upstream defaults to conditioning on; here it is opt-in).
    ``schedule="continuous"``: transcribe(schedule="continuous", slots=batch_size) -- the windows go through ``batch_size`` rows of one
    decode state with refill, 8 x ``batch_size`` files per call (what bounds a call is the host memory of its samples, not its rows);
    it serves ``seed`` (a retried window is admitted again with a temperature of its own) and ``condition_on_previous_text`` /
    ``initial_prompt`` (a window is admitted with its file's prompt in front of its admission column; with the default sample_len the
    prompt keeps the last 196 history tokens, not upstream's 223 -- transcribe's ``prompt_budget``), and refuses the rest by name.
    ``beams``: ``beam_size`` / ``patience`` / ``length_penalty`` for transcribe (rounds schedule: every window's temperature-0 decode is a
    beam search)."""
    from whisper_ipa_amd import transcribe

    texts = [""] * len(audio_paths)
    more = {"schedule": "continuous", "slots": batch_size} if schedule == "continuous" else {}
    per_call = 8 * batch_size if schedule == "continuous" else batch_size
    for b in range(0, len(audio_paths), per_call):
        clips, slots = [], []
        for i, path in enumerate(audio_paths[b:b + per_call]):
            try:
                clips.append(np.asarray(load_audio(path), dtype=np.float32))
                slots.append(b + i)
            except Exception as e:
                print(f"\nError transcribing {path}: {e}")
        if clips:
            for i, r in zip(slots, transcribe(model, clips, language="en", word_timestamps=False, seed=seed,
                                              condition_on_previous_text=condition_on_previous_text, initial_prompt=initial_prompt, **more,
                                              **(beams or {}))):
                texts[i] = r["text"].strip()
        if progress is not None:
            progress(min(b + per_call, len(audio_paths)))
    return texts


def transcribe_batch(model, audio_paths: List[str], n_mels: int, options: DecodingOptions) -> List[str]:
    """ONE batch with nothing else in flight (round 4's entry point, kept for callers that hold a single batch)"""
    assert n_mels == model.dims.n_mels
    return transcribe_clips(model, audio_paths, options, batch_size=max(1, len(audio_paths)), passes_in_flight=1)


def evaluate_model(model_path: str, test_data_path: str, num_samples: Optional[int] = None, model_name: str = "Model",
                   is_checkpoint: bool = False, n_mels: int = 80, base_model: str = "mlx-community/whisper-small-mlx",
                   batch_size: int = 64, passes_in_flight: int = 4, ingest: str = "device", scoring: str = "device",
                   base_decode: str = "decode", seed: Optional[int] = None, condition_on_previous_text: bool = False,
                   initial_prompt: Optional[str] = None, decode: str = "lockstep", beams: Optional[dict] = None,
                   audio_ctx: Optional[int] = None, adapter_bank: Optional[Dict[str, str]] = None) -> Dict:
    """``adapter_bank`` ({language: adapter directory}): the base model with those adapters unmerged, every sample decoded under the
    adapter of its language field in ONE mixed continuous decode (samples without a match on the base)"""
    if decode not in DECODE_MODES:
        raise ValueError(f"decode must be one of {DECODE_MODES}, got {decode!r}")
    rank, world_size = parallel.world()
    say = print if rank == 0 else (lambda *a, **k: None)
    say("=" * 70)
    say(f"Evaluating {model_name}")
    say("=" * 70)
    say(f"\nLoading test data: {test_data_path}")
    with open(test_data_path) as f:
        test_data = json.load(f)
    if num_samples:
        test_data = test_data[:num_samples]
        say(f"Evaluating on {num_samples} samples")
    else:
        say(f"Evaluating on all {len(test_data)} samples")
    say(f"\nModel: {model_path}")
    if adapter_bank is not None:
        model = load_model(base_model, audio_ctx=audio_ctx)  # the base architecture in fp32, as the checkpoint leg loads it
        model.set_dtype(torch.float32)
        set_adapter_bank_from(model, adapter_bank)
    elif is_checkpoint:
        say("\nLoading checkpoint...")
        model = load_checkpoint_model(model_path, base_model=base_model, audio_ctx=audio_ctx)
    else:
        model = load_model(model_path, audio_ctx=audio_ctx)
        model.set_dtype(torch.float32)
    if model.audio_ctx is not None:
        say(f"audio_ctx {model.audio_ctx}: the model runs on {model.audio_ctx * 0.02:.2f} s of context")
        if base_decode == "transcribe" and not is_checkpoint:
            raise SystemExit("--base-decode transcribe is not implemented with --audio-ctx (transcribe() assumes 30 s windows)")
    if model.dims.n_mels != n_mels:
        say(f"NOTE: --n-mels {n_mels} does not match the model ({model.dims.n_mels}); using the model's")
        n_mels = model.dims.n_mels
    options = DecodingOptions(language="en", without_timestamps=True)

    lo, hi = parallel.shard_bounds(len(test_data), world_size, rank)
    mine = test_data[lo:hi]
    say("\nTranscribing test samples...")
    if base_decode == "transcribe" and not is_checkpoint:
        local_hyp = transcribe_files(model, [s["audio_path"] for s in mine], batch_size=batch_size, seed=seed,
                                     condition_on_previous_text=condition_on_previous_text, initial_prompt=initial_prompt,
                                     schedule="continuous" if decode == "continuous" else "rounds", beams=beams,
                                     progress=lambda n: say(f"  {n}/{len(mine)} clips on rank 0", flush=True))
    elif adapter_bank is not None:  # per-row adapters ride the continuous decode: one mixed-language stream through all slots
        picked = sample_adapters(mine, adapter_bank)
        say(f"  adapters: {sum(p is not None for p in picked)} of {len(mine)} samples match a language of the bank, the rest decode on the base")
        local_hyp = transcribe_clips_continuous(model, [s["audio_path"] for s in mine], options, slots=batch_size, ingest=ingest,
                                                row_adapters=picked,
                                                progress=lambda n: say(f"  {n}/{len(mine)} clips read on rank 0", flush=True))
    elif decode == "continuous":
        local_hyp = transcribe_clips_continuous(model, [s["audio_path"] for s in mine], options, slots=batch_size, ingest=ingest,
                                                progress=lambda n: say(f"  {n}/{len(mine)} clips read on rank 0", flush=True))
    else:
        local_hyp = transcribe_clips(model, [s["audio_path"] for s in mine], options, batch_size=batch_size,
                                     passes_in_flight=passes_in_flight, ingest=ingest,
                                     progress=lambda n: say(f"  {n}/{len(mine)} clips on rank 0", flush=True))
    hypotheses = local_hyp
    if world_size > 1:
        import torch.distributed as dist

        parts: List = [None] * world_size
        dist.all_gather_object(parts, local_hyp)
        hypotheses = [h for part in parts for h in part]
    references = [s["ipa_transcription"] for s in test_data]

    # per-sample scores included (reference evaluate_ipa.py:370-378); scoring="device": every pair's edit distances in one launch
    results = evaluate_batch(references, hypotheses, scoring=scoring)
    for i in range(min(3, len(references))):
        say(f"\nSample {i + 1}:")
        say(f"  Reference:  {references[i]}")
        say(f"  Hypothesis: {hypotheses[i]}")
        say(f"  PER:  {results['per_scores'][i]:.2f}%")
        say(f"  PFER: {results['pfer_scores'][i]:.2f}%" + ("  (PER: no feature table)" if results["pfer_is_per_fallback"] else ""))
    say("\n" + "=" * 70)
    say(f"{model_name} - Overall Results")
    say("=" * 70)
    say(f"\nPER (Phone Error Rate):         {results['per']:.2f}% (±{results['per_std']:.2f}%)")
    say(f"PFER (Phone Feature Error Rate): {results['pfer']:.2f}% (±{results['pfer_std']:.2f}%)")
    say(f"Number of samples: {results['num_samples']}")
    return results


def compare_models(base_results: Dict, trained_results: Dict) -> None:
    """reference :235-268."""
    print("\n" + "=" * 70)
    print("Model Comparison")
    print("=" * 70)
    print(f"\n{'Metric':<30} {'Base Model':<15} {'Trained Model':<15} {'Improvement':<15}")
    print("-" * 70)
    for label, key in (("PER (Phone Error Rate)", "per"), ("PFER (Feature Error Rate)", "pfer")):
        diff = base_results[key] - trained_results[key]
        print(f"{label:<30} {base_results[key]:>6.2f}%{'':<8} {trained_results[key]:>6.2f}%{'':<8} {diff:>+6.2f}%")
    print("\n" + "=" * 70)
    print("Benchmark Comparison (from paper)")
    print("=" * 70)
    print("Target scores (zero-shot, unseen languages):")
    print("  - Best in paper (1k samples): 21.2% PFER")
    print("  - Wav2Vec2Phoneme: 22.4% PFER")
    print("  - Human IAA: 19.6% PFER")
    print("\nTarget scores (supervised, trained languages):")
    print("  - Overall: 5.7% PFER")
    print("  - Polish (best): 2.5% PFER")
    pfer = trained_results["pfer"]
    if pfer < 50:
        print("\n✅ MINIMUM VIABLE: PFER < 50% achieved!")
    if pfer < 30:
        print("✅ GOOD: PFER < 30% achieved!")
    if pfer < 25:
        print("✅ EXCELLENT: PFER < 25% achieved!")
    if pfer < 21.2:
        print("🎉 SOTA: Beat paper's best zero-shot result!")


def main(argv=None) -> Dict:
    ap = argparse.ArgumentParser(description="Evaluate Whisper-IPA model")
    ap.add_argument("--checkpoint", type=str, default="checkpoints/whisper-ipa-english/checkpoint-250",
                    help="Path to trained model checkpoint")
    ap.add_argument("--base-model", type=str, default="mlx-community/whisper-small-mlx",
                    help="Base model: local directory with config.json + weights.safetensors")
    ap.add_argument("--test-data", type=str, default="data/processed/english_only_test_ipa.json", help="Path to test data JSON")
    ap.add_argument("--num-samples", type=int, default=100, help="Number of samples to evaluate (default: 100, use 0 for all)")
    ap.add_argument("--skip-base", action="store_true", help="Skip base model evaluation (only evaluate checkpoint)")
    ap.add_argument("--n-mels", type=int, default=128, help="Number of mel bins (80 for small/medium, 128 for large)")
    ap.add_argument("--batch-size", type=int, default=64, help="clips decoded together per GPU")
    ap.add_argument("--passes-in-flight", type=int, default=4,
                    help="batches kept in flight on one GPU (whisper_ipa_amd.pipeline.transcribe_batches); 1 = one batch at a time")
    ap.add_argument("--ingest", choices=INGEST_MODES, default="device",
                    help="where the files' samples are converted, resampled to 16 kHz and padded: on the GPU (default) or in numpy "
                         "on the host (16 kHz files give the same bits either way)")
    ap.add_argument("--scoring", choices=SCORING_MODES[::-1], default="device",
                    help="where the PER / PFER edit distances are computed: all pairs in one launch on the GPU (default) or pair by "
                         "pair in Python on the host (PER is equal either way, PFER to float64 rounding)")
    ap.add_argument("--base-decode", choices=BASE_DECODE_MODES, default="decode",
                    help="the base-model leg: 'decode' = the checkpoint leg's decode(without_timestamps=True) (default, as before); "
                         "'transcribe' = whisper_ipa_amd.transcribe, the call the reference makes for it (timestamps on, timestamp "
                         "rules, segments, no-speech skip, 30 s windows)")
    ap.add_argument("--decode", choices=DECODE_MODES, default="lockstep",
                    help="how decode(without_timestamps=True) walks the clips: 'lockstep' = batches of --batch-size, each run until its "
                         "last row ends (default, as before); 'continuous' = whisper_ipa_amd.decode_continuous: --batch-size rows, and a "
                         "row whose clip has ended takes the next clip (--passes-in-flight does not apply); with --base-decode "
                         "transcribe the base leg runs transcribe(schedule='continuous', slots=--batch-size)")
    ap.add_argument("--seed", type=int, default=None,
                    help="with --base-decode transcribe: re-decode the windows that fail the compression-ratio / log-probability "
                         "thresholds at 0.2, 0.4, ... 1.0 as mlx_whisper.transcribe does, sampling reproducibly from this seed "
                         "(default: temperature 0 only)")
    ap.add_argument("--condition-on-previous-text", action="store_true",
                    help="with --base-decode transcribe: decode every window after a file's first with the file's previous tokens as "
                         "its prompt, as mlx_whisper.transcribe does by default (default here: off); served by --decode continuous too")
    ap.add_argument("--initial-prompt", type=str, default=None,
                    help="with --base-decode transcribe: mlx_whisper.transcribe's initial_prompt, the prompt of every file's first window")
    ap.add_argument("--beam-size", type=int, default=None,
                    help="with --base-decode transcribe: beam search with this many beams for every window's temperature-0 decode")
    ap.add_argument("--patience", type=float, default=None, help="with --beam-size: the finished store holds round(beam_size * patience) sequences")
    ap.add_argument("--length-penalty", type=float, default=None,
                    help="with --beam-size (or best-of retries): rank by sum_logprobs / ((5 + length) / 6) ** this instead of by length")
    ap.add_argument("--results-json", type=str, default=None, help="also write both result dicts here (rank 0)")
    ap.add_argument("--audio-ctx", type=int, default=None,
                    help="run both models on their first N audio positions of 20 ms (default: what the checkpoint's training_config.json "
                         "records, else all 1500).  A value other than the recorded one is used with a warning; clips longer than "
                         "N * 20 ms are cut and counted on a warning line")
    ap.add_argument("--allow-byte-fallback", action="store_true",
                    help="run without the Whisper vocabulary (WIPA_TIKTOKEN unset): hypotheses render ids >= 256 as <|idN|>; "
                         "synthetic weights only")
    ap.add_argument("--adapter", type=str, default=None, metavar="DIR",
                    help="score the base model with the LoRA adapter of DIR (adapter_model.safetensors + adapter_config.json, as a "
                         "--lora-rank training run writes them into its checkpoint directories) in place of --checkpoint")
    ap.add_argument("--adapter-bank", type=str, default=None, metavar="lang=DIR[,lang=DIR...]",
                    help="score the base model with one LoRA adapter per language kept unmerged (Whisper.set_adapter_bank): every sample "
                         "decodes under the adapter of its language field (locale), samples without a match on the base, all in one "
                         "mixed continuous decode; takes the place of the checkpoint leg")
    args = ap.parse_args(argv)
    bank_dirs = parse_adapter_bank(args.adapter_bank) if args.adapter_bank is not None else None
    if bank_dirs is not None and args.adapter is not None:
        ap.error("--adapter-bank and --adapter cannot be given together")
    if args.adapter is not None:
        args.checkpoint = args.adapter  # load_checkpoint_model applies the adapter files it finds there
    from whisper_ipa_amd.tokenizer import get_tokenizer, require_real_vocabulary

    require_real_vocabulary(get_tokenizer(True), args.allow_byte_fallback, "scoring a model's transcriptions")

    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist

        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    torch.set_num_threads(parallel.host_threads_per_rank())  # the host's cores shared among the ranks on it
    rank, _ = parallel.world()
    num_samples = None if args.num_samples == 0 else args.num_samples
    base_results = None
    beams = {k: v for k, v in (("beam_size", args.beam_size), ("patience", args.patience), ("length_penalty", args.length_penalty)) if v is not None}
    if beams and args.base_decode != "transcribe":
        ap.error("--beam-size / --patience / --length-penalty go with --base-decode transcribe")
    # both legs at ONE context: the requested one, else the one the checkpoint was trained at
    audio_ctx, warning = resolve_audio_ctx(args.audio_ctx, args.checkpoint)
    if warning and rank == 0:
        print(warning)
    if not args.skip_base:
        base_results = evaluate_model(args.base_model, args.test_data, num_samples, model_name="Base Whisper Model",
                                      is_checkpoint=False, n_mels=args.n_mels, base_model=args.base_model, batch_size=args.batch_size,
                                      passes_in_flight=args.passes_in_flight, ingest=args.ingest, scoring=args.scoring,
                                      base_decode=args.base_decode, seed=args.seed,
                                      condition_on_previous_text=args.condition_on_previous_text, initial_prompt=args.initial_prompt,
                                      decode=args.decode, beams=beams, audio_ctx=audio_ctx)
    trained_results = evaluate_model(args.checkpoint, args.test_data, num_samples, model_name="Trained Checkpoint",
                                     is_checkpoint=True, n_mels=args.n_mels, base_model=args.base_model, batch_size=args.batch_size,
                                     passes_in_flight=args.passes_in_flight, ingest=args.ingest, scoring=args.scoring, decode=args.decode,
                                     audio_ctx=audio_ctx, adapter_bank=bank_dirs)
    if rank == 0:
        if base_results:
            compare_models(base_results, trained_results)
        print("\n" + "=" * 70)
        print("✅ Evaluation Complete!")
        print("=" * 70)
        if args.results_json:
            Path(args.results_json).write_text(json.dumps({"base": base_results, "trained": trained_results}, indent=2))
    return {"base": base_results, "trained": trained_results}


if __name__ == "__main__":
    main()
