"""Inference entry point with the behaviour of the reference's scripts/transcribe_single.py:
base model -> fp32 -> overlay the fine-tuned ``decoder.*`` tensors of ``<checkpoint>/model.safetensors``
(reference :10-39), then load_audio -> pad_or_trim (one GPU launch: load_audio_batch) -> log_mel_spectrogram -> model.encoder -> greedy
``decode(language="en", without_timestamps=True)`` -> ``result[0].text.strip()`` (reference :41-56).

The reference hard-codes its three paths (:10,59-60) and fetches the base model by hub name; here
the same constants are the defaults and can be overridden on the command line, and the base
model is a local directory (config.json + weights.safetensors) because there is no network.
All compute runs in libwipa.so on the GPU.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from whisper_ipa_amd.audio import load_audio_batch, log_mel_spectrogram  # noqa: E402
from whisper_ipa_amd.decoding import DecodingOptions, decode  # noqa: E402
from whisper_ipa_amd.load_models import load_model, overlay_decoder_weights, resolve_audio_ctx  # noqa: E402


def load_checkpoint_model(checkpoint_path: str, base_model: str = "mlx-community/whisper-large-v3-mlx", audio_ctx=None):
    """``audio_ctx``: --audio-ctx; without one the value the checkpoint's training_config.json recorded is used, and a different one
    is used with a warning (load_models.resolve_audio_ctx)"""
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
    if checkpoint_path:
        try:
            n = overlay_decoder_weights(model, checkpoint_path)
        except FileNotFoundError as e:
            print(f"ERROR: {e}")
            sys.exit(1)
        print(f"Found {n} decoder parameters to load")
        print("✓ Decoder weights loaded successfully")
    return model


def transcribe_file(model, audio_path: str, temperature: float = 0.0, seed=None, best_of=None, beam_size=None, patience=None,
                    length_penalty=None) -> str:
    print(f"Transcribing {audio_path}...")
    report = {}
    audio = load_audio_batch([audio_path], audio_ctx=model.audio_ctx, report=report)  # load_audio -> pad_or_trim (reference :43-44) on the GPU: [1, 480000]
    if report["longer_than_audio_ctx"]:
        print(f"WARNING: {audio_path} is longer than audio_ctx {model.audio_ctx} ({model.audio_ctx * 0.02:.2f} s) and is cut")
    mel = log_mel_spectrogram(audio, n_mels=model.dims.n_mels).to(torch.float32)
    # IPA is decoded "as English"; a temperature above 0 samples, reproducibly, from ``seed``; ``best_of`` candidates, the best one kept
    # ``beam_size`` (temperature 0): beam search, with ``patience`` and ``length_penalty`` as upstream's DecodingOptions take them
    options = DecodingOptions(language="en", without_timestamps=True, temperature=temperature, seed=seed, best_of=best_of, beam_size=beam_size,
                              patience=patience, length_penalty=length_penalty)
    audio_features = model.encoder(mel)
    result = decode(model, audio_features, options)
    return result[0].text.strip()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", default="checkpoints/whisper-ipa/checkpoint-8000")
    ap.add_argument("--audio", default="4.wav")
    ap.add_argument("--base-model", default="mlx-community/whisper-large-v3-mlx",
                    help="local directory with config.json + weights.safetensors (hub names cannot resolve offline)")
    ap.add_argument("--temperature", type=float, default=0.0, help="above 0: sample instead of taking the arg-max (needs --seed)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the sampling draw: the same seed gives the same transcript")
    ap.add_argument("--best-of", type=int, default=None,
                    help="with --temperature above 0: draw this many candidates and keep the one with the highest length-normalised log-probability")
    ap.add_argument("--beam-size", type=int, default=None, help="at temperature 0: beam search with this many beams (1..16)")
    ap.add_argument("--patience", type=float, default=None, help="with --beam-size: the finished store holds round(beam_size * patience) sequences")
    ap.add_argument("--length-penalty", type=float, default=None,
                    help="with --beam-size or --best-of: rank by sum_logprobs / ((5 + length) / 6) ** this instead of by length")
    ap.add_argument("--word-timestamps", action="store_true",
                    help="transcribe through whisper_ipa_amd.transcribe(word_timestamps=True) and also print one line per word (start, end, probability)")
    ap.add_argument("--allow-byte-fallback", action="store_true",
                    help="run without the Whisper vocabulary (WIPA_TIKTOKEN unset): ids >= 256 print as <|idN|>; synthetic weights only")
    ap.add_argument("--audio-ctx", type=int, default=None,
                    help="run the model on its first N audio positions of 20 ms (default: what the checkpoint's training_config.json "
                         "records, else all 1500); a clip longer than N * 20 ms is cut, with a warning")
    ap.add_argument("--adapter", default=None, metavar="DIR",
                    help="transcribe with the base model and the LoRA adapter of DIR (adapter_model.safetensors + adapter_config.json) "
                         "in place of --checkpoint")
    args = ap.parse_args(argv)
    if args.adapter is not None:
        args.checkpoint = args.adapter  # load_checkpoint_model applies the adapter files it finds there
    from whisper_ipa_amd.tokenizer import get_tokenizer, require_real_vocabulary

    require_real_vocabulary(get_tokenizer(True), args.allow_byte_fallback, "transcribing with a trained checkpoint")
    model = load_checkpoint_model(args.checkpoint, args.base_model, audio_ctx=args.audio_ctx)
    if args.word_timestamps and model.audio_ctx is not None:
        ap.error("--word-timestamps goes through transcribe(), which is not implemented for a model with audio_ctx set")
    if args.temperature != 0.0 and args.seed is None:
        ap.error("--temperature above 0 needs --seed")
    if args.best_of is not None and args.temperature == 0.0 and not args.word_timestamps:
        ap.error("--best-of needs --temperature above 0 (best_of with greedy sampling is not compatible)")
    if args.beam_size is not None and (args.temperature != 0.0 or args.word_timestamps):
        ap.error("--beam-size runs at temperature 0 and without --word-timestamps")
    words = []
    if args.word_timestamps:  # one decode: the prediction is the transcript the words belong to
        if args.temperature != 0.0:
            ap.error("--word-timestamps goes through transcribe(), whose schedule starts at temperature 0: drop --temperature")
        from whisper_ipa_amd import transcribe

        print(f"Transcribing {args.audio}...")
        out = transcribe(model, args.audio, language="en", word_timestamps=True, seed=args.seed,
                         **({"best_of": args.best_of} if args.best_of is not None else {}))
        text = out["text"].strip()
        words = [w for seg in out["segments"] for w in seg.get("words", [])]
    else:
        text = transcribe_file(model, args.audio, temperature=args.temperature, seed=args.seed, best_of=args.best_of, beam_size=args.beam_size,
                               patience=args.patience, length_penalty=args.length_penalty)
    print("\n" + "=" * 50)
    print(f"Audio: {args.audio}")
    print(f"Prediction: {text}")
    print("=" * 50)
    for w in words:
        print(f"[{w['start']:7.2f} -> {w['end']:7.2f}] p={w['probability']:.3f} {w['word']}")
    return text


if __name__ == "__main__":
    main()
