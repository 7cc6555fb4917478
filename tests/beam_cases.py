"""The cases tests/test_beam_host.py and tests/test_gpu_beam.py share: crafted single-step scenes for wipa_beam_step, and the
(fixture clip, option set) list of the model tests with the restatement's decode of each -- computed once per process."""
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import beam_ref as BM
import prompt_ref as PR
from oracle import whisper_ref as R

# ---------------------------------------------------------------- crafted rows for wipa_beam_step
V = 1003            # V % 4 != 0: the row's three trailing columns take the scalar path
EOT, TB, NT = 880, 900, 890
N_INIT = 3
INITIAL = [870, 871, 872]
RULES = dict(tb=TB, nt=NT, max_init=50)
CRAFT_GAP = 1e-2    # crafted score gaps are at least this


def crafted_rows(seed: int, G: int, clips: int, eot_rank: Optional[int], spread: float = 0.37) -> np.ndarray:
    """[clips * G, V] f32 logits: small noise, and per row G + 2 boosted columns ``spread`` apart (a text column each, distinct per row);
    ``eot_rank``: EOT takes that rank among the row's boosted columns (0: every beam's best candidate is EOT; None: no EOT)"""
    rng = np.random.default_rng(seed)
    B = clips * G
    logits = (rng.standard_normal((B, V)) * 1e-3).astype(np.float32)
    for b in range(B):
        cols = rng.choice(np.arange(10, 800), size=G + 2, replace=False)
        for k, c in enumerate(cols):
            logits[b, EOT if k == eot_rank else c] = np.float32(6.0 - spread * k - 0.113 * (b % G) - 0.0291 * (b // G))
    return logits


SCENES = {
    # name: (G, patience, steps as (eot_rank, first generated step?), with rules?)
    "eot_inside_top": (3, None, [(1, False)], False),
    "eot_best_of_every_beam": (2, None, [(0, False)], False),
    "store_overflow_patience_1": (2, None, [(0, False), (0, False)], False),
    "store_overflow_patience_2": (2, 2.0, [(0, False), (0, False), (0, False)], False),
    "first_generated_step": (3, None, [(None, True), (2, False)], False),
    "completes_then_steps_on": (2, 0.5, [(0, False), (None, False), (None, False)], False),  # max_candidates 1 < G: filled at step 0
    "rules_timestamp_pair": (2, None, [(None, False)], True),  # the history ends in a closed timestamp pair: text next
}


# ---------------------------------------------------------------- the model cases
SAMPLE_LEN = 12
FIXTURE_SEED, LOGIT_SCALE = 1, 64.0  # found by a search over seeds 1..7 x scales 16..128 for the first pair that meets the margin
MODEL_CASES = [(G, patience, timed) for G in (2, 5) for patience in (None, 2.0) for timed in (False, True)]
LENGTH_PENALTIES = (None, 0.6)


def required_margin() -> float:
    return BM.required_margin(SAMPLE_LEN)


def decode_inputs(timed: bool):
    """(initial tokens, suppress_always, suppress_first, rules dict or None) of the model tests"""
    sp = PR.SP
    always, first = R.suppress_lists(sp)
    initial = list(PR.SOT_SEQUENCE) if timed else list(PR.SOT_SEQUENCE) + [sp.no_timestamps]
    rules = dict(tb=sp.timestamp_begin, nt=sp.no_timestamps, max_init=50) if timed else None
    return initial, always, first, rules


@functools.lru_cache(maxsize=None)
def micro_fixture():
    """(W, features [2, 1500, d] f32) of the MICRO f32 model on the two fixture clips, on the CPU oracle"""
    import torch

    W = R.synthetic_weights(PR.MICRO, seed=FIXTURE_SEED)
    # the synthetic model's logits are nearly flat, and flat rows put the beams' scores closer together than an f32 device can be asked
    # to resolve: the final LayerNorm is scaled, which scales the logits, so that the restatement alone meets required_margin()
    W["decoder.ln.weight"] = W["decoder.ln.weight"] * LOGIT_SCALE
    W["decoder.ln.bias"] = W["decoder.ln.bias"] * LOGIT_SCALE
    with torch.no_grad():
        xa = R.encoder_forward(W, PR.MICRO, PR.clip_mels())
    return W, xa


@functools.lru_cache(maxsize=None)
def restated(G: int, patience: Optional[float], timed: bool, length_penalty: Optional[float]) -> Tuple[BM.BeamResult, ...]:
    """the restatement's decode of both fixture clips for one option set"""
    W, xa = micro_fixture()
    sp = PR.SP
    initial, always, first, rules = decode_inputs(timed)
    Vm = PR.MICRO.n_vocab
    m_always = BM.TR.vocab_mask(Vm, always)
    m_first = BM.TR.vocab_mask(Vm, list(always) + list(first))
    return tuple(BM.decode_clip(BM.oracle_logits_fn(R, W, PR.MICRO, xa[c]), initial, G, patience, length_penalty, sp.eot, SAMPLE_LEN, m_first,
                                m_always, rules) for c in range(xa.shape[0]))


# ---------------------------------------------------------------- transcribe(beam_size=): the restatement's window loop
TRANSCRIBE_BEAMS = 2


def transcribe_audio():
    """a 40 s file (two windows at least) and a 5 s file"""
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    return [long, R.synthetic_clip(1, 5.0)[: 5 * 16000]]


def restatement_decode_fn(tok, beam_size: int, patience: Optional[float] = None, length_penalty: Optional[float] = None):
    """a ``decode_fn`` for whisper_ipa_amd.transcribe that decodes every window with the restatement on the CPU oracle (log-mel, encoder,
    beam search under the timestamp rules, no-speech probability of the [sot] pass); ``fn.margins`` collects every window's margin"""
    import torch

    from whisper_ipa_amd.decoding import DecodingResult, compression_ratio

    W, _ = micro_fixture()
    sp = PR.SP
    initial, always, first, rules = decode_inputs(True)
    Vm = PR.MICRO.n_vocab
    m_always = BM.TR.vocab_mask(Vm, always)
    m_first = BM.TR.vocab_mask(Vm, list(always) + list(first))

    def fn(windows, languages):
        out = []
        for w in windows:
            with torch.no_grad():
                mel = torch.from_numpy(R.log_mel_spectrogram(np.asarray(w, dtype=np.float32)))[None]
                xa = R.encoder_forward(W, PR.MICRO, mel)
                sot_logits = R.decoder_forward(W, PR.MICRO, torch.tensor([[sp.sot]]), xa)[0, -1].double()
            r = BM.decode_clip(BM.oracle_logits_fn(R, W, PR.MICRO, xa[0]), initial, beam_size, patience, length_penalty, sp.eot, SAMPLE_LEN, m_first,
                               m_always, rules)
            fn.margins.append(float(r.clip.margin))
            text = tok.decode([t for t in r.tokens if t < sp.timestamp_begin]).strip()
            out.append(DecodingResult(audio_features=None, language="en", tokens=list(r.tokens), text=text,
                                      avg_logprob=float(r.sum_logprob) / (len(r.tokens) + 1),
                                      no_speech_prob=float(torch.softmax(sot_logits, -1)[sp.no_speech]), temperature=0.0,
                                      compression_ratio=compression_ratio(text)))
        return out

    fn.beams = True  # what transcribe asks of a custom decoder before it hands it beam_size
    fn.margins = []
    return fn


@functools.lru_cache(maxsize=None)
def restated_transcribe():
    """(transcribe's output through the restatement's decoder, the margins of the windows it decoded)"""
    import warnings

    from whisper_ipa_amd import transcribe
    from whisper_ipa_amd.tokenizer import get_tokenizer

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, language="en", task="transcribe")
        fn = restatement_decode_fn(tok, TRANSCRIBE_BEAMS)
        out = transcribe(None, transcribe_audio(), language="en", decode_fn=fn, tokenizer=tok, beam_size=TRANSCRIBE_BEAMS)
    return out, tuple(fn.margins)
