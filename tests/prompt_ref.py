"""CPU restatement of prompt conditioning: every row is decoded ALONE, batch of one, with its own unpadded initial tokens
([sot_prev] + history + sot_sequence) through tests/timestamp_ref.greedy_with_rules on the CPU oracle -- padding, a common prompt width
and per-row starts do not exist here.  What the ragged decode (include/wipa.h: wipa_decoder_begin_ragged / wipa_decode_call.starts_dev;
whisper_ipa_amd.decoding.ragged_decode_tokens) and transcribe's conditioning are tested against."""
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

import sampling_ref as SR
import timestamp_ref as TR
from oracle import whisper_ref as R

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
W384 = R.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
SP = R.SpecialTokens.multilingual()
V, TB, NT, EOT = 51865, SP.timestamp_begin, SP.no_timestamps, SP.eot
SOT_SEQUENCE = [SP.sot, SP.lang_first, SP.transcribe]
STEPS = 20
HISTORY_LENGTHS = (0, 1, 17, 70, 223)


def walking_script(n_ctx: int = 448) -> List[int]:
    """The 20-entry plot of ``TR.timestamp_script`` repeated over all positions, every text slot filled with a DIFFERENT id (448 distinct
    ids from default_rng(3).permutation(arange(1000, 50000)) minus the non-speech list): what the model wants next names the position
    it is at, so a wrong per-row position offset picks a wrong token at once.  script[p] is what the model wants at position p + 1."""
    base = TR.timestamp_script(n_ctx, TB, EOT, seed=3)
    plot = base[2:22]  # the plot starts at n_init - 1 = 2
    banned = set(R.NON_SPEECH_TOKENS_MULTI)
    ids = [int(t) for t in np.random.default_rng(3).permutation(np.arange(1000, 50000)) if int(t) not in banned][:n_ctx]
    assert len(set(ids)) == n_ctx
    script = []
    for p in range(n_ctx):
        t = plot[p % len(plot)]
        script.append(t if (t >= TB or t == EOT) else ids[p])
    return script


def weights(dims, seed: int, scripted: bool):
    W = R.synthetic_weights(dims, seed=seed)
    if scripted:
        W["decoder.positional_embedding"] = TR.scripted_positional_table(W, walking_script(dims.n_text_ctx))
    return W


def histories() -> List[List[int]]:
    """five histories of 0, 1, 17, 70 and 223 tokens, drawn in that order from ONE generator; every ninth token from the fourth on is
    a timestamp"""
    rng = np.random.default_rng(11)
    out = []
    for n in HISTORY_LENGTHS:
        body = [int(t) for t in rng.integers(1000, 50000, size=n)]
        for j in range(3, n, 9):
            body[j] = TB + 5 * j
        out.append(body)
    return out


def initial_rows() -> List[List[int]]:
    """row b's initial tokens: [sot_prev] + history + sot_sequence; the bare sot_sequence without a history"""
    return [([SP.sot_prev] + h if h else []) + SOT_SEQUENCE for h in histories()]


def clip_mels() -> torch.Tensor:
    clips = np.stack([R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0)])
    return torch.from_numpy(np.stack([R.log_mel_spectrogram(a) for a in clips]))


@dataclass
class RowRef:
    initial: List[int]
    loop: TR.RulesLoop          # batch of one: tokens [1, n_b + STEPS]
    sot_logits: np.ndarray      # [V] f32: the unfiltered logits at the row's <|startoftranscript|> position
    no_speech: float            # softmax(sot_logits)[no_speech]


def per_row_reference(W, dims, xa: torch.Tensor, rows: Sequence[Sequence[int]], n_steps: int = STEPS) -> List[RowRef]:
    """row b uses clip b % len(xa); each row alone through the rules loop, with every step's logits kept"""
    always, first = R.suppress_lists(SP)
    out = []
    for b, init in enumerate(rows):
        x = xa[b % xa.shape[0]: b % xa.shape[0] + 1]
        loop = TR.greedy_with_rules(R, W, dims, x, list(init), always, first, EOT, TB, NT, n_steps, keep_logits=True)
        k = len(init) - len(SOT_SEQUENCE)  # the row's sot position
        with torch.no_grad():
            sot = R.decoder_forward(W, dims, torch.tensor([list(init[: k + 1])], dtype=torch.long), x)[0, -1].float().numpy()
        pr = np.exp(sot.astype(np.float64) - TR._logsumexp(sot.astype(np.float64)))
        out.append(RowRef(list(init), loop, sot, float(pr[SP.no_speech])))
    return out


@dataclass
class SampleLoop:
    tokens: np.ndarray       # [n_b + n_steps]
    sum_logprob: float
    key_margins: np.ndarray  # [n_steps]: top-1 minus top-2 key of every draw (inf on latched steps)


def sample_row_loop(W, dims, x: torch.Tensor, initial: Sequence[int], n_steps: int, seed: int, temperature: float, stream, attempt: int = 0,
                    with_rules: bool = True) -> SampleLoop:
    """one row alone at a temperature above 0: the draw of tests/sampling_ref.py fed the row's OWN position (the index of the token
    whose logits these are in the row's unpadded sequence) as the counter's position word"""
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    rules = dict(tb=TB, nt=NT, eot=EOT, max_init=50) if with_rules else None
    tokens = torch.tensor([list(initial)], dtype=torch.long)
    cache = [dict() for _ in range(dims.n_text_layer)]
    n_init, slp = len(initial), 0.0
    margins = np.full(n_steps, np.inf)
    with torch.no_grad():
        for i in range(n_steps):
            inp = tokens if i == 0 else tokens[:, -1:]
            logits = R.decoder_forward(W, dims, inp, x, cache)[0, -1].float().numpy()
            p_own = tokens.shape[1] - 1
            if int(tokens[0, -1]) == EOT:
                nxt = EOT
            else:
                noise = SR.gumbel_noise(seed, [stream], attempt, p_own, V)[0]
                st = SR.sample_row(logits, temperature, noise, m_first if i == 0 else m_always, rules, tokens[0, n_init:].tolist(), i == 0)
                nxt, margins[i] = st.next, st.key_margin
                slp += st.logprob
            tokens = torch.cat([tokens, torch.tensor([[nxt]])], dim=1)
    return SampleLoop(tokens[0].numpy(), slp, margins)
