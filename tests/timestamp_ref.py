"""numpy restatement of the timestamp rules (ApplyTimestampRules of openai-whisper's decoding.py; transformers'
WhisperTimeStampLogitsProcessor is the same algorithm, tests/golden/timestamp_rules.json is recorded from it; mlx_whisper 0.4.3's
port is [UPSTREAM-UNVERIFIED]) and a greedy loop over the CPU oracle's KV-cached decoder that applies them and counts how often
every branch fires.  What the device tail (csrc/elementwise.hip: rules_row_pick) is tested against."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

BRANCHES = ("first_position", "text_after_closed_pair", "after_single_timestamp", "monotone_cut", "timestamp_mass_over_text",
            "text_over_timestamp_mass")


def _logsumexp(x: np.ndarray) -> float:
    m = x.max() if x.size else -np.inf
    if not np.isfinite(m):
        return -np.inf
    return float(m + np.log(np.exp(x - m).sum()))


@dataclass
class RuleStep:
    row: np.ndarray          # the filtered row, float64, -inf where a rule or a mask killed the column
    next: int                # arg-max, lowest index on ties
    logprob: float           # row[next] - logsumexp(row)
    fired: Dict[str, bool]   # which branches acted on this row
    margin: float            # top-1 minus top-2 of the filtered row
    mass_gap: float          # |logsumexp(timestamps) - max(text)| before rule 5 (inf when either side is empty)


def apply_rules(logits: np.ndarray, seq: Sequence[int], tb: int, nt: int, eot: int, first: bool, max_init_index: int = 50,
                mask: Optional[np.ndarray] = None) -> RuleStep:
    """``logits`` [V]; ``mask`` [V] of 0 / -inf (mask_first or mask_always, chosen by the caller); ``seq`` the tokens sampled so
    far; ``first``: this is the first sampled position (p + 1 == n_init); ``max_init_index`` < 0: no cap."""
    l = np.asarray(logits, dtype=np.float64).copy()
    if mask is not None:
        l = l + np.asarray(mask, dtype=np.float64)
    seq = [int(t) for t in seq]
    fired = {k: False for k in BRANCHES}
    l[nt] = -np.inf
    last = len(seq) >= 1 and seq[-1] >= tb
    pen = len(seq) < 2 or seq[-2] >= tb
    if last and pen:
        l[tb:] = -np.inf
        fired["text_after_closed_pair"] = True
    if last and not pen:
        l[:eot] = -np.inf
        fired["after_single_timestamp"] = True
    stamps = [t for t in seq if t >= tb]
    if stamps:
        t_last = stamps[-1] if (last and not pen) else stamps[-1] + 1  # the last in ORDER, not the maximum
        l[tb:t_last] = -np.inf
        fired["monotone_cut"] = True
    if first:
        l[:tb] = -np.inf
        if max_init_index >= 0:
            l[tb + max_init_index + 1:] = -np.inf
        fired["first_position"] = True
    ts, mt = _logsumexp(l[tb:]), float(l[:tb].max())
    gap = abs(ts - mt) if np.isfinite(ts) and np.isfinite(mt) else np.inf
    if ts > mt:
        l[:tb] = -np.inf
        fired["timestamp_mass_over_text"] = np.isfinite(mt)  # counted where there was a text token to beat
    elif np.isfinite(ts):
        fired["text_over_timestamp_mass"] = True
    nxt = int(np.argmax(l))
    top2 = np.sort(l)[-2:]
    return RuleStep(l, nxt, float(l[nxt] - _logsumexp(l)), fired, float(top2[1] - top2[0]), float(gap))


def case_logits(seed: int, scale: float, boosts, V: int, tb: int) -> np.ndarray:
    """the logits of a case of tests/golden/timestamp_rules.json: float32 normal draws x scale, then the boosted columns SET to their
    values; the column "ts" adds its value to every timestamp column"""
    l = (np.random.default_rng(seed).standard_normal(V) * scale).astype(np.float32)
    for col, val in boosts:
        if col == "ts":
            l[tb:] += np.float32(val)
        else:
            l[int(col)] = np.float32(val)
    return l


def vocab_mask(V: int, ids: Sequence[int]) -> np.ndarray:
    m = np.zeros(V, dtype=np.float32)
    m[list(ids)] = -np.inf
    return m


@dataclass
class RulesLoop:
    tokens: np.ndarray        # [B, n_init + n_steps] int64, EOT-latched
    sum_logprobs: np.ndarray  # [B]
    counts: Dict[str, int]    # how often each branch fired, over rows that were not latched
    margins: np.ndarray       # [B, n_steps]
    mass_gaps: np.ndarray     # [B, n_steps]
    step_logits: List[np.ndarray] = field(default_factory=list)  # per step [B, V] unfiltered f32 (keep_logits)


def greedy_with_rules(R, W, dims, xa: torch.Tensor, initial: Sequence[int], always: Sequence[int], first: Sequence[int], eot: int,
                      tb: int, nt: int, n_steps: int, max_init_index: int = 50, keep_logits: bool = False) -> RulesLoop:
    """DecodingTask._main_loop at temperature 0 with SuppressBlank, SuppressTokens and ApplyTimestampRules, on
    ``R.decoder_forward`` with its KV cache.  ``R`` is the oracle module (oracle.whisper_ref)."""
    B, V, n_init = xa.shape[0], dims.n_vocab, len(initial)
    m_always = vocab_mask(V, always)
    m_first = vocab_mask(V, list(always) + list(first))
    tokens = torch.tensor([list(initial)] * B, dtype=torch.long)
    cache = [dict() for _ in range(dims.n_text_layer)]
    slp = np.zeros(B, dtype=np.float64)
    counts = {k: 0 for k in BRANCHES}
    margins, gaps = np.zeros((B, n_steps)), np.zeros((B, n_steps))
    kept = []
    with torch.no_grad():
        for i in range(n_steps):
            inp = tokens if i == 0 else tokens[:, -1:]
            logits = R.decoder_forward(W, dims, inp, xa, cache)[:, -1].float().numpy()
            if keep_logits:
                kept.append(logits.copy())
            nxt = np.zeros(B, dtype=np.int64)
            for b in range(B):
                seq = tokens[b, n_init:].tolist()
                st = apply_rules(logits[b], seq, tb, nt, eot, i == 0, max_init_index, m_first if i == 0 else m_always)
                margins[b, i], gaps[b, i] = st.margin, st.mass_gap
                if int(tokens[b, -1]) == eot:
                    nxt[b] = eot
                    margins[b, i] = gaps[b, i] = np.inf  # a latched row's arithmetic decides nothing
                    continue
                nxt[b] = st.next
                slp[b] += st.logprob
                for k, v in st.fired.items():
                    counts[k] += int(v)
            tokens = torch.cat([tokens, torch.from_numpy(nxt)[:, None]], dim=1)
    return RulesLoop(tokens.numpy(), slp, counts, margins, gaps, kept)


def scripted_positional_table(W, script: Sequence[int], gain: float = 128.0) -> torch.Tensor:
    """``peaky_positional_table``'s construction with a GIVEN script instead of a random draw: position p's row carries
    gain * token_embedding[script[p]], so the model WANTS script[p] at position p + 1 with a wide margin -- and the rules decide
    whether it gets it.  ``script`` covers every position (n_text_ctx entries)."""
    idx = torch.tensor([int(t) for t in script], dtype=torch.long)
    return W["decoder.positional_embedding"] + gain * W["decoder.token_embedding.weight"][idx].float()


def timestamp_script(n_ctx: int, tb: int, eot: int, seed: int, n_init: int = 3) -> List[int]:
    """A script that walks every branch within 20 sampled positions: opening timestamp, text, a closing pair, text, a DECREASING
    timestamp (the monotone cut must refuse it), a pair, text right after a single timestamp (refused: only EOT or a timestamp
    may follow), EOT.  Text ids are a seeded draw from 1000..50000 that avoids the published non-speech list; the positions past the
    plot repeat EOT."""
    from oracle import whisper_ref as R

    rng = np.random.default_rng(seed)
    banned = set(R.NON_SPEECH_TOKENS_MULTI)
    pool = [int(t) for t in rng.permutation(np.arange(1000, 50000)) if int(t) not in banned][:32]
    a = iter(pool)
    T = tb
    plot = [T + 0, next(a), next(a), T + 100, T + 100, next(a), T + 40, next(a), T + 250, T + 250, next(a), next(a), T + 300,
            next(a), T + 400, T + 400, next(a), T + 450, eot, eot]
    script = [eot] * n_ctx
    # script[p] is what the model wants at position p + 1; the first sampled position is n_init
    for i, t in enumerate(plot):
        script[n_init - 1 + i] = t
    return script
