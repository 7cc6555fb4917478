"""numpy restatement of beam search as openai-whisper's decoding.py does it (BeamSearchDecoder.update / finalize with
MaximumLikelihoodRanker), written from the description in include/wipa.h: what csrc/beam.hip, decode(beam_size=) and
transcribe(beam_size=) are tested against.  One clip at a time: a clip's beams never look at another clip."""
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

import best_of_ref as BR
import timestamp_ref as TR

LOGITS_TOL = 1e-3  # the project's f32 logits tolerance (tests/test_gpu_model.py): what one row's score may be off by


def required_margin(steps: int) -> float:
    """two rows compared, each with at most ``steps`` accumulated adds of a log-probability that is off by at most LOGITS_TOL"""
    return 2 * steps * LOGITS_TOL


def filtered_row(logits: np.ndarray, mask: np.ndarray, rules: Optional[dict], seq: Sequence[int], eot: int, first: bool) -> np.ndarray:
    """the row every tail reduces, float64: logits + mask, then rules 1-5 when ``rules`` = dict(tb, nt, max_init) is given"""
    if rules is None:
        return np.asarray(logits, dtype=np.float64) + np.asarray(mask, dtype=np.float64)
    return TR.apply_rules(logits, seq, rules["tb"], rules["nt"], eot, first, rules["max_init"], mask).row


def logprobs(row: np.ndarray) -> np.ndarray:
    return row - TR._logsumexp(row)


def top_columns(row: np.ndarray, k: int) -> np.ndarray:
    """the k best columns, lowest column on ties (a dead column is -inf and still a column)"""
    return np.argsort(-row, kind="stable")[:k]


@dataclass
class Clip:
    tokens: np.ndarray                      # [G, L] int64: the live beams
    sums: np.ndarray                        # [G] float32
    finished: List[Tuple[List[int], np.float32]] = field(default_factory=list)  # (sequence with its EOT, score), in store order
    anc: Optional[np.ndarray] = None        # [G, n_ctx] uint8: the ancestor table, when the caller tracks it
    src: Optional[np.ndarray] = None        # [G] the last step's sources
    margin: float = np.inf                  # the smallest gap of an order decision that mattered, over all steps
    steps: int = 0


def update(clip: Clip, rows: Sequence[np.ndarray], eot: int, max_candidates: int, first: bool) -> None:
    """one step of one clip.  ``rows``: the G filtered rows (float64).  Candidates: every beam's G + 1 best columns (beam 0 alone when
    ``first``), cumulative score = f32(sum) + f32(logprob) in f32, walked in descending score (ties: lower beam, then lower rank)."""
    G, L = clip.tokens.shape
    cands = []  # (score f32, beam, rank, column)
    next_gap = np.inf
    for j in range(1 if first else G):
        lp = logprobs(rows[j])
        cols = top_columns(rows[j], G + 2)
        for rk, c in enumerate(cols[:G + 1]):
            cands.append((np.float32(clip.sums[j]) + np.float32(lp[c]), j, rk, int(c)))
        if len(cols) > G + 1:  # the column the row did not offer: it matters when the row's last offer is taken
            next_gap = min(next_gap, float(lp[cols[G]] - lp[cols[G + 1]]))
    order = sorted(range(len(cands)), key=lambda i: (-float(cands[i][0]), cands[i][1], cands[i][2]))
    beams, newly, visited = [], [], []
    for i in order:
        visited.append(i)
        if len(beams) == G:  # the first candidate the walk does not reach: the gap to it is an order decision too
            break
        score, j, rk, c = cands[i]
        (newly if c == eot else beams).append((score, j, rk, c))
    for a, b in zip(visited, visited[1:]):
        gap = float(cands[a][0]) - float(cands[b][0])
        if np.isfinite(gap):
            clip.margin = min(clip.margin, gap)
    if any(rk == G for _, _, rk, _ in beams + newly):
        clip.margin = min(clip.margin, next_gap)
    old_tokens, old_anc = clip.tokens.copy(), None if clip.anc is None else clip.anc.copy()
    for score, j, rk, c in newly:  # already in descending score: the walk's order
        if len(clip.finished) < max_candidates:
            clip.finished.append((old_tokens[j].tolist() + [eot], np.float32(score)))
    src = np.array([j for _, j, _, _ in beams], dtype=np.int64)
    clip.tokens = np.concatenate([old_tokens[src], np.array([[c] for _, _, _, c in beams], dtype=np.int64)], axis=1)
    clip.sums = np.array([s for s, _, _, _ in beams], dtype=np.float32)
    clip.src = src
    if old_anc is not None:
        clip.anc = old_anc.copy()
        clip.anc[:, :L] = old_anc[src][:, :L]  # column L - 1 = p held the identity: it now names the source
    clip.steps += 1


def complete(clip: Clip, max_candidates: int) -> bool:
    return len(clip.finished) >= max_candidates


def finalize(clip: Clip, eot: int) -> None:
    """fewer than G finished: live beams + EOT in descending sum (lower beam on ties) until there are G"""
    G = clip.tokens.shape[0]
    for j in sorted(range(G), key=lambda j: (-float(clip.sums[j]), j)):
        if len(clip.finished) >= G:
            break
        clip.finished.append((clip.tokens[j].tolist() + [eot], np.float32(clip.sums[j])))


def rank(clip: Clip, sample_begin: int, eot: int, length_penalty: Optional[float]):
    """-> (index of the winner in the store, its generated tokens, its f32 sum): float(sum) / penalty(length), first maximum"""
    best, best_score = 0, None
    for k, (seq, score) in enumerate(clip.finished):
        length = BR.generated_length(seq[sample_begin:], eot)
        sc = float(score) / BR.penalty(length, length_penalty) if length > 0 else float("-inf")
        if best_score is None or sc > best_score:
            best, best_score = k, sc
    seq, score = clip.finished[best]
    return best, seq[sample_begin:sample_begin + BR.generated_length(seq[sample_begin:], eot)], np.float32(score)


@dataclass
class BeamResult:
    tokens: List[int]      # the winner's generated tokens, before EOT
    sum_logprob: np.float32
    clip: Clip
    steps: int


def decode_clip(logits_fn: Callable[[np.ndarray], np.ndarray], initial: Sequence[int], beam_size: int, patience: Optional[float],
                length_penalty: Optional[float], eot: int, sample_len: int, m_first: np.ndarray, m_always: np.ndarray,
                rules: Optional[dict] = None) -> BeamResult:
    """the decode of one clip.  ``logits_fn(tokens [G, L]) -> [G, V]``: the unfiltered logits after every beam's last token."""
    G = int(beam_size)
    max_candidates = round(G * (1.0 if patience is None else patience))
    n_init = len(initial)
    clip = Clip(np.array([list(initial)] * G, dtype=np.int64), np.zeros(G, dtype=np.float32))
    for i in range(sample_len):
        logits = logits_fn(clip.tokens)
        rows = [filtered_row(logits[j], m_first if i == 0 else m_always, rules, clip.tokens[j, n_init:].tolist(), eot, i == 0) for j in range(G)]
        update(clip, rows, eot, max_candidates, i == 0)
        if complete(clip, max_candidates):
            break
    steps = clip.steps
    finalize(clip, eot)
    _, toks, s = rank(clip, n_init, eot, length_penalty)
    return BeamResult([int(t) for t in toks], s, clip, steps)


def oracle_logits_fn(R, W, dims, xa_clip: torch.Tensor):
    """``logits_fn`` on the CPU oracle: the teacher-forced decoder on every beam's whole sequence (no cache to permute), last position"""
    def fn(tokens: np.ndarray) -> np.ndarray:
        with torch.no_grad():
            t = torch.from_numpy(np.asarray(tokens, dtype=np.int64))
            xa = xa_clip[None].expand(t.shape[0], -1, -1)
            return R.decoder_forward(W, dims, t, xa)[:, -1].float().numpy()
    return fn


def min_margin(results: Sequence[BeamResult]) -> float:
    """the smallest gap between a chosen and the best rejected cumulative score (and every other order decision the walk made), over all
    steps of all given decodes"""
    return min(float(r.clip.margin) for r in results)
