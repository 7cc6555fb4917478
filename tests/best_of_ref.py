"""CPU restatement of best-of-N sampling (upstream's n_group = best_of with MaximumLikelihoodRanker): the candidate-stream rule, the
length penalty and the ranker in Python floats, and the per-candidate check of a sampled history against the draw of
tests/sampling_ref.py.  What wipa_rank_groups and decode(best_of=) are tested against."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

import sampling_ref as SR
import timestamp_ref as TR

MARGIN = 1e-3  # as tests/test_gpu_sampling.py: f32 keys below 256 in magnitude have an ulp <= 1.5e-5, 30 x headroom


def candidate_stream(stream, k: int) -> Tuple[int, int]:
    """candidate k of a row with stream (lo, hi) draws from (lo, hi + (k << 24)); candidate 0 keeps the row's stream"""
    lo, hi = int(stream[0]), int(stream[1])
    return lo, hi + (k << 24)


def candidate_streams(streams: Sequence, n_group: int) -> List[Tuple[int, int]]:
    """clip-major: the n_group streams of clip 0, then those of clip 1, ..."""
    return [candidate_stream(s, k) for s in streams for k in range(n_group)]


def penalty(length: int, length_penalty: Optional[float]) -> float:
    """MaximumLikelihoodRanker: ``length`` without a length penalty, else the Google NMT penalty ((5 + length) / 6) ** alpha"""
    if length_penalty is None:
        return float(length)
    return ((5 + length) / 6) ** length_penalty


def generated_length(row: Sequence[int], eot: int) -> int:
    """upstream's slice t[sample_begin : first eot]: the tokens before the first EOT, all of them when there is none"""
    row = [int(t) for t in row]
    return row.index(eot) if eot in row else len(row)


def rank(tokens: np.ndarray, sum_logprobs: np.ndarray, n_group: int, sample_begin: int, n: int, eot: int,
         length_penalty: Optional[float] = None):
    """-> (winner [clips], lengths [clips, G], scores [clips, G] as Python floats).  score = float(f32 sum) / penalty(length) in Python
    (IEEE double) arithmetic; length 0 scores -inf (the one deviation: upstream divides by zero); the winner is the FIRST maximum."""
    tokens = np.asarray(tokens)
    B = tokens.shape[0]
    assert B % n_group == 0
    winner, lengths, scores = [], [], []
    for c in range(B // n_group):
        ls, sc = [], []
        for k in range(n_group):
            b = c * n_group + k
            length = generated_length(tokens[b, sample_begin:sample_begin + n], eot)
            ls.append(length)
            sc.append(float(np.float32(sum_logprobs[b])) / penalty(length, length_penalty) if length > 0 else float("-inf"))
        best = 0
        for k in range(1, n_group):
            if sc[k] > sc[best]:
                best = k
        winner.append(best)
        lengths.append(ls)
        scores.append(sc)
    return np.array(winner, dtype=np.int64), np.array(lengths, dtype=np.int64), scores


def check_history(trace: np.ndarray, hist: Sequence[int], n_init: int, eot: int, seed: int, temperature: float, stream, attempt: int,
                  m_first: np.ndarray, m_always: np.ndarray, rules: Optional[dict], steps: int):
    """One candidate's sampled history against the restated draw on the logits of its OWN history (``trace`` [n_steps, V]: the
    unfiltered logits of positions n_init - 1 ..., from forced_decode_logits).  Every sampled position of the row, its EOT included,
    is redrawn; a position whose key margin exceeds MARGIN must reproduce the token.  -> (checked, left out, sum of log-probs)"""
    V = trace.shape[1]
    hist = [int(t) for t in hist]
    body = hist[n_init:]
    n_tok = body.index(eot) if eot in body else len(body)
    checked = left_out = 0
    slp = 0.0
    for i in range(min(n_tok + 1, steps, len(body))):
        p = n_init - 1 + i
        noise = SR.gumbel_noise(seed, [stream], attempt, p, V)[0]
        st = SR.sample_row(trace[i], temperature, noise, m_first if i == 0 else m_always, rules, body[:i], i == 0)
        got = body[i]
        assert np.isfinite(st.row[got]), (i, got)
        slp += st.row[got] - st.lse
        if st.key_margin > MARGIN:
            assert got == st.next, (i, got, st.next, st.key_margin)
            checked += 1
        else:
            left_out += 1
    return checked, left_out, slp
