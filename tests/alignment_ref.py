"""numpy / torch restatement of word-timestamp alignment (openai-whisper timing.py find_alignment, which mlx_whisper ports;
[UPSTREAM-UNVERIFIED]: restated from memory, pinned by tests/golden/alignment.npz to the local transformers copy of the same
chain -- _extract_token_timestamps' softmax / std_mean / _median_filter / head mean and _dynamic_time_warping).

  weights_chain     steps 2-5: softmax over the window's own frames, z-score over tokens, median filter, head mean; float32 or
                    float64 (``dtype``)
  dtw_f32           step 6 on an already negated matrix: float32 cost with ONE float32 add per cell, by anti-diagonals
  word_times        step 7: jumps of the text index -> a start and an end per word
  token_probs       step 8
  decoder_forward_qk  oracle.whisper_ref's teacher-forced decoder, rebuilt from its helpers so that every layer's cross q.k^T
                    (both sides scaled by 64^-0.25) comes back with the logits
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

FILTER_WIDTH = 7
TIME_PER_FRAME = 0.02


def median_filter(x: np.ndarray, width: int = FILTER_WIDTH) -> np.ndarray:
    """along the last axis, reflect padding of width // 2; an input with <= width // 2 frames is returned as it is"""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def weights_chain(qk, n_frames: int, dtype=np.float32) -> np.ndarray:
    """qk [heads, T, >= n_frames] -> [T, n_frames]: softmax over frames [0, n_frames), (w - mean) / std over the T rows
    (population std, no epsilon), median filter, mean over heads -- every operation in ``dtype``"""
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    w = torch.as_tensor(np.asarray(qk)).to(tdt)[..., :n_frames]
    w = torch.softmax(w, dim=-1).numpy()
    mean = w.mean(axis=-2, keepdims=True, dtype=dtype)
    std = np.sqrt(((w - mean) ** 2).mean(axis=-2, keepdims=True, dtype=dtype))
    w = ((w - mean) / std).astype(dtype)
    w = median_filter(w)
    return w.mean(axis=0, dtype=dtype)


def dtw_f32(x) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """x [N, M] (ALREADY negated) -> (text_indices, time_indices, cost [N+1, M+1] f32, trace).  Every cell is
    float32(x[i-1, j-1]) + float32(c) in float32, c chosen by upstream's strict-less rule; cells of one anti-diagonal do not
    depend on each other, so walking diagonals changes no bit."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = -np.ones((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2)).astype(np.float32)
        cost[i, j] = np.add(x[i - 1, j - 1], c, dtype=np.float32)
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    ti, tj = [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        tj.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1], dtype=np.int64), np.array(tj[::-1], dtype=np.int64), cost, trace


def dtw_min_cost_f64(x) -> float:
    """the cost of the cheapest monotone path through x [N, M] (ALREADY negated), in float64: what the best alignment costs"""
    x = np.asarray(x, dtype=np.float64)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf)
    cost[0, 0] = 0
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        cost[i, j] = x[i - 1, j - 1] + np.minimum(np.minimum(cost[i - 1, j - 1], cost[i - 1, j]), cost[i, j - 1])
    return float(cost[N, M])


def path_cost(x, text_indices, time_indices) -> float:
    """sum of the (negated) matrix along a path, in float64"""
    return float(np.asarray(x, dtype=np.float64)[np.asarray(text_indices), np.asarray(time_indices)].sum())


def word_times(text_indices, time_indices, word_tokens: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """step 7.  ``word_tokens``: split_to_word_tokens(text_tokens + [eot])[1]"""
    word_boundaries = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    jump_times = np.asarray(time_indices)[jumps] * TIME_PER_FRAME
    return jump_times[word_boundaries[:-1]], jump_times[word_boundaries[1:]]


def token_probs(logits, text_tokens: Sequence[int], first_row: int, eot: int) -> np.ndarray:
    """step 8: logits [T, V] of tokens = [*sot_sequence, no_timestamps, *text_tokens, eot], first_row = len(sot_sequence)"""
    p = torch.softmax(torch.as_tensor(np.asarray(logits))[first_row:, :eot].double(), dim=-1).numpy()
    return np.array([p[k, t] for k, t in enumerate(text_tokens)], dtype=np.float64)


def decoder_forward_qk(R, W, dims, tokens: torch.Tensor, xa: torch.Tensor):
    """R = oracle.whisper_ref.  tokens [B, T], xa [B, 1500, d] -> (logits [B, T, V], [per layer: q.k^T [B, H, T, 1500]])"""
    B, T = tokens.shape
    H = dims.n_text_head
    x = W["decoder.token_embedding.weight"][tokens] + W["decoder.positional_embedding"][:T]
    mask = R.causal_mask(max(dims.n_text_ctx, T))
    qks: List[torch.Tensor] = []
    for i in range(dims.n_text_layer):
        p = f"decoder.blocks.{i}"
        y, _ = R._mha(R._layer_norm(x, W, p + ".attn_ln"), W, p + ".attn", H, mask=mask)
        x = x + y
        xn = R._layer_norm(x, W, p + ".cross_attn_ln")
        q = R._linear(xn, W, p + ".cross_attn.query")
        k = R._linear(xa, W, p + ".cross_attn.key")
        hd = q.shape[-1] // H
        scale = hd ** -0.25
        qh = q.view(B, T, H, hd).permute(0, 2, 1, 3) * scale
        kh = k.view(B, k.shape[1], H, hd).permute(0, 2, 3, 1) * scale
        qks.append(qh @ kh)
        y, _ = R._mha(xn, W, p + ".cross_attn", H, xa=xa)
        x = x + y
        h = R._gelu(R._linear(R._layer_norm(x, W, p + ".mlp_ln"), W, p + ".mlp1"))
        x = x + R._linear(h, W, p + ".mlp2")
    x = R._layer_norm(x, W, "decoder.ln")
    return x @ W["decoder.token_embedding.weight"].T, qks


def alignment_matrix(qks, b: int, heads: Sequence[Tuple[int, int]], n_tokens: int, n_frames: int, dtype=np.float64) -> np.ndarray:
    """clip b's [n_tokens, n_frames] head-mean matrix from decoder_forward_qk's per-layer q.k^T"""
    qk = np.stack([qks[l][b, h, :n_tokens].detach().numpy() for l, h in heads])
    return weights_chain(qk, n_frames, dtype)
