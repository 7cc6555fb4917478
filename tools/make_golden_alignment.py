"""Records tests/golden/alignment.npz from the local transformers copy of Whisper's word-timestamp chain:
``_median_filter`` and ``_dynamic_time_warping`` of transformers.models.whisper.generation_whisper, plus the softmax /
std_mean / head-mean steps written as ``_extract_token_timestamps`` writes them.  tests/alignment_ref.py is checked against it
(tests/test_alignment_host.py).

    python tools/make_golden_alignment.py

DTW cases hold a float32 matrix (already negated, as the chain passes it) and the recorded path; chain cases hold float64
q.k^T scores [heads, tokens, frames], the frame count used, and the recorded float64 matrix.
"""
import os

import numpy as np
import torch
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "alignment.npz")


def chain(qk: np.ndarray, n_frames: int) -> np.ndarray:
    w = torch.from_numpy(qk)[None]  # [1, heads, tokens, frames], float64
    w = w[..., :n_frames]
    w = w.softmax(dim=-1)
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    w = (w - mean) / std
    w = _median_filter(w, 7)
    return w.mean(dim=1)[0].numpy()


def main():
    rng = np.random.default_rng(20240607)
    out = {}
    dtw_cases = {
        "random_5x9": rng.standard_normal((5, 9)),
        "random_12x40": rng.standard_normal((12, 40)),
        "random_33x70": rng.standard_normal((33, 70)),
        "ties_quarter_9x30": rng.integers(-4, 5, (9, 30)) * 0.25,
        "ties_quarter_17x17": rng.integers(-2, 3, (17, 17)) * 0.25,
        "ties_all_equal_6x11": np.full((6, 11), 0.5),
        "ties_zero_4x4": np.zeros((4, 4)),
        "one_row_1x7": rng.standard_normal((1, 7)),
        "one_col_6x1": rng.standard_normal((6, 1)),
        "one_cell_1x1": rng.standard_normal((1, 1)),
        "tall_20x8": rng.standard_normal((20, 8)),
        "tall_ties_15x4": rng.integers(-1, 2, (15, 4)) * 0.25,
    }
    for name, m in dtw_cases.items():
        x = np.asarray(m, dtype=np.float32)
        ti, tj = _dynamic_time_warping(x)
        out[f"dtw/{name}/x"] = x
        out[f"dtw/{name}/text"] = np.asarray(ti, dtype=np.int32)
        out[f"dtw/{name}/time"] = np.asarray(tj, dtype=np.int32)
    for name, (h, t, f, nf) in {"f3": (2, 5, 8, 3), "f4": (3, 6, 4, 4), "f7": (1, 4, 9, 7), "f20": (3, 9, 24, 20), "f20_all": (2, 2, 20, 20)}.items():
        qk = rng.standard_normal((h, t, f)) * 2.0
        out[f"chain/{name}/qk"] = qk
        out[f"chain/{name}/n_frames"] = np.int32(nf)
        out[f"chain/{name}/matrix"] = chain(qk, nf)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(dtw_cases), "dtw cases")


if __name__ == "__main__":
    main()
