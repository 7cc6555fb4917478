"""GPU: word-timestamp alignment -- csrc/align.hip (wipa_align_weights, wipa_dtw_batch, wipa_token_probs), wipa_decoder_align
and whisper_ipa_amd.timing / transcribe(word_timestamps=True) -- against the numpy / torch restatement of tests/alignment_ref.py.
Reference: openai-whisper timing.py find_alignment, which mlx_whisper ports ([UPSTREAM-UNVERIFIED]).
``pytest -m gpu`` on an MI355X."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import alignment_ref as AR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
W384 = R.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)  # the absorbed-eligible shape
SP = R.SpecialTokens.multilingual()
TB, EOT = SP.timestamp_begin, SP.eot
SOT_SEQ = [SP.sot, SP.lang_first, SP.transcribe]
TA = 1500
QK_SCALE = 64 ** -0.25
CAP = 1e-4        # the weights kernel: a wrong frame, row or head moves a z-scored cell by O(0.1 - 1)
MODEL_CAP = 0.05  # the model-level matrix against the oracle's forward
# largest |matrix - restatement on the oracle's forward| measured on an MI355X (printed by the tests below)
DELTA_MICRO_F32 = {"default": 2.275e-5, "pairs": 2.981e-5}


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---------------------------------------------------------------- the weights kernel through the C ABI
def _weights(q, k, heads, n_tokens, n_frames, divisor=0.0):
    """q [B, T, d], k [B, H, 1500, 64] (torch, one dtype) -> out [B, T, 1500] f32 numpy; cells outside a clip's range stay 0"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import dt_code, on_stream, ptr, sptr

    L = _lib.lib()
    B, T, d = q.shape
    H = k.shape[1]
    hh = np.asarray(heads, dtype=np.int32)
    with on_stream() as s:
        qd, kd = q.cuda().contiguous(), k.cuda().contiguous()
        nt = torch.tensor(list(n_tokens), dtype=torch.int32, device="cuda")
        nf = torch.tensor(list(n_frames), dtype=torch.int32, device="cuda")
        need = L.wipa_align_weights_scratch_bytes(B, T, len(hh), TA)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.zeros(B, T, TA, dtype=torch.float32, device="cuda")
        _lib.check(L.wipa_align_weights(ptr(qd), ptr(kd), H * TA * 64, TA * 64, dt_code(q.dtype), B, T, d, TA, _i32p(hh), len(hh), ptr(nt), ptr(nf),
                                        ptr(scratch), need, ptr(out), TA, float(divisor), sptr(s)), "wipa_align_weights")
        res = out.cpu().numpy()
    return res


def _draw(rng, B, T, H, dtype):
    """q with std 3 * 64^-0.25 and k with std 64^-0.25: scores of std 3, softmaxes with a few strong frames"""
    q = torch.from_numpy((rng.standard_normal((B, T, H * 64)) * 3.0 * QK_SCALE).astype(np.float32)).to(dtype)
    k = torch.from_numpy((rng.standard_normal((B, H, TA, 64)) * QK_SCALE).astype(np.float32)).to(dtype)
    return q, k


def _scores(q, k, b, heads, nt):
    """float64 q.k^T of clip b, [len(heads), nt, 1500], from the SAME (possibly bf16) operands"""
    qb = q[b, :nt].double().view(nt, -1, 64)
    return np.stack([(qb[:, h] @ k[b, h].double().T).numpy() for h in heads])


TOKENS = (2, 5, 17, 65)
FRAMES = (3, 4, 7, 58, 59, 64, 65, 70, 1499, 1500)  # 58 / 59: one and two tiles of this kernel; 64 / 65: one and two statistics chunks
# Two token rows meet the three frame counts around the filter's own thresholds only.  With two rows a z-score is +-1 in exact
# arithmetic and (w - mean) cancels: wherever the two rows' weights agree to a relative g, float32 leaves an error of 6e-8 / g, and
# among 70 or 1500 columns some pair always agrees closely.  The float32 CPU restatement itself is then off by 3e-6 .. 2e-2
# (measured over seeds), 16 x which is past the 1e-4 cap: such a clip measures float32 cancellation, not the kernel.  From five
# rows on the restatement stays within 3e-7 .. 4e-6 at every frame count.
CASES = [(2, f) for f in FRAMES[:3]] + [(t, f) for t in TOKENS[1:] for f in FRAMES]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("heads", [[2], [2, 0, 1]], ids=["1head", "3heads"])
def test_weights_kernel_against_the_float64_restatement(dtype, heads):
    """One launch holds every (n_tokens, n_frames) pair of CASES as a clip of its own.  Tolerance: 16 x the float32 CPU restatement's
    own largest deviation from the float64 one over the launch's clips (the restatement's error is set by the clips whose
    column std is smallest; a clip of two rows and three frames can come out exact on the CPU, which would leave no room at
    all for a correctly rounded GPU result one ulp away), and under 1e-4 in any case."""
    rng = np.random.default_rng(11 + len(heads))
    cases = CASES
    B, T = len(cases), max(TOKENS)
    q, k = _draw(rng, B, T, 3, dtype)
    got = _weights(q, k, heads, [c[0] for c in cases], [c[1] for c in cases])
    ref_dev, devs, min_std = 0.0, [], np.inf
    for b, (nt, nf) in enumerate(cases):
        s = _scores(q, k, b, heads, nt)
        want = AR.weights_chain(s, nf, np.float64) * len(heads)  # the kernel leaves the SUM over heads without a divisor
        want32 = AR.weights_chain(s.astype(np.float32), nf, np.float32).astype(np.float64) * len(heads)
        ref_dev = max(ref_dev, float(np.abs(want32 - want).max()))
        devs.append(float(np.abs(got[b, :nt, :nf] - want).max()))
        w = torch.softmax(torch.from_numpy(s[..., :nf]), dim=-1).numpy()
        min_std = min(min_std, float(w.std(axis=-2).min()))
        assert np.isfinite(got[b, :nt, :nf]).all()
        assert (got[b, nt:] == 0).all() and (got[b, :, nf:] == 0).all(), (nt, nf)  # nothing outside the clip's own range
    tol = 16 * ref_dev
    print(f"weights {dtype} heads {heads}: float32 restatement deviation {ref_dev:.3e}, tolerance {tol:.3e}, smallest column std {min_std:.3e}")
    for (nt, nf), dv in zip(cases, devs):
        print(f"  n_tokens {nt:3d} n_frames {nf:4d}: deviation {dv:.3e}")
    assert tol < CAP, tol
    assert max(devs) <= tol, (max(devs), tol)


def test_weights_kernel_full_window():
    """T = 448 rows, 1500 frames, one head: the largest LDS tile (112 KB) and every tile and chunk of a window"""
    rng = np.random.default_rng(5)
    q, k = _draw(rng, 1, 448, 1, torch.float32)
    got = _weights(q, k, [0], [448], [1500])[0]
    s = _scores(q, k, 0, [0], 448)
    want = AR.weights_chain(s, 1500, np.float64)
    ref_dev = float(np.abs(AR.weights_chain(s.astype(np.float32), 1500, np.float32) - want).max())
    dev = float(np.abs(got - want).max())
    print(f"weights 448 x 1500: float32 restatement deviation {ref_dev:.3e}, GPU deviation {dev:.3e}")
    assert 16 * ref_dev < CAP and dev <= 16 * ref_dev


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_clip_depends_on_nothing_but_itself(dtype):
    """the same clip alone and as row 1 of a three-row batch whose other rows have other sizes: bit-equal matrices; and the
    divisor of the last head is a plain division of the sum"""
    rng = np.random.default_rng(3)
    q, k = _draw(rng, 3, 65, 3, dtype)
    heads = [1, 2, 0]
    alone = _weights(q[1:2, :17], k[1:2], heads, [17], [70])
    batch = _weights(q, k, heads, [65, 17, 5], [1500, 70, 64])
    assert np.array_equal(alone[0], batch[1, :17])
    mean = _weights(q[1:2, :17], k[1:2], heads, [17], [70], divisor=3.0)
    assert np.array_equal(mean[0], alone[0] / np.float32(3.0))


# ---------------------------------------------------------------- the DTW kernel through the C ABI
def _dtw(mats, first_row=2):
    """mats: list of [N_b, M_b] float32 (or None for an empty clip) -> list of (text_indices, time_indices)"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    B = len(mats)
    n_rows = np.array([0 if m is None else m.shape[0] for m in mats], dtype=np.int32)
    n_cols = np.array([1 if m is None else m.shape[1] for m in mats], dtype=np.int32)
    rows_avail = first_row + int(n_rows.max())
    ld = int(n_cols.max())
    host = np.full((B, rows_avail, ld), np.nan, dtype=np.float32)  # a cell outside a clip's range poisons the path that reads it
    for b, m in enumerate(mats):
        if m is not None:
            host[b, first_row:first_row + m.shape[0], :m.shape[1]] = m
    ld_path = int((n_rows + n_cols).max())
    with on_stream() as s:
        dm = torch.from_numpy(host).cuda()
        dn, dc = torch.from_numpy(n_rows).cuda(), torch.from_numpy(n_cols).cuda()
        need = L.wipa_dtw_scratch_bytes(B, int(n_rows.max()))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        path = torch.full((2, B, ld_path), -7, dtype=torch.int32, device="cuda")
        plen = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        _lib.check(L.wipa_dtw_batch(ptr(dm), rows_avail * ld, ld, first_row, rows_avail, ptr(dn), ptr(dc), _i32p(n_rows), _i32p(n_cols), B,
                                    ptr(scratch), need, ptr(path[0]), ptr(path[1]), ld_path, ptr(plen), sptr(s)), "wipa_dtw_batch")
        ph, lh = path.cpu().numpy(), plen.cpu().numpy()
    return [(ph[0, b, :lh[b]], ph[1, b, :lh[b]]) for b in range(B)]


def test_dtw_paths_equal_the_float32_restatement():
    """every N x M of the issue's grid, random and tie-heavy, and two empty clips among them, in ONE launch: the paths are the
    restatement's exactly (the kernel negates the matrix itself; the restatement takes the negated one)"""
    rng = np.random.default_rng(17)
    mats = []
    for N in (1, 2, 63, 64, 65, 130, 448):
        for M in (1, 2, 64, 65, 1500):
            mats.append(rng.standard_normal((N, M)).astype(np.float32))
            mats.append((rng.integers(-2, 3, (N, M)) * 0.25).astype(np.float32))
    mats.insert(1, None)
    mats.insert(40, None)
    mats.append(np.full((9, 33), 0.5, dtype=np.float32))  # all equal: every comparison is a tie
    got = _dtw(mats)
    for b, m in enumerate(mats):
        ti, tj = got[b]
        if m is None:
            assert len(ti) == 0
            continue
        wi, wj, _, _ = AR.dtw_f32(-m)
        assert len(ti) == len(wi) <= m.shape[0] + m.shape[1] - 1, (b, m.shape, len(ti), len(wi))
        assert np.array_equal(ti, wi) and np.array_equal(tj, wj), (b, m.shape)


# ---------------------------------------------------------------- the model level
def _model(dims_o, W, dtype, **kw):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype, **kw)
    m.load_weights(W)
    return m


@pytest.fixture(scope="module")
def mels():
    clips = np.stack([R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0)])
    return torch.from_numpy(np.stack([R.log_mel_spectrogram(a) for a in clips]))


TEXT = [[1200 + 37 * i for i in range(12)], [3400 + 91 * i for i in range(7)]]  # token rows of different lengths
ROWS = [[*SOT_SEQ, SP.no_timestamps, *t, EOT] for t in TEXT]
N_FRAMES = [1500, 250]  # 30 s and 5 s of content


def _oracle(dims, W, mels):
    """(xa, logits [2, T, V], per-layer q.k^T) of the oracle's forward on the padded token rows"""
    T = max(len(r) for r in ROWS)
    tok = torch.full((2, T), EOT, dtype=torch.long)
    for b, r in enumerate(ROWS):
        tok[b, :len(r)] = torch.tensor(r)
    with torch.no_grad():
        xa = R.encoder_forward(W, dims, mels)
        logits, qks = AR.decoder_forward_qk(R, W, dims, tok, xa)
    return xa, logits, qks


@pytest.fixture(scope="module")
def micro_oracle(mels):
    W = R.synthetic_weights(MICRO, seed=7)
    return (W,) + _oracle(MICRO, W, mels)


def _check_model(m, xa, logits, qks, heads, label, prob_tol=None):
    """runs align_tokens and returns the largest matrix deviation from the float64 restatement on the oracle's scores"""
    from whisper_ipa_amd import timing

    first = len(SOT_SEQ)
    n_rows = [len(t) + 1 for t in TEXT]
    matrix, paths, probs = timing.align_tokens(m, ROWS, n_rows, first, EOT, xa, N_FRAMES)
    matrix = matrix.cpu().numpy()
    delta, checks = 0.0, []
    for b in range(2):
        nt, nf, N = len(ROWS[b]), N_FRAMES[b], n_rows[b]
        want = AR.alignment_matrix(qks, b, heads, nt, nf, np.float64)
        got = matrix[b, :nt, :nf]
        assert (matrix[b, nt:] == 0).all() and (matrix[b, :, nf:] == 0).all()
        delta = max(delta, float(np.abs(got - want).max()))
        checks.append((b, got, want, N, nf))
    for b, got, want, N, nf in checks:
        ti, tj = paths[b]
        wi, wj, _, _ = AR.dtw_f32(-got[first:first + N])  # the GPU's path is the CPU's DTW of the GPU's own matrix, exactly
        assert np.array_equal(ti, wi) and np.array_equal(tj, wj), (label, b)
        x = -want[first:first + N]
        excess = AR.path_cost(x, ti, tj) - AR.dtw_min_cost_f64(x)
        bound = 2 * (N + nf - 1) * delta  # a path has at most N + M - 1 cells, each off by at most delta on either matrix
        print(f"{label} clip {b}: path of {len(ti)} cells costs {excess:.3e} above the oracle optimum (bound {bound:.3e})")
        assert -1e-9 <= excess <= bound, (label, b, excess, bound)
        p_want = AR.token_probs(logits[b, :len(ROWS[b])].numpy(), TEXT[b], first, EOT)
        p_got = probs[b, first:first + len(TEXT[b])]
        dp = float(np.abs(p_got - p_want).max())
        rel = float((np.abs(p_got - p_want) / p_want).max())
        print(f"{label} clip {b}: token probabilities {p_want.min():.2e} .. {p_want.max():.2e}, largest relative deviation {rel:.3e}")
        print(f"{label} clip {b}: token probabilities within {dp:.3e}")
        assert (p_got > 0).all()
        if prob_tol is not None:  # relative: these probabilities are 1e-5 .. 1e-4, an absolute bound would pass any answer
            assert (np.abs(p_got - p_want) <= prob_tol * p_want).all(), (label, b, rel)
        assert (probs[b, first + len(TEXT[b]):] == 0).all()  # the row that predicts EOT and the padding carry no text token
    print(f"{label}: largest matrix deviation delta = {delta:.3e}")
    return delta


@pytest.mark.parametrize("which", ["default", "pairs"])
def test_model_alignment_micro_f32(micro_oracle, which):
    """f32 MICRO (128 wide, 2 heads, 2 layers), a 30 s and a 5 s clip, rows of 17 and 12 tokens; default heads = both heads of
    layer 1, ``pairs`` = [(0, 1), (1, 0)] (two layers, list order != layer order).  delta, the largest deviation of the matrix
    from the float64 restatement on the oracle's forward, was measured on an MI355X at 2.275e-5 (default) and 2.981e-5 (pairs)
    (DELTA_MICRO_F32); asserted: 4 x that, and <= 0.05.  Measured beside it: the path costs at most 1.3e-12 more than the optimum
    on the oracle's matrix (bounds 1.2e-2 .. 9.0e-2), token probabilities (3e-8 .. 7e-5) within 1.3e-5 of p.
    Token probabilities are asserted within 2.1e-3 of p, each: the project's 1e-3 logit tolerance gives |dp| <= p (e^(2 * 1e-3) - 1)."""
    W, xa, logits, qks = micro_oracle
    m = _model(MICRO, W, torch.float32)
    if which == "pairs":
        m.set_alignment_heads([(0, 1), (1, 0)])
    heads = m.alignment_heads
    assert heads == ([(1, 0), (1, 1)] if which == "default" else [(0, 1), (1, 0)])
    delta = _check_model(m, xa, logits, qks, heads, f"micro f32 {which}", prob_tol=2.1e-3)
    assert 4 * DELTA_MICRO_F32[which] <= MODEL_CAP
    assert delta <= 4 * DELTA_MICRO_F32[which], (delta, DELTA_MICRO_F32[which])


def test_model_alignment_logits_in_row_blocks(micro_oracle):
    """the final projection in blocks of 5 rows (34 rows: seven blocks, the last of 4) gives the probabilities of one block
    (MI355X: bit for bit; asserted within 2.1e-3 of p, as against the oracle)"""
    from whisper_ipa_amd import timing

    W, xa, _, _ = micro_oracle
    m = _model(MICRO, W, torch.float32)
    n_rows = [len(t) + 1 for t in TEXT]
    _, paths_a, probs_a = timing.align_tokens(m, ROWS, n_rows, len(SOT_SEQ), EOT, xa, N_FRAMES)
    _, paths_b, probs_b = timing.align_tokens(m, ROWS, n_rows, len(SOT_SEQ), EOT, xa, N_FRAMES, logits_rows=5)
    assert ((probs_b > 0) == (probs_a > 0)).all() and (probs_a > 0).sum() == sum(len(t) for t in TEXT)
    live = probs_a > 0
    rel = np.abs(probs_a[live] - probs_b[live]) / probs_a[live]
    print(f"row blocks: probabilities {probs_a[live].min():.2e} .. {probs_a[live].max():.2e}, largest relative difference {rel.max():.3e}")
    assert (rel <= 2.1e-3).all(), rel.max()  # a block read at the wrong row, or a probability of another token, is off by O(1) of p
    for (ti, tj), (ui, uj) in zip(paths_a, paths_b):
        assert np.array_equal(ti, ui) and np.array_equal(tj, uj)


def test_model_alignment_w384_bf16_after_an_absorbed_decode(mels):
    """bf16 W384 (the absorbed-eligible shape), decoded with the absorbed cross-attention first, then aligned: the teacher-forced
    pass projects its keys whatever form the decode step took.  delta against the f32 oracle is measured and printed (MI355X:
    3.048e-2; the path of the 30 s clip costs 5.9e-2 more than the optimum on the oracle's matrix, bound 92; token probabilities
    within 1.4e-7), asserted only against the 0.05 cap; the exact-path and cost-bound checks hold as
    for f32.  An fp8-quantised model is refused."""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import timing

    W = R.synthetic_weights(W384, seed=7)
    xa, logits, qks = _oracle(W384, W, mels)
    m = _model(W384, W, torch.bfloat16, cross_attention="absorbed")
    always, first = R.suppress_lists(SP)
    res = wipa.decoding.greedy_decode_tokens(m, xa.to(torch.bfloat16), [*SOT_SEQ, SP.no_timestamps], always, first, EOT, max_new_tokens=4,
                                             stop_on_eot=False)
    assert res.tokens.shape[0] == 2 and m.use_absorbed(2, 4)
    delta = _check_model(m, xa, logits, qks, m.alignment_heads, "w384 bf16")
    assert delta <= MODEL_CAP, delta
    m.quantize_weights("fp8_e4m3")
    with pytest.raises(NotImplementedError, match="fp8"):  # the public path, before anything is decoded
        wipa.transcribe(m, R.synthetic_clip(1, 5.0)[: 5 * 16000], language="en", word_timestamps=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        timing.align_tokens(m, ROWS, [len(t) + 1 for t in TEXT], len(SOT_SEQ), EOT, xa, N_FRAMES)


# ---------------------------------------------------------------- end to end
def test_transcribe_word_timestamps_end_to_end():
    """transcribe(word_timestamps=True) on a 40 s and a 10 s clip, scripted timestamp weights: every segment with text has words
    whose tokens are the segment's text tokens, times are ordered and inside the window, and the whole result equals
    add_word_timestamps applied here to the plain transcript with features computed from the windows' own samples."""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import timing
    from whisper_ipa_amd.tokenizer import get_tokenizer

    W = R.synthetic_weights(MICRO, seed=7)
    # the script of tests/timestamp_ref.py with text a tokenizer can cut into words: " a b" | " c" | " d e" in the byte vocabulary
    # (220 is the blank, 64.. the letters), closed by a single timestamp so that a window is consumed whole
    sp_, a_, b_, c_, d_, e_ = 220, 64, 65, 66, 67, 68
    plot = [TB + 0, sp_, a_, sp_, b_, TB + 100, TB + 100, sp_, c_, TB + 250, TB + 250, sp_, d_, sp_, e_, TB + 400, EOT]
    script = [EOT] * MICRO.n_text_ctx
    for pos, t in enumerate(plot):
        script[len(SOT_SEQ) - 1 + pos] = t
    W["decoder.positional_embedding"] = TR.scripted_positional_table(W, script)
    m = _model(MICRO, W, torch.float32)
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])
    short = R.synthetic_clip(1, 10.0)[: 10 * 16000]
    clips = [long, short]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=m.num_languages, language="en", task="transcribe")
        out = wipa.transcribe(m, clips, language="en", sample_len=20, fp16=False, word_timestamps=True)
        plain = wipa.transcribe(m, clips, language="en", sample_len=20, fp16=False)
    n_words = 0
    windows = {}  # (file, seek) -> the window's segments of the plain transcript, in order
    for i, (o, p) in enumerate(zip(out, plain)):
        assert [{k: v for k, v in s.items() if k != "words"} for s in o["segments"]] == p["segments"] and o["text"] == p["text"]
        for s, ps in zip(o["segments"], p["segments"]):
            windows.setdefault((i, s["seek"]), []).append(dict(ps))
            text_tokens = [t for t in s["tokens"] if t < EOT]
            assert "words" in s and (len(s["words"]) > 0) == (len(text_tokens) > 0)
            assert "".join(w["word"] for w in s["words"]) == s["text"]
            lo, size = s["seek"] / 100.0, min(3000, len(clips[i]) // 160 - s["seek"]) / 100.0
            prev = lo
            for w in s["words"]:
                assert lo <= w["start"] <= w["end"] <= lo + size + 1e-9 and w["start"] >= prev - 1e-9, (i, s["seek"], w)
                assert 0.0 <= w["probability"] <= 1.0
                prev = w["start"]
            n_words += len(s["words"])
        # the words of a window do not run backwards across its segments either
        for key in {k for k in windows if k[0] == i}:
            starts = [w["start"] for s in o["segments"] if s["seek"] == key[1] for w in s["words"]]
            assert starts == sorted(starts)
    assert n_words == 15 and [s["text"] for s in out[1]["segments"]] == [" a b", " c", " d e"]  # three windows of five words
    # the same words from a direct call: all windows of both files in one batch
    keys = sorted(windows)
    sizes = [min(3000, len(clips[i]) // 160 - seek) for i, seek in keys]
    win = np.zeros((len(keys), 480000), dtype=np.float32)
    for r, ((i, seek), size) in enumerate(zip(keys, sizes)):
        chunk = clips[i][seek * 160: seek * 160 + size * 160]
        win[r, :len(chunk)] = chunk
    feats = m.embed_audio(wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80))
    segs = [windows[k] for k in keys]
    timing.add_word_timestamps(segs, m, tok, feats, sizes, [seek / 100.0 for _, seek in keys])
    for (i, seek), ws in zip(keys, segs):
        got = [s["words"] for s in out[i]["segments"] if s["seek"] == seek]
        assert got == [s["words"] for s in ws], (i, seek)
    # the words' tokens concatenate to the segment's text tokens: through find_alignment itself, which keeps them
    text_tokens = [[t for s in ws for t in s["tokens"] if t < EOT] for ws in segs]
    for row, al in zip(text_tokens, timing.find_alignment(m, tok, text_tokens, feats, sizes)):
        assert [t for w in al for t in w.tokens] == row
        assert all(w.start <= w.end for w in al)


def test_align_known_transcripts():
    """whisper_ipa_amd.align: tokenise, log-mel, encoder, find_alignment -- the words of find_alignment on the same features,
    after merge_punctuations"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import timing
    from whisper_ipa_amd.tokenizer import get_tokenizer

    m = _model(MICRO, R.synthetic_weights(MICRO, seed=7), torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tok = get_tokenizer(True, num_languages=m.num_languages, language="en", task="transcribe")
    clips = [R.synthetic_clip(0, 30.0), R.synthetic_clip(1, 5.0)[: 5 * 16000]]
    texts = [" ðə kwɪk (bɹaʊn) fɑks.", " tʰɪs"]
    got = wipa.align(m, clips, texts, tokenizer=tok)
    win = np.zeros((2, 480000), dtype=np.float32)
    win[0], win[1, : len(clips[1])] = clips[0], clips[1]
    feats = m.embed_audio(wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80))
    want = timing.find_alignment(m, tok, [tok.encode(t) for t in texts], feats, [3000, 500])
    for g, w, text in zip(got, want, texts):
        timing.merge_punctuations(w)
        assert g == [x for x in w if x.word]
        assert "".join(x.word for x in g) == text and [t for x in g for t in x.tokens] == tok.encode(text)
        assert all(0.0 <= x.start <= x.end for x in g) and [x.start for x in g] == sorted(x.start for x in g)
    assert [x.word for x in got[0]] == [" ðə", " kwɪk", " (bɹaʊn)", " fɑks."]  # both punctuation passes
    assert got[1][-1].end <= 5.0 - 0.02 + 1e-9  # 5 s of content: 250 frames of 20 ms, the last one starts at 4.98 s
