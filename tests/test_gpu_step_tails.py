"""GPU: every fused decode-step tail of csrc/elementwise.hip (greedy_tail_kernel, timestamp_tail_kernel, sample_tail_kernel and their
RAGGED instantiations, behind wipa_greedy_step_embed / wipa_timestamp_step_embed / wipa_sample_step_embed / wipa_step_embed_ragged /
wipa_greedy_step_embed_partials) is BIT FOR BIT the unfused composition on the same inputs:

    the matching step entry point (wipa_greedy_step / wipa_timestamp_step / wipa_sample_step / wipa_sample_step_ragged),
    a host-side position advance,
    wipa_embed_layernorm / wipa_embed_layernorm_ragged.

The step kernels of the composition are themselves held to the numpy references by test_gpu_timestamps.py and test_gpu_sampling.py.
Shapes: B = 5 (several workgroups for the last-arrival counter, no power of two), V = 4099 (V mod 4 = 3: the trailing elements;
timestamp_begin below V, the last columns are timestamps), D = 1028 (the second 1024-column chunk of the row routine partly filled)
and D = 64, n_ctx = 16 with one scene at the last column (the min(p + 1, n_ctx - 1) clamp).  ``pytest -m gpu`` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, V, LDL, N_CTX, LD_TOK, N_INIT = 5, 4099, 4104, 16, 20, 3
TB, NT, EOT, MAX_INIT = 4000, 3995, 3990, 50
T = TB
# scenes: (column of the step, the rows' histories tokens[N_INIT .. p]); every row of a launch is at the same column
SCENES = {
    # empty history: the first sampled position -- mask_first, and under rules rule 4 with max_initial_timestamp_index
    "first": (N_INIT - 1, [[], [], [], [], []]),
    # text | a single timestamp | a closed pair | latched on eot | text after a pair's end
    "two": (N_INIT + 1, [[1200, 2400], [1200, T + 5], [T + 5, T + 5], [1200, EOT], [T + 3, 1200]]),
    # the last column of the context: the next position-embedding row is clamped to n_ctx - 1
    "last": (N_CTX - 1, [[T + 0, 7, 8, T + 9, T + 9, 11, 12, 13, 14, 15, 16, 17, 18],
                         [T + 0, 7, 8, T + 9, T + 9, 11, 12, 13, 14, 15, 16, 17, T + 30],
                         [T + 0, 7, 8, T + 9, T + 9, 11, 12, 13, 14, 15, 16, T + 30, T + 30],
                         [T + 0, 7, 8, T + 9, T + 9, 11, 12, 13, 14, 15, 16, EOT, EOT],
                         [T + 70, T + 70, 8, T + 9, T + 9, 11, 12, 13, 14, 15, 16, 17, 18]]),
}
STARTS = [0, 2, 0, 1, 0]  # rows 1 and 3 are left-padded: their own tokens start above column 0


@pytest.fixture(scope="module")
def inputs():
    """made once, shared, never written by a test"""
    g = torch.Generator().manual_seed(1234)
    out = {"logits": torch.zeros(B, LDL)}
    out["logits"][:, :V] = torch.randn(B, V, generator=g) * 2
    mask_always = torch.zeros(LDL)
    mask_always[[15, 16, 2000, V - 2]] = float("-inf")
    mask_first = mask_always.clone()
    mask_first[[EOT, 220]] = float("-inf")
    out["mask_first"], out["mask_always"] = mask_first, mask_always
    for D in (1028, 64):
        out[D] = dict(emb=torch.randn(V, D, generator=g) * 0.05, pos_emb=torch.randn(N_CTX, D, generator=g) * 0.02,
                      ln_w=1 + 0.1 * torch.randn(D, generator=g), ln_b=0.1 * torch.randn(D, generator=g))
    return {k: ({n: t.cuda() for n, t in v.items()} if isinstance(v, dict) else v.cuda()) for k, v in out.items()}


def _record(seed, attempt, temperature, nrows):
    from whisper_ipa_amd import _lib

    L = _lib.lib()
    n = L.wipa_sample_record_bytes(nrows)
    host = np.zeros(n, dtype=np.uint8)
    flat = (C.c_uint32 * (2 * nrows))(*[v for i in range(nrows) for v in (100 + 3 * i, i % 2)])
    _lib.check(L.wipa_sample_record_fill(host.ctypes.data, n, seed, attempt, temperature, flat, nrows), "record_fill")
    return torch.from_numpy(host).cuda()


def _run(inp, fused, p, tokens0, n_init, rules, sample, starts, y_dtype, D):
    """one step on fresh state: the fused tail, or step entry point + host position advance + embed_layernorm"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    w = inp[D]
    with on_stream() as s:
        tokens = tokens0.cuda()
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        posd = torch.tensor([p * D], dtype=torch.int64, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        slp = torch.linspace(-3.0, -1.0, B, device="cuda")
        nd = torch.full((1,), 2, dtype=torch.int32, device="cuda")
        x = torch.full((B, D), 9.0, device="cuda")
        y = torch.full((B, D), 9.0, device="cuda", dtype=y_dtype)
        rec = _record(77, 2, 0.7, B) if sample else None
        st = torch.tensor(STARTS, dtype=torch.int32, device="cuda") if starts else None
        r = C.byref(_lib.DecodeRules(TB, NT, MAX_INIT)) if rules else None
        yd = _lib.WIPA_F32 if y_dtype == torch.float32 else _lib.WIPA_BF16
        lg, mf, ma = ptr(inp["logits"]), ptr(inp["mask_first"]), ptr(inp["mask_always"])
        head = (lg, LDL, B, V, mf, ma, ptr(tokens), LD_TOK)
        emb = (ptr(w["emb"]), _lib.WIPA_F32, None, ptr(w["pos_emb"]), N_CTX, ptr(x), ptr(w["ln_w"]), ptr(w["ln_b"]), ptr(y), yd, D, 1e-5, sptr(s))
        if fused:
            state = (ptr(pos), ptr(posd), ptr(done), n_init, EOT)
            if starts:
                rc = L.wipa_step_embed_ragged(*head, *state, r, ptr(rec), ptr(st), ptr(slp), ptr(nd), *emb)
            elif sample:
                rc = L.wipa_sample_step_embed(*head, *state, r, ptr(rec), ptr(slp), ptr(nd), *emb)
            elif rules:
                rc = L.wipa_timestamp_step_embed(*head, *state, r, ptr(slp), ptr(nd), *emb)
            else:
                rc = L.wipa_greedy_step_embed(*head, *state, ptr(slp), ptr(nd), *emb)
            _lib.check(rc, "fused tail")
        else:
            if sample and starts:
                rc = L.wipa_sample_step_ragged(*head, ptr(pos), n_init, EOT, r, ptr(rec), ptr(st), ptr(slp), ptr(nd), sptr(s))
            elif sample:
                rc = L.wipa_sample_step(*head, ptr(pos), n_init, EOT, r, ptr(rec), ptr(slp), ptr(nd), sptr(s))
            elif rules:
                rc = L.wipa_timestamp_step(*head, ptr(pos), n_init, EOT, r, ptr(slp), ptr(nd), sptr(s))
            else:
                rc = L.wipa_greedy_step(*head, ptr(pos), n_init, EOT, ptr(slp), ptr(nd), sptr(s))
            _lib.check(rc, "step")
            pos += 1
            posd.fill_((p + 1) * D)
            if starts:
                rc = L.wipa_embed_layernorm_ragged(ptr(tokens), LD_TOK, B, ptr(pos), ptr(st), *emb)
            else:
                rc = L.wipa_embed_layernorm(ptr(tokens), LD_TOK, B, ptr(pos), *emb)
            _lib.check(rc, "embed_layernorm")
    torch.cuda.synchronize()
    return dict(tokens=tokens.cpu(), sum_logprobs=slp.cpu(), not_done=nd.cpu(), x=x.cpu(), y=y.cpu(), pos=pos.cpu(), posd=posd.cpu(),
                done=done.cpu())


def _tokens(hist, n_init=N_INIT):
    tk = torch.full((B, LD_TOK), 1, dtype=torch.int32)
    for b, h in enumerate(hist):
        tk[b, n_init:n_init + len(h)] = torch.tensor(h, dtype=torch.int32)
    return tk


def _same(got, ref, what):
    for k in ("tokens", "sum_logprobs", "not_done", "x", "y", "pos", "posd"):
        assert torch.equal(got[k], ref[k]), (what, k, got[k], ref[k])
    assert int(got["done"]) == 0, what


def _check_scenes(inp, rules, sample, starts, y_dtype, D):
    for name, (p, hist) in SCENES.items():
        tk = _tokens(hist)
        ref = _run(inp, False, p, tk, N_INIT, rules, sample, starts, y_dtype, D)
        got = _run(inp, True, p, tk, N_INIT, rules, sample, starts, y_dtype, D)
        _same(got, ref, name)
        # the composition did something: the column after p is written, the position moved, rows x / y are filled
        assert int(got["pos"]) == p + 1 and int(got["posd"]) == (p + 1) * D
        assert bool((got["x"] != 9.0).any(1).all()) and bool((got["y"].float() != 9.0).any(1).all())
        if name != "first":  # row 3's previous token is eot: eot again, no log-prob added
            assert int(got["tokens"][3, p + 1]) == EOT and float(got["sum_logprobs"][3]) == float(torch.linspace(-3.0, -1.0, B)[3])
            if rules:  # row 1 ends in a single timestamp: eot or a timestamp next; row 2 in a closed pair: text next
                assert int(got["tokens"][1, p + 1]) >= EOT and int(got["tokens"][2, p + 1]) < TB
        elif rules:  # rule 4: a timestamp no later than max_initial_timestamp_index
            assert bool(((got["tokens"][:, p + 1] >= TB) & (got["tokens"][:, p + 1] <= TB + MAX_INIT)).all())


@pytest.mark.parametrize("y_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("starts", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("sample", [False, True], ids=["argmax", "sample"])
@pytest.mark.parametrize("rules", [False, True], ids=["plain", "rules"])
def test_fused_tail_is_the_unfused_composition(inputs, rules, sample, starts, y_dtype):
    _check_scenes(inputs, rules, sample, starts, y_dtype, 1028)


def test_fused_tail_is_the_unfused_composition_at_d64(inputs):
    """one 256-thread pass of the row routine with most threads idle"""
    _check_scenes(inputs, True, True, True, torch.bfloat16, 64)


@pytest.mark.parametrize("starts", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("sample", [False, True], ids=["argmax", "sample"])
@pytest.mark.parametrize("rules", [False, True], ids=["plain", "rules"])
def test_prompt_walk_copies_the_token_in_place(inputs, rules, sample, starts):
    """pos + 1 < n_init: the tail leaves the token, sum_logprobs and not_done alone, and still embeds and advances"""
    n_init, p, D = 6, 2, 1028
    tk = _tokens([[1200, 2400]] * B, n_init)
    tk[:, :n_init] = torch.tensor([[50, 51, 52, 53 + b, 54, 55] for b in range(B)], dtype=torch.int32)
    ref = _run(inputs, False, p, tk, n_init, rules, sample, starts, torch.float32, D)
    got = _run(inputs, True, p, tk, n_init, rules, sample, starts, torch.float32, D)
    _same(got, ref, "prompt walk")
    assert torch.equal(got["tokens"], tk)
    assert torch.equal(got["sum_logprobs"], torch.linspace(-3.0, -1.0, B)) and int(got["not_done"]) == 2
    assert int(got["pos"]) == p + 1 and int(got["posd"]) == (p + 1) * D
    # the embedded token is the prompt's own: row b holds emb[53 + b] + pos_emb[3 - start[b]]
    for b in range(B):
        want = inputs[D]["emb"][53 + b] + inputs[D]["pos_emb"][p + 1 - (STARTS[b] if starts else 0)]
        assert torch.equal(got["x"][b], want.cpu()), b


def test_partials_tail_against_the_row_scanning_tail():
    """wipa_greedy_step_embed_partials on wipa_logits_greedy's per-wave partials against wipa_greedy_step_embed on the logits the
    same launch wrote (modelled on test_logits_projection_with_greedy_partials, at B = 5).  Everything is bit-identical but
    sum_logprobs: the partials path sums exp per wave of the GEMM's grid and rescales, the row scan sums per thread of the tail --
    two groupings of one f32 sum, held to the 1e-6 of the test this one is modelled on (an ulp or two of a log-prob)."""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    Vp, d, n_ctx, n_init, eot, ld_tok = 8203, 384, 16, 3, 7, 20
    ldl = (Vp + 7) // 8 * 8
    assert L.wipa_logits_greedy_supported(B, Vp, d, _lib.WIPA_BF16) == 1
    g = torch.Generator(device="cuda").manual_seed(B + d)
    rn = lambda *sh, s=1.0: torch.randn(*sh, device="cuda", generator=g) * s
    W, xin = rn(Vp, d, s=0.05).bfloat16(), rn(B, d).bfloat16()
    W[Vp - 1] = W[100]  # a tie across tiles: the lower column wins wherever it is the maximum
    mask_always = torch.zeros(ldl, device="cuda")
    mask_always[torch.randperm(Vp, device="cuda", generator=g)[:50]] = float("-inf")
    mask_first = mask_always.clone()
    mask_first[:64] = float("-inf")
    pos_emb, ln_w, ln_b = rn(n_ctx, d, s=0.02), 1 + 0.1 * rn(d), 0.1 * rn(d)

    def run(partials, p0):
        tokens = torch.full((B, ld_tok), 1, dtype=torch.int32, device="cuda")
        tokens[2, p0] = eot  # latched
        pos = torch.tensor([p0], dtype=torch.int32, device="cuda")
        posd = torch.zeros(1, dtype=torch.int64, device="cuda")
        done = torch.zeros(1, dtype=torch.int32, device="cuda")
        slp = torch.linspace(-3.0, -1.0, B, device="cuda")
        nd = torch.full((1,), 2, dtype=torch.int32, device="cuda")
        logits = torch.zeros(B, ldl, device="cuda")
        xo, yo = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
        nb = L.wipa_logits_greedy_partials_bytes(B)
        part = torch.empty(nb, dtype=torch.uint8, device="cuda")
        tail = (ptr(tokens), ld_tok, ptr(pos), ptr(posd), ptr(done), n_init, eot, ptr(slp), ptr(nd), ptr(W), _lib.WIPA_BF16, None, ptr(pos_emb),
                n_ctx, ptr(xo), ptr(ln_w), ptr(ln_b), ptr(yo), _lib.WIPA_BF16, d, 1e-5)
        with on_stream() as s:
            _lib.check(L.wipa_logits_greedy(ptr(xin), d, ptr(W), d, ptr(logits), ldl, B, Vp, d, ptr(mask_first), ptr(mask_always), ptr(pos), n_init,
                                            ptr(part), nb, sptr(s)), "wipa_logits_greedy")
            if partials:
                _lib.check(L.wipa_greedy_step_embed_partials(ptr(part), _lib.GREEDY_PARTS, B, *tail, sptr(s)), "partials tail")
            else:
                _lib.check(L.wipa_greedy_step_embed(ptr(logits), ldl, B, Vp, ptr(mask_first), ptr(mask_always), *tail, sptr(s)), "logits tail")
        torch.cuda.synchronize()
        return dict(tokens=tokens.cpu(), sum_logprobs=slp.cpu(), not_done=nd.cpu(), x=xo.cpu(), y=yo.cpu(), pos=pos.cpu(), posd=posd.cpu(),
                    done=done.cpu())

    for p0 in (n_init - 1, n_init + 3, n_ctx - 1):  # mask_first, mask_always, the clamp at the last column
        ref, got = run(False, p0), run(True, p0)
        for k in ("tokens", "not_done", "x", "y", "pos", "posd"):
            assert torch.equal(got[k], ref[k]), (p0, k)
        print(f"p0 {p0}: max |sum_logprobs difference| {float((got['sum_logprobs'] - ref['sum_logprobs']).abs().max()):.2e}")
        assert torch.allclose(got["sum_logprobs"], ref["sum_logprobs"], rtol=1e-6, atol=1e-6), p0
        assert int(got["done"]) == 0 and int(got["pos"]) == p0 + 1
        assert int(got["tokens"][2, p0 + 1]) == eot and float(got["sum_logprobs"][2]) == float(ref["sum_logprobs"][2]) == -2.0
