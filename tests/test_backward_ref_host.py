"""CPU tests of tests/backward_ref.py: every float64 reference against torch.autograd in float64, and every float32 floor,
on every case of the GPU tables, against the bound committed in tests/test_gpu_backward_kernels.py: floor < bound / margin, so
an edit of a table cannot silently outgrow a constant.  No GPU."""
import numpy as np
import pytest
import torch

import backward_ref as BR
import test_gpu_backward_kernels as G

TOL64 = 1e-12


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("causal,Tq,Tk,scale", [(True, 9, 9, 1.0), (True, 5, 12, 0.37), (False, 7, 10, 64 ** -0.25)])
def test_attention_reference_equals_float64_autograd(causal, Tq, Tk, scale):
    """dq / dk are gradients of the UNSCALED projections: the forward sees q = scale q_raw, k = scale k_raw"""
    g = torch.Generator().manual_seed(Tq)
    B, H = BR.ATTN_B, BR.ATTN_H
    q_raw, k_raw = (torch.randn(B, T, H, 64, generator=g, dtype=torch.float64).requires_grad_(True) for T in (Tq, Tk))
    v = torch.randn(B, Tk, H, 64, generator=g, dtype=torch.float64).requires_grad_(True)
    d_out = torch.randn(B, Tq, H, 64, generator=g, dtype=torch.float64)
    s = torch.einsum("bqhd,bkhd->bhqk", q_raw * scale, k_raw * scale)
    if causal:
        s = s + torch.triu(torch.full((Tk, Tk), float("-inf"), dtype=torch.float64), 1)[Tk - Tq:]
    out_t = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)
    out_t.backward(d_out)
    q, k = (q_raw * scale).detach(), (k_raw * scale).detach()
    out, lse = BR.attn_forward(q, k, v.detach(), causal)
    dq, dk, dv, dvec = BR.attn_backward(q, k, v.detach(), out, lse, d_out, causal, scale)
    assert _rel(out, out_t.detach()) < TOL64 and _rel(lse, torch.logsumexp(s.detach(), -1)) < TOL64
    assert _rel(dq, q_raw.grad) < TOL64 and _rel(dk, k_raw.grad) < TOL64 and _rel(dv, v.grad) < TOL64
    assert _rel(dvec, (d_out * out_t.detach()).sum(-1).permute(0, 2, 1)) < TOL64


def test_attention_table_is_the_issues():
    shapes = {(c.causal, c.Tq, c.Tk) for c in BR.ATTN_CASES}
    assert shapes == {(True, 21, 21), (True, 64, 64), (True, 65, 65), (True, 130, 130), (True, 100, 164), (True, 33, 70),
                      (False, 13, 150), (False, 64, 128), (False, 70, 200), (False, 16, 220), (False, 129, 65)}
    for lay in "ab":  # each layout meets a causal and a non-causal case
        assert {c.causal for c in BR.ATTN_CASES if c.layout == lay} == {True, False}
    assert {c.qk_scale for c in BR.ATTN_CASES} == set(BR.QK_SCALES)
    assert len(BR.ATTN_CHAIN_CASES) == 3 and any(c.Tq == 13 for c in BR.ATTN_CHAIN_CASES)
    for c in BR.ATTN_CASES:  # the strides differ where the issue says so, and every one keeps 16-byte alignment
        lay = BR.attn_layout(c)
        assert all(s.rs % 4 == 0 and s.bs % 4 == 0 and s.off % 4 == 0 for s in lay.values())
        if c.layout == "b":
            assert len({lay[n].rs for n in "qkvo"}) == 4 and len({lay[n].bs for n in "qkvo"}) == 4


def test_attention_floors_lie_under_the_committed_bounds():
    worst = {}
    for case in BR.ATTN_CASES:
        f = BR.attn_floor32(case)
        if case in BR.ATTN_CHAIN_CASES:
            f.update(BR.attn_forward_floor32(case))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\nattention float32 floors:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= G.ATTN_CHAIN_BOUND[k] / BR.ATTN_MARGIN, (k, v)
    assert all(G.ATTN_BOUND[k] == G.ATTN_CHAIN_BOUND[k] for k in G.ATTN_BOUND)


def test_a_dropped_key_in_the_flattest_head_breaks_the_bound():
    """what the bound must see: key 63 (a tile edge) dropped from head 0 of the 70 x 200 case"""
    case = next(c for c in BR.ATTN_CASES if (c.Tq, c.Tk) == (70, 200))
    x, out32, lse32, ref = BR.attn_reference(case)
    k2, v2 = x["k"].clone(), x["v"].clone()
    q2 = x["q"].clone()
    k2[:, 63, 0] = -1e3 * torch.sign(q2[:, :, 0].sum(1))  # score far below every other: the key drops out of every row
    dq, dk, dv, dvec = BR.attn_backward(q2, k2, v2, out32, lse32, x["d_out"], case.causal, case.qk_scale)
    errs = BR.attn_slice_errors({"dq": dq}, ref)
    assert errs["dq"] > 10 * G.ATTN_BOUND["dq"], errs


@pytest.mark.parametrize("rows,D", [(3, 64), (9, 132)])
def test_layernorm_reference_equals_float64_autograd(rows, D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(rows, D, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(D, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(rows, D, generator=g, dtype=torch.float64)
    torch.nn.functional.layer_norm(x, (D,), w, b, BR.LN_EPS).backward(dy)
    r = BR.ln_backward(x.detach(), w.detach(), dy)
    assert _rel(r["dx"], x.grad) < TOL64 and _rel(r["dw"], w.grad) < TOL64 and _rel(r["db"], b.grad) < TOL64
    assert _rel(r["mean"], x.detach().mean(-1)) < TOL64
    assert _rel(r["rstd"], 1 / torch.sqrt(x.detach().var(-1, unbiased=False) + BR.LN_EPS)) < TOL64


def test_layernorm_floors_lie_under_the_committed_bounds():
    for fams, bound in (((0, 1), G.LN_BOUND), ((2,), G.LN_OFFSET_BOUND)):
        worst = dict.fromkeys(BR.LN_OUTPUTS, 0.0)
        for rows, D in BR.LN_CASES:
            for fam in fams:
                for k, v in BR.ln_floor32(rows, D, fam).items():
                    worst[k] = max(worst[k], v)
        print(f"\nlayernorm float32 floors, families {fams}:", {k: f"{v:.2e}" for k, v in worst.items()})
        for k, v in worst.items():
            assert v <= bound[k] / BR.LN_MARGIN, (fams, k, v)


def test_masked_ce_reference_equals_float64_autograd_and_floors():
    mask = torch.tensor(BR.CE_MASK, dtype=torch.float64)
    for V in BR.CE_VS:
        logits, tgt = BR.ce_inputs(V)
        assert 0 in tgt and V - 1 in tgt
        for count in BR.CE_COUNTS:
            lg = logits.double().requires_grad_(True)
            ce = torch.nn.functional.cross_entropy(lg, tgt, reduction="none")
            ((ce * mask).sum() / max(count, 1.0)).backward()
            ref = BR.ce_backward(logits, tgt, mask, count)
            assert float((ref - lg.grad).abs().max()) < TOL64
        f = BR.ce_floor32(V)
        assert f <= G.CE_BOUND / BR.CE_MARGIN, (V, f)
    # the chained case: float32 torch on the CPU against float64
    s32, n, g32, _ = BR.ce_chain_reference(torch.float32)
    s64, n64, g64, mask_c = BR.ce_chain_reference()
    assert n == n64 == 9.0 and mask_c.view(3, 5).tolist() == [[True] * 5, [True] + [False] * 4, [True] * 3 + [False] * 2]
    assert float((g32.double() - g64).abs().max()) * n <= G.CE_BOUND / BR.CE_MARGIN
    assert abs(float(s32) - float(s64)) / float(s64) <= G.CE_SUM_BOUND / BR.CE_MARGIN


@pytest.mark.parametrize("B,T,D", BR.EMB_CASES)
def test_embedding_sequential_loop_equals_float64_autograd(B, T, D):
    tok, dx, d_tok0 = BR.embed_inputs(B, T, D)
    E = torch.zeros(BR.EMB_VOCAB, D, dtype=torch.float64, requires_grad=True)
    P = torch.zeros(T, D, dtype=torch.float64, requires_grad=True)
    (E[tok.long()] + P[None]).reshape(B * T, D).backward(dx.double())
    d_tok, d_pos = BR.embed_backward_sequential(tok, dx, d_tok0)
    # float32 sums of at most B*T terms of |x| < 6 against float64
    assert np.abs(d_tok - (d_tok0.double() + E.grad).numpy()).max() < 1e-5 and np.abs(d_pos - P.grad.numpy()).max() < 1e-5


def test_colsum_chunk_rule_and_path_length():
    assert BR.colsum_chunks(511, 64, 1 << 20) == 1 and BR.colsum_chunks(512, 64, 1 << 20) == 2
    assert BR.colsum_chunks(512, 64, 127) == 1 and BR.colsum_chunks(16385, 133, 64 * 133) == 64
    assert BR.colsum_chunks(16385, 133, 64 * 133 - 1) == 63 and BR.colsum_chunks(16385, 133, 0) == 1
    assert BR.colsum_path_adds(1, 1, 0) == 1 + 12 and BR.colsum_path_adds(16385, 64, 1) == 9 + 12 + 64 + 1
    # the integer inputs stay exact in float32 whatever the order
    assert 8 * (BR.COLSUM_MAX_ROWS + 1) < 2 ** 24


def test_gelu_reference_and_the_series_floor():
    z = BR.gelu_points()
    assert z.numel() == 4104 and float(z[4]) == -12.0 and float(z[4099]) == 12.0
    zz = z.double().requires_grad_(True)
    u_t = torch.nn.functional.gelu(zz)
    u_t.sum().backward()
    u, d = BR.gelu64(z)
    assert float((u - u_t.detach()).abs().max()) < TOL64 and float((d - zz.grad).abs().max()) < TOL64
    u32, d32 = BR.gelu_series32(z)
    e_u = float(np.max(np.abs(u32 - u.numpy()) / np.maximum(np.abs(z.numpy()), 1.0)))
    e_d = float(np.max(np.abs(d32 - d.numpy())))
    print(f"\nfloat32 A-S 7.1.26 series on the CPU: gelu {e_u:.2e} max(|z|, 1), gelu' {e_d:.2e}")
    assert e_u <= 1.8e-7 and e_d <= 2.6e-7
    assert G.GELU_BOUND == 7e-7 and G.GELU_GRAD_BOUND == 1e-6
