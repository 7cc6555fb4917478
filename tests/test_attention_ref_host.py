"""CPU tests of tests/attention_ref.py: the conditions its inputs promise, every floor of a CPU restatement against the constant
committed in tests/test_gpu_attention_forward.py (floor <= constant, so an edit of a table cannot silently outgrow a bound), that
the per-row criterion sees every mutation it is for, and the gap in the older whole-tensor test that it closes.  No GPU."""
import pytest
import torch

import attention_ref as AR
import backward_ref as BR
import test_gpu_attention_forward as G


def _ids(c):
    return c.id


def test_case_tables_are_the_issues():
    assert {c.Tq for c in AR.FLASH_BF16_CASES} == {1, 33, 64, 65, 200, 256, 257, 300, 320, 520} and len(AR.FLASH_BF16_CASES) == 20
    assert {c.Tq for c in AR.FLASH_F32_CASES} == {1, 37, 64, 65, 128, 129, 200}
    assert {(c.dtype, c.variant, c.Tq, c.Tk, c.causal) for c in AR.ATTN_CASES} == (
        {("bf16", "valu", *s) for s in ((1, 1, False), (5, 69, True), (15, 64, False), (16, 65, True), (17, 17, True), (33, 200, False))} |
        {("f32", "valu", 3, 130, False), ("f32", "valu", 15, 15, True), ("f32", "tkdev", 32, 100, False)} |
        {("f32", "mfma", *s) for s in ((16, 16, True), (64, 65, False), (65, 129, True), (80, 200, False))})
    assert all(c.Tq < 16 for c in AR.ATTN_CASES if c.dtype == "f32" and c.variant == "valu")
    assert all(c.Tq >= 16 for c in AR.ATTN_CASES if c.variant in ("mfma", "tkdev"))
    assert {(c.dtype, c.Tq, c.starts) for c in AR.ATTN_RAGGED_CASES} == {
        (dt, T, st) for dt in ("bf16", "f32") for T, st in ((40, (0, 1, 15, 16, 17, 39)), (130, (0, 63, 64, 65, 100, 129)))}
    assert {c.Tk for c in AR.DECODE_CACHE_CASES if c.dtype == "bf16"} == {1, 8, 31, 32, 33, 127, 128, 129, 448}
    assert {c.Tk for c in AR.DECODE_CACHE_CASES if c.dtype == "f32"} == {1, 15, 16, 17, 63, 64, 65, 448}
    assert {c.Tk for c in AR.DECODE_CROSS_CASES} == {512, 513, 1500}
    for c in AR.DECODE_RAGGED_CASES:
        assert c.Tk == 200 and c.B == 9 and c.starts[:8] == (0, 1, 31, 32, 33, 127, 128, 199) and c.starts[8] > c.Tk - 1
        lo, hi = AR.key_range(c)
        assert int(lo[8, 0]) == int(hi[8, 0]) == 199  # the start above the query row sees the row's own key only
    assert all(c.B == 6 for c in AR.ATTN_RAGGED_CASES) and all(c.H == 3 for c in AR.ALL_CASES)
    assert all(c.B == 2 for c in AR.ALL_CASES if not c.starts) and max(c.Tk for c in AR.ALL_CASES) == 1500
    assert len({c.id for c in AR.ALL_CASES}) == len(AR.ALL_CASES)
    assert set(G.FLOOR) == {AR.floor_key(c, s) for c in AR.ALL_CASES for s in ((False, True) if c.family == "flash_f32" else (False,))}


def test_reference_equals_torch_softmax_in_float64():
    for case in (AR.Case("attn", "f32", 5, 12, True, "valu"), AR.Case("attn", "bf16", 7, 10, False, "valu"),
                 AR.Case("attn_ragged", "f32", 9, 9, True, "", (0, 3))):
        x, ref = AR.inputs(case, "flat"), AR.reference(case, "flat")
        assert bool((x["q"].to(AR.TORCH_DTYPE[case.dtype]).float() == x["q"]).all())  # the kernel's own values
        s = torch.einsum("bqhd,bkhd->bhqk", x["q"].double(), x["k"].double())
        i, j = torch.arange(case.Tq)[:, None], torch.arange(case.Tk)[None, :]
        ok = torch.ones(case.B, case.Tq, case.Tk, dtype=torch.bool)
        if case.causal:
            ok &= (j <= i + case.Tk - case.Tq)[None]
        if case.starts:
            ok &= j[None] >= torch.tensor(case.starts)[:, None, None]
        s = s.masked_fill(~ok[:, None], float("-inf"))
        live = ok.any(-1)
        assert torch.equal(live, x["live"])
        out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), x["v"].double())
        assert float((out - ref["out"])[live].abs().max()) < 1e-12
        assert float((torch.logsumexp(s, -1).permute(0, 2, 1) - ref["lse"].permute(0, 2, 1))[live].abs().max()) < 1e-12
        assert bool((ref["A"][live] >= ref["out"][live].abs().amax(-1)).all())


@pytest.mark.parametrize("case", AR.ALL_CASES, ids=_ids)
def test_inputs_keep_their_promises(case):
    """the witness weight, the coverage of the edge keys, finite live rows and A > 0, in every regime"""
    wit, uncovered = AR.witness_map(case)
    # all edge keys are witnessed; a one-row decode case has 3 queries per batch row and covers them in edge_keys' order
    assert not uncovered or case.Tq == 1, uncovered
    if case.Tq == 1:
        n_q = case.H * (1 if case.starts else case.B)
        for bs, _ in AR.required_edges(case):
            row = [e for b2, e in AR.required_edges(case) if b2 == bs]
            assert not any((bs, e) in uncovered for e in row[:min(n_q, len(row))]), (bs, row, uncovered)
    for regime in AR.REGIMES:
        x, ref = AR.inputs(case, regime), AR.reference(case, regime)
        live = x["live"]
        assert bool(live.any()) and all(bool(torch.isfinite(x[n]).all()) for n in "qkv")
        assert bool(torch.isfinite(ref["out"][live]).all()) and bool(torch.isfinite(ref["lse"].permute(0, 2, 1)[live]).all())
        assert bool((ref["A"][live] > 0).all())
    x = AR.inputs(case, "witness")
    p = AR.attend(AR.scores(x), AR.visible(x["lo"], x["hi"], case.Tk), x["v"])[3]
    w = torch.gather(p, 3, wit.clamp(min=0)[..., None])[..., 0]  # [B, H, Tq]
    many = (x["live"] & (x["hi"] > x["lo"]))[:, None, :].expand_as(w)  # a query with one visible key holds it whole
    if bool(many.any()):
        assert AR.WITNESS_RANGE[0] <= float(w[many].min()) and float(w[many].max()) <= AR.WITNESS_RANGE[1], (w[many].min(), w[many].max())
    if case.causal:  # even rows hold their diagonal key
        assert bool((wit[:, :, 0::2] == x["hi"][:, None, 0::2])[x["live"][:, None, 0::2].expand_as(wit[:, :, 0::2])].all())


def test_ramp_scores_rise_for_even_queries_fall_for_odd_ones_and_stay_below_zero_on_the_ramp():
    case = next(c for c in AR.FLASH_BF16_CASES if c.Tq == 300)
    x = AR.inputs(case, "ramp")
    ramp = torch.einsum("bqhd,bkhd->bhqk", x["q"][..., 62:].double(), x["k"][..., 62:].double())  # the two ramp dims alone
    assert float(ramp.max()) <= 0.0 and float(ramp.min()) >= -AR.RAMP_SPAN - 0.1
    d = ramp[..., 1:] - ramp[..., :-1]
    par = (torch.arange(case.B)[:, None, None] * case.H + torch.arange(case.H)[None, :, None] + torch.arange(case.Tq)[None, None, :]) % 2
    assert bool((d[par == 0] >= 0).all()) and bool((d[par == 1] <= 0).all())
    assert abs(float(ramp[0, 0, 0, -1] - ramp[0, 0, 0, 0]) - AR.RAMP_SPAN) < 0.1


def test_floors_lie_under_the_committed_constants():
    worst, worst_lse = {}, [0.0, 0.0, 0.0]
    for case in AR.ALL_CASES:
        for split in ((False, True) if case.family == "flash_f32" else (False,)):
            key = AR.floor_key(case, split)
            w = worst.setdefault(key, [0.0, 0.0, 0.0])
            for r, regime in enumerate(AR.REGIMES):
                f, f_lse = AR.floor(case, regime, split)
                w[r] = max(w[r], f)
                if case.family == "attn" and case.dtype == "f32":
                    worst_lse[r] = max(worst_lse[r], f_lse)
    for key, w in sorted(worst.items()):
        print(f"\nfloor {key} (witness, flat, ramp): " + ", ".join(f"{v:.2e}" for v in w))
    print("\nfloor lse (witness, flat, ramp): " + ", ".join(f"{v:.2e}" for v in worst_lse))
    for key, w in worst.items():
        for r in range(3):
            assert w[r] <= G.FLOOR[key][r], (key, AR.REGIMES[r], w[r], G.FLOOR[key][r])
            assert G.FLOOR[key][r] <= 1.5 * w[r], (key, AR.REGIMES[r], "the constant has drifted from its floor", w[r])
    for r in range(3):
        assert worst_lse[r] <= G.LSE_FLOOR[r] <= 1.5 * worst_lse[r], (AR.REGIMES[r], worst_lse[r])
    assert G.BF16_MARGIN == 3.0 and BR.ATTN_MARGIN == 8.0


@pytest.mark.parametrize("case", AR.ALL_CASES, ids=_ids)
def test_every_mutation_exceeds_three_bounds_in_some_regime(case):
    best = {}
    for regime in AR.REGIMES:
        x, ref = AR.inputs(case, regime), AR.reference(case, regime)
        for name, out in AR.mutations(case, regime).items():
            best[name] = max(best.get(name, 0.0), AR.worst_row(out, ref, x["live"]) / G.bound(case, regime))
    assert "v_head+1" in best and "clip+1" in best
    assert case.Tk == 1 or any(n.startswith("drop_key") for n in best)
    assert ("causal+1" in best) == (case.causal and case.Tq > 1) and ("start+1" in best) == bool(case.starts)
    print(f"\n{case.id}: " + "  ".join(f"{n} {v:.0f}x" for n, v in best.items()))
    for name, v in best.items():
        assert v >= 3.0, (case.id, name, v)


def test_flash_mutations_at_300_are_of_the_issues_order():
    """counting the padding keys: about 1e-2 in the flat regime and a few tenths on the ramp; a dropped last key: most of the row"""
    case = next(c for c in AR.FLASH_BF16_CASES if c.Tq == 300 and c.variant == "min")
    errs = {}
    for regime in AR.REGIMES:
        x, ref = AR.inputs(case, regime), AR.reference(case, regime)
        m = AR.mutations(case, regime)
        errs[regime] = (AR.worst_row(m["pad_denominator"], ref, x["live"]), AR.worst_row(m["drop_key[0..:299]"], ref, x["live"]))
    print("\nT = 300 (padded denominator, dropped last key):", {k: (f"{a:.2e}", f"{b:.2e}") for k, (a, b) in errs.items()})
    assert errs["flat"][0] > 2 * G.bound(case, "flat") and errs["ramp"][0] > 0.1 > 3 * G.bound(case, "ramp") and errs["witness"][1] > 0.5


@pytest.mark.parametrize("T", [1500, 200])
def test_padded_denominator_passes_the_whole_tensor_test_and_fails_the_per_row_criterion(T):
    """On the inputs of test_gpu_kernels.py::test_flash_attention_encoder_bf16 the bf16 flash arithmetic with the padding keys of
    the ragged last tile counted in l stays under that test's 1.5e-2 by max|got - ref| / max|ref|: it passes there.  At T = 200
    (56 padding keys) it lies over the per-row bound of every regime here while the unmutated arithmetic lies under it.  At
    T = 1500 these inputs cannot show the defect to any criterion: 36 zero-score keys against a denominator of about 1e5 (scores of
    standard deviation 2.9 over 1500 keys) move no row by more than the bf16 rounding of the output -- which is why the ramp
    regime keeps every score at or below zero, where the same 36 keys are a quarter of the denominator."""
    x = AR.old_flash_inputs(T)
    pad = torch.full((2, T), (T + 63) // 64 * 64 - T)
    clean, _ = AR.restate_inputs(x, "flash_bf16")
    mutant, _ = AR.restate_inputs(x, "flash_bf16", pad=pad)
    out, lse, A, _ = AR.attend(AR.scores(x), AR.visible(x["lo"], x["hi"], T), x["v"])
    ref = {"out": out, "lse": lse, "A": A}
    old_ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(AR.scores(x, torch.float32), -1), x["v"])  # the old test's statement
    old_rel = float((mutant - old_ref).abs().max() / old_ref.abs().max())
    case = AR.FLASH_BF16_CASES[0]
    new_bound = max(G.bound(case, r) for r in AR.REGIMES)
    e_clean, e_mut = AR.worst_row(clean, ref, x["live"]), AR.worst_row(mutant, ref, x["live"])
    print(f"\nT = {T}: padded denominator  old _rel {old_rel:.2e} (tolerance 1.5e-2)  per row {e_mut:.2e}, clean {e_clean:.2e} (bound {new_bound:.2e})")
    assert old_rel < 1.5e-2
    assert e_clean <= new_bound
    if T == 200:
        assert e_mut > new_bound
    else:
        assert e_mut < new_bound  # invisible on these inputs at this length; see the docstring
