"""The pipelined loop of the absorbed cross-attention's streaming kernel (transposed reads of the next column block in flight
behind the current block's MFMAs, softmax exchanges on the register file, the merge kernel built for the call's split count)
reads the same bytes and does the same arithmetic in the same order as the loop before it, which WIPA_ABS_LOOP=0 still selects.
The variable is read per call, so one process runs both: the partials (m, l, O'), the merged output and greedy token ids must
be the same BITS.  Shapes: both instantiated widths below 1024 with three waves (768: six column blocks, 384: three), B = 3, one
group / a ragged second group / fewer groups than waves / the real length, 1, 2 and 4 frame splits, a drift case that makes the
waves restart against their exact maximum, partial rows of the padded heads that nobody may read or write, and one full group
of 64 clips, where a last-bit difference in the merge has enough rows to show and most of xa streams with the nt policy."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
WIDTHS = ((768, 12), (384, 6))
FRAMES = (16, 17, 47, 1500)
SPLITS = (1, 2, 4)


class _Env:
    """a variable set (or removed: None) for the calls inside the block; the library reads it per call"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _parts(scratch, d, S, nb):
    """(m [nb][S][16], l [nb][S][16], o [nb][S][16][d]) out of a call's scratch, on the host"""
    q_bytes = nb * 16 * d * 2
    n = nb * S * 16
    f = scratch[q_bytes: q_bytes + n * (2 + d) * 4].view(torch.float32).cpu()
    return f[:n].view(nb, S, 16).clone(), f[n:2 * n].view(nb, S, 16).clone(), f[2 * n:].view(nb, S, 16, d).clone()


def _poison_parts(scratch, d, nb):
    scratch[nb * 16 * d * 2:] = 0xFF  # every float of the partials a NaN: what a launch does not write stays one


@pytest.fixture(scope="module")
def lib():
    from whisper_ipa_amd import _lib

    return _lib, _lib.lib()


def _attention(lib, variant, q, wkT, xa, wv, bv, d, H, Tk, splits, stages=None, nb=B):
    """one wipa_cross_absorbed_attention call, then the streaming launch alone once more on the poisoned partials; returns
    (out, m, l, o of the attention call, m, l, o of the lone streaming launch)"""
    from whisper_ipa_amd.runtime import ptr

    _lib, L = lib
    S = L.wipa_cross_absorbed_splits(splits, Tk)
    nbytes = L.wipa_cross_absorbed_scratch_bytes(nb, d, Tk)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    _poison_parts(scratch, d, nb)
    out = torch.full((nb, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    with _Env(WIPA_ABS_LOOP=variant, WIPA_ABS_STAGES=stages):
        if stages is not None:  # the caller's absorbed queries: they sit where the first stage would have put them
            scratch[: nb * 16 * d * 2] = q.contiguous().view(torch.uint8).flatten()
            qarg = wkT  # any valid bf16 pointer: the stage that reads it is off
        else:
            qarg = q
        _lib.check(L.wipa_cross_absorbed_attention(ptr(qarg), d, ptr(wkT), ptr(xa), ptr(wv), ptr(bv), ptr(out), d, ptr(scratch), nbytes,
                                                   nb, H, d, Tk, 64 ** -0.25, splits, None))
        torch.cuda.synchronize()
        first = _parts(scratch, d, S, nb)
        _poison_parts(scratch, d, nb)
        _lib.check(L.wipa_cross_absorbed_stream(ptr(xa), ptr(scratch), nbytes, nb, H, d, Tk, splits, None))
        torch.cuda.synchronize()
        lone = _parts(scratch, d, S, nb)
    return (out.cpu(),) + first + lone


def _assert_same(a, b, what):
    names = ("out", "part_m", "part_l", "part_o", "stream part_m", "stream part_l", "stream part_o")
    for n, x, y in zip(names, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, n)
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {n} differs between WIPA_ABS_LOOP=0 and the default"


def _check_padded_heads(res, H, what):
    out, m, l, o = res[:4]
    assert torch.isfinite(out.float()).all(), f"{what}: the merge read a partial row nobody wrote"
    assert torch.isfinite(m).all() and torch.isfinite(l).all() and torch.isfinite(o[:, :, :H]).all(), what
    # the rows of heads >= H are not written (still the NaN pattern they were poisoned with) ...
    assert (_bits(o[:, :, H:]) == -1).all(), f"{what}: the streaming kernel wrote a padded head's partial row"
    assert (_bits(res[6][:, :, H:]) == -1).all(), what
    # ... and not read: a finite output above, and the real rows do not depend on them (both launches of a variant agree)
    assert torch.equal(_bits(o[:, :, :H]), _bits(res[6][:, :, :H])), what


@pytest.mark.parametrize("d,H", WIDTHS)
def test_partials_and_output_are_bit_identical_to_the_loop_before(lib, d, H):
    _lib, L = lib
    _lib.check(L.wipa_cross_absorbed_init(d))
    g = torch.Generator().manual_seed(31 + d)
    q = (torch.randn(B, d, generator=g) * 0.3).bfloat16().cuda()
    wkT = (torch.randn(d, d, generator=g) * 0.05).bfloat16().cuda()
    wv = (torch.randn(d, d, generator=g) * 0.05).bfloat16().cuda()
    bv = (torch.randn(d, generator=g) * 0.1).cuda()
    seen = set()
    for Tk in FRAMES:
        xa = torch.randn(B, Tk, d, generator=g).bfloat16().cuda()
        for splits in SPLITS:
            S = L.wipa_cross_absorbed_splits(splits, Tk)
            what = f"d={d} Tk={Tk} splits={splits} (S={S})"
            old = _attention(lib, "0", q, wkT, xa, wv, bv, d, H, Tk, splits)
            new = _attention(lib, None, q, wkT, xa, wv, bv, d, H, Tk, splits)
            one = _attention(lib, "1", q, wkT, xa, wv, bv, d, H, Tk, splits)
            _assert_same(old, new, what)
            _assert_same(old, one, what + " WIPA_ABS_LOOP=1")
            _check_padded_heads(old, H, what + " loop=0")
            _check_padded_heads(new, H, what)
            assert new[0].float().abs().max() > 0 and new[2].min() > 0, what  # not vacuous: an output, positive softmax sums
            seen.add(S)
    assert seen == {1, 2, 4}  # the real length ran every split count; the short ones fall back to one split


@pytest.mark.parametrize("d,H", WIDTHS)
def test_drift_restart_is_bit_identical(lib, d, H):
    """Scores that climb by more than 40 after every wave's first group: the wave drops its accumulators, finds its exact maximum
    in a scores-only sweep (the exchanges of the maximum run there too) and streams again against it."""
    _lib, L = lib
    _lib.check(L.wipa_cross_absorbed_init(d))
    Tk = 1500
    g = torch.Generator().manual_seed(77 + d)
    xa = (torch.randn(B, Tk, d, generator=g) * 0.5).bfloat16()
    qp = (torch.randn(B, 16, d, generator=g) * 0.02).bfloat16()
    qp[:, H:] = 0  # padded heads: zero rows, as the prologue leaves them
    # channel 0 carries the climb: 0 in the first 48 frames (the three waves' first groups), then a ramp up to +96 per unit of Qp
    ramp = torch.zeros(Tk)
    ramp[48:] = torch.linspace(48.0, 96.0, Tk - 48)
    xa[:, :, 0] = ramp.bfloat16()
    qp[:, :H, 0] = 1.0
    scores = torch.einsum("bhc,btc->bht", qp.float(), xa.float())[:, :H]
    first, top = scores[:, :, :48].max(-1).values, scores.max(-1).values
    assert (top - first).min() > 45  # every head of every clip drifts, with room over the kernel's 40
    wv = (torch.randn(d, d, generator=g) * 0.05).bfloat16().cuda()
    bv = torch.zeros(d).cuda()
    xa_d, qp_d = xa.cuda(), qp.cuda()
    for splits in (1, 2):  # one split: every wave restarts; two: the first split restarts, the second starts high
        old = _attention(lib, "0", qp_d, wv, xa_d, wv, bv, d, H, Tk, splits, stages="6")
        new = _attention(lib, None, qp_d, wv, xa_d, wv, bv, d, H, Tk, splits, stages="6")
        _assert_same(old, new, f"drift d={d} splits={splits}")
        _check_padded_heads(new, H, f"drift d={d} splits={splits}")
        # the restart ran: split 0's reference is the exact maximum of its frames, not the first groups' (f32 sums of bf16
        # products in another order: 1e-3 relative is wide for them and 40 away from the first groups' maximum)
        S = L.wipa_cross_absorbed_splits(splits, Tk)
        n0 = 32 * ((((Tk + 31) // 32) + S - 1) // S)
        ref = scores[:, :, :n0].max(-1).values
        assert torch.allclose(new[1][:, 0, :H], ref, rtol=1e-3, atol=1e-3), (new[1][:, 0, :H] - ref).abs().max()


def test_a_full_clip_group_is_bit_identical(lib):
    """64 clips, the real length, 1 .. 4 splits: 49 152 merged outputs per launch, enough rows for a last-bit difference in the
    merge's sums to show (the merge built for two splits once paired its two products into a packed multiply and added them
    rounded, where the general form fuses: five outputs per launch differed, none at three clips); and enough clips for the
    residency rule to stream most groups with the nt policy, as the pipelined passes do."""
    _lib, L = lib
    d, H, Tk, nb = 768, 12, 1500, 64
    _lib.check(L.wipa_cross_absorbed_init(d))
    g = torch.Generator(device="cuda").manual_seed(5)
    q = (torch.randn(nb, d, device="cuda", generator=g) * 0.3).bfloat16()
    wkT = (torch.randn(d, d, device="cuda", generator=g) * 0.05).bfloat16()
    wv = (torch.randn(d, d, device="cuda", generator=g) * 0.05).bfloat16()
    bv = torch.randn(d, device="cuda", generator=g) * 0.1
    xa = torch.randn(nb, Tk, d, device="cuda", generator=g).bfloat16()
    for splits in (1, 2, 3, 4):
        old = _attention(lib, "0", q, wkT, xa, wv, bv, d, H, Tk, splits, nb=nb)
        new = _attention(lib, None, q, wkT, xa, wv, bv, d, H, Tk, splits, nb=nb)
        _assert_same(old, new, f"64 clips, splits={splits}")
        for part in ("2", "3"):  # the two parts of the change apart: the pipelined loop alone, the specialised merge alone
            _assert_same(old, _attention(lib, part, q, wkT, xa, wv, bv, d, H, Tk, splits, nb=nb), f"64 clips, splits={splits}, WIPA_ABS_LOOP={part}")
    assert L.wipa_cross_absorbed_resident_groups(nb, d, Tk, 2) < 2 * (((Tk + 31) // 32 + 1) // 2)  # most groups stream nt


def test_greedy_ids_are_identical(lib):
    """a short greedy decode (captured step graphs, prefill and steps) under both loop variants: same ids, same log-probabilities"""
    from oracle import whisper_ref as R
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    dims = R.ModelDimensions(80, 1500, 384, 6, 2, 51865, 448, 384, 6, 2)
    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.bfloat16, cross_attention="absorbed")
    m.load_weights(R.synthetic_weights(dims, seed=5))
    feats = torch.randn(B, 1500, 384, generator=torch.Generator().manual_seed(3)).bfloat16().cuda()
    sp = R.SpecialTokens.multilingual()
    always, first = R.suppress_lists(sp)
    runs = {}
    for variant in ("0", None):
        for splits in (2, 4):
            m.cross_splits = splits
            with _Env(WIPA_ABS_LOOP=variant):
                r = wipa.decoding.greedy_decode_tokens(m, feats, list(sp.sot_sequence_including_notimestamps(0)), always, first, sp.eot,
                                                       max_new_tokens=6, stop_on_eot=False)
            runs[(variant, splits)] = (torch.as_tensor(r.tokens).cpu().clone(), torch.as_tensor(r.sum_logprobs).float().cpu().clone())
    for splits in (2, 4):
        a, b = runs[("0", splits)], runs[(None, splits)]
        assert a[0].shape[0] == B and torch.equal(a[0], b[0]), f"ids differ at {splits} splits"
        assert torch.equal(_bits(a[1]), _bits(b[1])), f"summed log-probabilities differ at {splits} splits"
