"""GPU tests of encoder fine-tuning (DecoderTrainer(train_encoder_layers=...)): the conv-stem backward and the attention backward
at encoder shapes against the float64 restatements of tests/encoder_bwd_ref.py, every gradient of a step from the mel against
torch.autograd through the CPU oracle's encoder and decoder, one whole train_step, the refusals and data parallelism.

Every bound is a constant of tests/encoder_bwd_ref.py: the margin of its section times the float32 CPU floor that
tests/test_encoder_training_host.py measures; the figures the kernels measured on an MI355X stand in the docstrings and enter no bound.
"""
import functools

import numpy as np
import pytest
import torch

import backward_ref as BR
import encoder_bwd_ref as E
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
EOT = 50257

STEM_BOUND, CONV2_DX_BOUND = E.STEM_BOUND, E.CONV2_DX_BOUND
ENC_ATTN_BOUND, ENC_ATTN_SPLIT_BOUND = E.ENC_ATTN_BOUND, E.ENC_ATTN_SPLIT_BOUND


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _model(dims, W, **kw):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.float32, **kw)
    m.load_weights(W)
    return m


# ====================================================================== 4. conv stem
@functools.lru_cache(maxsize=None)
def _stem_trainer(d: int, n_mels: int):
    """a one-block model of width d on n_mels bands with a tiny vocabulary, exact f32 products, every encoder tensor trained"""
    from whisper_ipa_amd.training import DecoderTrainer

    dims = R.ModelDimensions(n_mels, 1500, d, d // 64, 1, 64, 16, d, d // 64, 1)
    m = _model(dims, R.synthetic_weights(dims, seed=3), f32_split=False)
    return DecoderTrainer(m, train_encoder_layers="all")


@pytest.mark.parametrize("case", E.STEM_CASES, ids=lambda c: f"N{c.N}-B{c.B}-d{c.d}-mel{c.n_mels}")
def test_conv_stem_backward_matches_float64(case):
    """the trainer's stem on the case's mel and weights (conv1 / conv2 as GEMMs over overlapping rows, pre-activations kept), then
    its backward from the case's dx: both weight gradients, both bias gradients and dz1 against the float64 restatement.
    Measured on MI355X (worst over the table): dW1 3.8e-06, db1 1.4e-06, dW2 7.8e-06, db2 1.1e-06, dz1 3.9e-06."""
    N, B, d, n_mels = case
    tr = _stem_trainer(d, n_mels)
    x, ref = E.stem_inputs(case), E.stem_reference(case)
    tr.model.audio_ctx = N
    for name, key in (("encoder.conv1.weight", "W1"), ("encoder.conv1.bias", "b1"), ("encoder.conv2.weight", "W2"),
                      ("encoder.conv2.bias", "b2")):
        tr.p(name).copy_(x[key].cuda())
    _, ectx = tr._encoder_forward(x["mel"].cuda())
    stem = ectx["stem"]
    R_ = 2 * N + 2
    # the halo rows of conv2's input are zero, whatever conv1's bias
    c1 = stem["c1"][: B * R_ + 1].cpu()
    halo = torch.cat([c1[0:1]] + [c1[b * R_ + 2 * N + 1: b * R_ + 2 * N + 3] for b in range(B)])
    assert float(halo.abs().max()) == 0.0
    tr.flat_g.fill_(float("nan"))
    dz1 = tr._stem_backward(stem, x["dx"].cuda().view(B * N, d).contiguous(), B, N)
    torch.cuda.synchronize()
    dz1 = dz1.cpu()
    assert float(dz1[B * R_:].abs().max() if dz1.shape[0] > B * R_ else 0.0) == 0.0  # padding of the contraction
    rows = dz1[: B * R_].view(B, R_, d)
    assert float(rows[:, 2 * N:].abs().max()) == 0.0  # the two dead rows of every clip
    got = {"dW1": tr.g("encoder.conv1.weight").cpu(), "db1": tr.g("encoder.conv1.bias").cpu(),
           "dW2": tr.g("encoder.conv2.weight").cpu(), "db2": tr.g("encoder.conv2.bias").cpu(), "dz1": rows[:, : 2 * N]}
    errs = E.stem_errors(got, ref)
    print(f"\nstem {tuple(case)}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < STEM_BOUND[k], (case, k, v, STEM_BOUND[k])


def _run_conv2_dx(taps, z1, N, d):
    """taps [B, N + 1, 3, d] (row N of every clip NaN: the dead row of conv2's GEMM), z1 [B, 2N, d] -> the raw dz1 buffer
    [B * (2N + 2) + 4, d] (prefilled with SENTINEL) of one wipa_conv2_dx call with zero_rows = 2"""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    B, R_ = taps.shape[0], 2 * N + 2
    zbuf = torch.full((B, R_, d), float("nan"))  # halo rows NaN: frame s of clip b at row b*R + s + 1
    zbuf[:, 1: 2 * N + 1] = z1
    with on_stream() as s:
        t_d, z_d = taps.contiguous().cuda(), zbuf.cuda()
        out = torch.full((B * R_ + 4, d), BR.SENTINEL, dtype=torch.float32).cuda()
        _lib.check(_lib.lib().wipa_conv2_dx(ptr(t_d), (N + 1) * 3 * d, ptr(z_d.view(-1, d)[1:]), R_ * d, ptr(out), R_ * d, B, N, d, 2,
                                            sptr(s)), "wipa_conv2_dx")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("N", E.STEM_NS)
@pytest.mark.parametrize("d", (64, 128))
def test_conv2_dx_overlap_add_halo_batch_and_bits(N, d):
    """wipa_conv2_dx alone on float32 taps and z1: every frame against float64 (the last odd frame, which has one tap only, and the
    frames either side of a clip boundary among them); NaN in the dead tap row of every clip and in z1's halo rows does not
    leak; the dead rows of dz1 are zero and nothing is written past the last clip; clip b alone gives the bits it has in a batch
    of 3.  Measured on MI355X: 1.2e-06 (worst)."""
    B = 3
    ref = E.stem_reference(E.StemCase(N, B, d, 80))
    taps32, z32 = ref["taps"].float(), ref["z1"].float()
    taps = torch.full((B, N + 1, 3, d), float("nan"))
    taps[:, :N] = taps32
    raw = _run_conv2_dx(taps, z32, N, d)
    R_ = 2 * N + 2
    assert bool((raw[B * R_:] == BR.SENTINEL).all()), "written past the last clip"
    rows = raw[: B * R_].view(B, R_, d)
    assert not bool(torch.isnan(rows).any()) and float(rows[:, 2 * N:].abs().max()) == 0.0
    want = E.conv2_dx(taps32.double(), z32.double())
    err = BR.err_rms(rows[:, : 2 * N], want)
    worst_rows = {s: BR.err_rms(rows[:, s], want[:, s]) for s in {0, 2 * N - 1, max(2 * N - 2, 0)}}
    print(f"\nconv2_dx N={N} d={d}: {err:.2e}  first / last frames {worst_rows}")
    assert err < CONV2_DX_BOUND, (err, CONV2_DX_BOUND)
    for b in range(B):
        alone = _run_conv2_dx(taps[b:b + 1], z32[b:b + 1], N, d)
        assert BR.bits_equal(alone[:R_], raw[b * R_:(b + 1) * R_]), (b, "a clip's bits depend on its batch")


# ====================================================================== 5. attention backward at encoder shapes
@pytest.mark.parametrize("case", E.ENC_ATTN_CASES, ids=lambda c: f"T{c.Tq}-{c.layout}")
def test_attention_backward_at_encoder_shapes(case):
    """the exact kernels, non-causal with Tq = Tk, under the method of test_gpu_backward_kernels: strided and poisoned buffers, two
    runs bit-equal, gaps untouched, per-slice errors under margin x the float32 floor of these shapes.
    Measured on MI355X (worst over the table): dq 4.3e-05, dk 3.7e-05, dv 3.9e-05, dvec 4.4e-07."""
    BR.check_attention_bwd(case, ENC_ATTN_BOUND)
    assert E.check_attention_bwd_ex(case, ENC_ATTN_BOUND, 0)  # the new entry with f32_split = 0 is the same pair of kernels


@pytest.mark.parametrize("case", E.ENC_ATTN_CASES, ids=lambda c: f"T{c.Tq}-{c.layout}")
def test_split_attention_backward_at_encoder_shapes(case):
    """wipa_attention_bwd_ex with f32_split = 1 (five matmuls on the bf16 MFMA over operands split in registers) on the same strided,
    poisoned buffers: two runs bit-equal, gaps untouched, per-slice errors under margin 8 x the float32 floor of the restatement
    with every matmul operand cut to the bf16 terms the kernels keep (E.attn_backward_split32).
    Measured on MI355X (worst over the table): dq 1.35e-04, dk 1.27e-04, dv 8.4e-05, dvec 4.4e-07."""
    E.check_attention_bwd_ex(case, ENC_ATTN_SPLIT_BOUND, 1)


# ====================================================================== 6. every gradient of a step from the mel
def _batch(B: int, T: int = 8, seed: int = 11):
    """mel [B, 3000, 80] in the front end's range and tokens [B, T + 1]: rows end in EOT at different lengths"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, 3000, 80, generator=g) * 2.0 - 1.0
    rng = np.random.default_rng(seed)
    sot = [50258, 50259, 50359, 50363]
    rows = []
    for b in range(B):
        n = T + 1 - len(sot) - 1 - (b % 2) * 2
        row = sot + rng.integers(0, 50257, size=n).tolist() + [EOT]
        rows.append(row + [EOT] * (T + 1 - len(row)))
    return mel, torch.tensor(rows, dtype=torch.int64)


def _oracle(W, dims, mel, tokens, n_ctx, dtype=torch.float32):
    """loss, every gradient and the encoder output by torch.autograd through R.encoder_forward on the first 2N frames and
    R.loss_from_features"""
    N = n_ctx or dims.n_audio_ctx
    names = list(W)
    leaves = {k: W[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    xa = R.encoder_forward(leaves, dims, mel[:, : 2 * N].to(dtype))
    loss = R.loss_from_features(leaves, dims, xa, tokens, EOT)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return float(loss.detach()), dict(zip(names, grads)), xa.detach()


def _features_floor(W, dims, mel, n_ctx) -> float:
    """how far the oracle's float32 encoder is from the float64 evaluation (E.encoder_forward64): the float32 floor of the features"""
    N = n_ctx or dims.n_audio_ctx
    with torch.no_grad():
        x32 = R.encoder_forward(W, dims, mel[:, : 2 * N])
    return float((x32.double() - E.encoder_forward64(W, dims, mel[:, : 2 * N])).abs().max())


@functools.lru_cache(maxsize=None)
def _micro_oracle(n_ctx):
    """shared by the tests below; do not modify"""
    W = R.synthetic_weights(MICRO, seed=7)
    mel, tokens = _batch(2)
    return (W, mel, tokens) + _oracle(W, MICRO, mel, tokens, n_ctx) + (_features_floor(W, MICRO, mel, n_ctx),)


@pytest.mark.parametrize("n_ctx", [33, 75, None])
def test_loss_and_every_gradient_match_oracle_from_the_mel(n_ctx):
    """MICRO, train_encoder_layers="all", audio_ctx 33 / 75 / unset (1500), 2 clips x 8 targets: loss within 1e-3 and every encoder
    and decoder gradient within 2e-3 of its largest element, the bounds of test_loss_and_every_decoder_gradient_match_oracle.  The
    features of the saving forward agree with embed_audio of the same f32 model.  Then K = 1: the tensors below the last block are
    no parameters, the gradients of the trained ones are those of the "all" run bit for bit.
    Measured on MI355X: worst gradient error 3.6e-06 / 4.5e-06 / 2.6e-06 at N = 33 / 75 / 1500 (encoder tensors: 1.7e-06 / 2.9e-06 /
    2.6e-06); features 1.0e-06 / 1.2e-06 / 3.0e-06 from embed_audio's at float32 floors of 1.6e-06 / 1.8e-06 / 1.9e-06."""
    from whisper_ipa_amd.training import DecoderTrainer

    W, mel, tokens, ref_loss, ref, ref_xa, xa_floor = _micro_oracle(n_ctx)
    N = n_ctx or 1500
    m = _model(MICRO, W, audio_ctx=n_ctx, f32_split=False)
    tr = DecoderTrainer(m, train_encoder_layers="all")
    loss, _, n_valid = tr.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) < 1e-3, (float(loss), ref_loss)
    assert int(n_valid) == int(R.loss_mask(tokens[:, 1:], EOT).sum())
    assert set(tr.names) == set(ref) and len(tr.names) == len(ref)
    errs = {n: _rel(tr.g(n), ref[n]) for n in tr.names}
    worst = max(errs, key=errs.get)
    print(f"\nN={N}: loss {float(loss):.6f} (oracle {ref_loss:.6f}); worst gradient {worst} {errs[worst]:.2e}; "
          f"worst encoder gradient {max(v for k, v in errs.items() if k.startswith('encoder.')):.2e}")
    assert errs[worst] < 2e-3, (worst, errs[worst])
    # features: the saving forward and embed_audio are two float32 evaluations of one function with differently grouped sums (GEMM
    # shapes and the attention kernel differ).  The floor of such a pair is what the oracle's own float32 evaluation is off its
    # float64 one; margin 8 as everywhere here.  The north-star bound on features, 1e-3, holds for each against the oracle.
    feats = tr.last_features
    assert tuple(feats.shape) == (2, N, 128)
    e_train, e_infer = float((feats.cpu() - ref_xa).abs().max()), float((m.embed_audio(mel.cuda()).cpu() - ref_xa).abs().max())
    e_both = float((feats - m.embed_audio(mel.cuda())).abs().max())
    print(f"features: training forward {e_train:.2e}, embed_audio {e_infer:.2e} off the oracle; {e_both:.2e} apart (float32 floor {xa_floor:.2e})")
    assert e_train < 1e-3 and e_infer < 1e-3 and e_both < E.STEM_MARGIN * xa_floor
    # K = 1
    m1 = _model(MICRO, W, audio_ctx=n_ctx, f32_split=False)
    tr1 = DecoderTrainer(m1, train_encoder_layers=1)
    loss1, _, _ = tr1.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert float(loss1) == float(loss)
    enc1 = [n for n in tr1.names if n.startswith("encoder.")]
    assert enc1 and all(n.startswith(("encoder.blocks.1.", "encoder.ln_post.")) for n in enc1)
    assert not any(n.startswith(("encoder.conv", "encoder.blocks.0.")) for n in tr1.names)
    for n in tr1.names:
        assert BR.bits_equal(tr1.g(n).cpu(), tr.g(n).cpu()), n


# ====================================================================== 7. full-size tile paths
def test_small_width_gradients_match_oracle_from_the_mel(f32_mode):
    """whisper-small width (768, 12 heads), one encoder and one decoder block, audio_ctx 300, 2 clips: the tile GEMMs (600 rows), the
    K-major weight gradients with split-K slabs and the attention kernels at 12 heads.  Bounds of
    test_small_width_gradients_match_oracle: loss 1e-3, every gradient 3e-3.  ``split`` takes the GEMMs as split-bf16 products and the encoder's
    attention backward on the split-product kernels (wipa_attention_bwd_ex); the decoder's attention keeps the exact ones.
    Measured on MI355X: worst gradient 7.6e-06 exact, 3.8e-05 split."""
    from whisper_ipa_amd.training import DecoderTrainer

    dims = R.ModelDimensions(80, 1500, 768, 12, 1, 51865, 448, 768, 12, 1)
    W = R.synthetic_weights(dims, seed=13)
    mel, tokens = _batch(2, seed=17)
    ref_loss, ref, _ = _oracle(W, dims, mel, tokens, 300)
    m = _model(dims, W, audio_ctx=300, f32_split=(f32_mode == "split"))
    tr = DecoderTrainer(m, train_encoder_layers="all")
    assert tr.f32_split == (f32_mode == "split")
    loss, _, _ = tr.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert abs(float(loss) - ref_loss) < 1e-3, (float(loss), ref_loss)
    errs = {n: _rel(tr.g(n), ref[n]) for n in tr.names}
    worst = max(errs, key=errs.get)
    print(f"\nwidth 768 {f32_mode}: loss {float(loss):.6f} (oracle {ref_loss:.6f}); worst gradient {worst} {errs[worst]:.2e}")
    assert set(tr.names) == set(ref)
    assert errs[worst] < 3e-3, (worst, errs[worst])


# ====================================================================== 8. one whole step
def test_train_step_all_updates_encoder_and_drops_what_depends_on_it(f32_mode):
    """one train_step with "all" on MICRO at audio_ctx 75 against R.clip_gradients + R.adamw_mlx on the oracle's gradients, under
    the tolerances of test_train_step_matches_oracle_clip_and_adamw; afterwards the inference encoder runs on the updated weights
    and a FrozenFeatureCache filled before the step has dropped its entries.
    Measured on MI355X: the features move by 3.3 and are 3.5e-04 (exact) / 2.2e-04 (split) off the oracle on the updated weights."""
    from parity_util import norm64
    from whisper_ipa_amd.training import DecoderTrainer, FrozenFeatureCache

    p_tol0 = 2e-4 if f32_mode == "exact" else 5e-4
    W, mel, tokens, ref_loss, g_raw, _, _ = _micro_oracle(75)
    m = _model(MICRO, W, audio_ctx=75, f32_split=(f32_mode == "split"))
    tr = DecoderTrainer(m, lr=1e-3, f32_split=(f32_mode == "split"), train_encoder_layers="all")
    cache = FrozenFeatureCache(m, 4)
    before = cache.assemble([0, 1], mel.cuda()).clone()
    assert cache.missing([0, 1]) == [False, False]
    gen = m._enc_generation
    loss, grads = tr.train_step(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert m._enc_generation > gen and cache.missing([0, 1]) == [True, True]
    assert abs(float(loss) - ref_loss) < 1e-3
    g = R.clip_gradients(g_raw, 1.0, "reference")
    for k in g_raw:  # the clip by name: stem and ln_post clipped, blocks passed through
        if k.startswith("encoder.blocks."):
            assert torch.equal(g[k], g_raw[k])
    Wn = {}
    for k, gk in g.items():
        Wn[k], _, _ = R.adamw_mlx(W[k], gk, torch.zeros_like(gk), torch.zeros_like(gk), lr=1e-3)
    for n in tr.names:
        assert _rel(grads[n], g[n]) < 3e-3, ("clipped grad", n)
        assert (tr.p(n).cpu() - Wn[n]).abs().max() < p_tol0 * max(1.0, norm64(g[n])), ("param", n)
        assert m._params[n].data_ptr() == tr.p(n).data_ptr()
    after = m.embed_audio(mel.cuda())
    with torch.no_grad():
        ref_after = R.encoder_forward(Wn, MICRO, mel[:, :150])
    moved = float((after - before).abs().max())
    print(f"\nfeatures moved by {moved:.2e}; {float((after.cpu() - ref_after).abs().max()):.2e} off the oracle on the updated weights")
    assert moved > 1e-3 and float((after.cpu() - ref_after).abs().max()) < 1e-3


# ====================================================================== 9. refusals
def test_decoder_only_entry_points_refuse_a_trainer_of_encoder_layers():
    from whisper_ipa_amd._lib import WipaError
    from whisper_ipa_amd.training import DecoderTrainer, FineTuneTrainer

    W, mel, tokens, *_ = _micro_oracle(33)
    m = _model(MICRO, W, audio_ctx=33)
    tr = FineTuneTrainer(m, train_encoder_layers=1)
    assert isinstance(tr, DecoderTrainer)
    feats = m.embed_audio(mel.cuda())
    for call in (lambda: tr.enable_feature_cache(), lambda: tr.enable_feature_cache(4),
                 lambda: tr.differentiable_logits(tokens[:, :-1].cuda(), feats), lambda: tr.leaves(),
                 lambda: m.logits(tokens[:, :-1].cuda(), feats, differentiable=True),
                 lambda: tr.loss_and_grads(feats, tokens.cuda(), EOT)):
        with pytest.raises(WipaError, match="train_encoder_layers"):
            call()
    with pytest.raises(WipaError, match="train_encoder_layers"):
        DecoderTrainer(_model(MICRO, W), train_encoder_layers=3)
    # the plain inference paths stay open
    with torch.no_grad():
        assert m.logits(tokens[:, :-1].cuda(), feats).shape[:2] == (2, 8)


# ====================================================================== 10. data parallel
def _dp_worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    from whisper_ipa_amd.training import DecoderTrainer

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # one GPU box: gloo moves the CUDA tensors
    try:
        W = R.synthetic_weights(MICRO, seed=7)
        mel, tokens = _batch(4, seed=23)
        m = _model(MICRO, W, audio_ctx=33, f32_split=False)
        tr = DecoderTrainer(m, train_encoder_layers=1)
        lo, hi = rank * 2, rank * 2 + 2
        loss, _, n = tr.loss_and_grads_from_mel(mel[lo:hi].cuda(), tokens[lo:hi].cuda(), EOT)
        torch.cuda.synchronize()
        q.put((rank, float(loss), float(n), tr.flat_g.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks_equal_single_process_at_k1():
    """two ranks on one GPU, each half of 4 clips, K = 1: the all-reduced loss statistics and every gradient segment (the
    encoder's among them) equal one process on the whole batch, as test_data_parallel_two_ranks_equal_single_process has it"""
    import os

    import torch.multiprocessing as mp

    from whisper_ipa_amd.training import DecoderTrainer

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 90
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    W = R.synthetic_weights(MICRO, seed=7)
    mel, tokens = _batch(4, seed=23)
    m = _model(MICRO, W, audio_ctx=33, f32_split=False)
    tr = DecoderTrainer(m, train_encoder_layers=1)
    loss, _, n = tr.loss_and_grads_from_mel(mel.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    full = tr.flat_g.cpu().numpy()
    lo = tr.offsets["encoder.blocks.1.attn.query.weight"]
    assert np.abs(full[lo:]).max() > 0
    for r in res:
        assert abs(r[1] - float(loss)) < 1e-5 and r[2] == float(n)
        assert np.abs(r[3] - full).max() < 1e-5 * (np.abs(full).max() + 1e-9) + 1e-7
        assert np.abs(r[3][lo:] - full[lo:]).max() < 1e-5 * (np.abs(full[lo:]).max() + 1e-9) + 1e-7
    assert np.array_equal(res[0][3], res[1][3])
