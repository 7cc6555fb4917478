"""Host half of the encoder fine-tune tests (no GPU): the flat layout of a trainer that trains encoder layers, the float64
restatements of tests/encoder_bwd_ref.py against torch.autograd, and the float32 / split floors behind every bound of
tests/test_gpu_encoder_training.py (the constants live in encoder_bwd_ref.py)."""
import pytest
import torch

import backward_ref as BR
import encoder_bwd_ref as E
from oracle import whisper_ref as R

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)  # as tests/test_gpu_training.py


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@pytest.mark.parametrize("tel", [0, 1, 2, "all"])
def test_flat_layout_keeps_the_decoder_and_appends_the_trained_encoder_tensors(tel):
    from whisper_ipa_amd.training import clip_reaches, flat_layout, parameter_shape
    from whisper_ipa_amd.whisper import parameter_names

    W = R.synthetic_weights(MICRO, seed=7)
    every = parameter_names(MICRO)
    assert all(tuple(W[n].shape) == parameter_shape(MICRO, n) for n in every)
    lay = flat_layout(MICRO, tel)
    # the decoder: today's names, order and offsets (the running sum of the decoder tensors in parameter_names order)
    dec = [n for n in every if n.startswith("decoder.")]
    off = 0
    for i, n in enumerate(dec):
        assert lay["names"][i] == n and lay["offsets"][n] == off
        off += W[n].numel()
    dec_total = off
    # the trained encoder tensors follow in parameter_names order
    L = MICRO.n_audio_layer
    first = {0: L, 1: L - 1, 2: L - 2, "all": 0}[tel]
    want = [n for n in every if n.startswith("encoder.") and (
        tel == "all" or (n.startswith("encoder.ln_post.") and first < L)
        or (n.startswith("encoder.blocks.") and int(n.split(".")[2]) >= first))]
    assert lay["names"][len(dec):] == want
    assert "encoder._positional_embedding" not in lay["names"]
    for n in want:
        assert lay["offsets"][n] == off
        off += W[n].numel()
    assert lay["total"] == off and (tel != 0 or off == dec_total)
    # the segments tile the buffer exactly once ...
    spans = sorted((lo, hi) for _, lo, hi in lay["segments"])
    assert spans[0][0] == 0 and spans[-1][1] == lay["total"]
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and all(lo < hi for lo, hi in spans)
    # ... each holds whole tensors of its own part only ...
    for label, lo, hi in lay["segments"]:
        inside = [n for n in lay["names"] if lo <= lay["offsets"][n] < hi]
        assert sum(_numel(parameter_shape(MICRO, n)) for n in inside) == hi - lo
        if label.startswith(("decoder.blocks.", "encoder.blocks.", "encoder.ln_post")):
            assert all(n.startswith(label + ".") for n in inside), label
        if label == "encoder.stem":
            assert all(n.startswith("encoder.conv") for n in inside)
    # ... and finish in the order of the backward
    order = [label for label, _, _ in lay["segments"]]
    want_order = ["decoder.tail"] + [f"decoder.blocks.{l}" for l in reversed(range(MICRO.n_text_layer))] + ["decoder.head"]
    if first < L:
        want_order += ["encoder.ln_post"] + [f"encoder.blocks.{l}" for l in reversed(range(first, L))]
    if tel == "all":
        want_order += ["encoder.stem"]
    assert order == want_order
    # the clip by name, as it stands
    for n in want:
        block = n.startswith("encoder.blocks.")
        assert clip_reaches(n, "reference") == (not block), n
        assert clip_reaches(n, "all")


def test_train_encoder_layers_values_are_checked():
    from whisper_ipa_amd._lib import WipaError
    from whisper_ipa_amd.training import FineTuneTrainer, DecoderTrainer, resolve_train_encoder_layers

    assert FineTuneTrainer is DecoderTrainer
    assert resolve_train_encoder_layers(0, 12) == (12, False) and resolve_train_encoder_layers(12, 12) == (0, False)
    assert resolve_train_encoder_layers(2, 12) == (10, False) and resolve_train_encoder_layers("all", 12) == (0, True)
    for bad in (-1, 13, True, "2", 1.0, None):
        with pytest.raises(WipaError, match="train_encoder_layers"):
            resolve_train_encoder_layers(bad, 12)


@pytest.mark.parametrize("N", E.STEM_NS)
def test_stem_restatement_equals_autograd_in_float64(N):
    """conv1 / conv2 and the overlap-add written out tap by tap against torch.autograd through F.conv1d and the oracle's _gelu"""
    for case in (c for c in E.STEM_CASES if c.N == N):
        errs = E.stem_errors(E.stem_autograd(E.stem_inputs(case)), E.stem_reference(case))
        assert max(errs.values()) < 1e-12, (case, errs)
    # the last odd frame has one tap only, and an even frame never more than one
    case = E.StemCase(N, 1, 64, 80)
    ref = E.stem_reference(case)
    taps, z1 = ref["taps"], ref["z1"]
    last = taps[:, N - 1, 2] * E.gelu_grad(z1[:, 2 * N - 1])
    assert torch.equal(ref["dz1"][:, 2 * N - 1], last)
    assert torch.equal(ref["dz1"][:, 0], taps[:, 0, 1] * E.gelu_grad(z1[:, 0]))


@pytest.mark.parametrize("T", (1, 2, 33, 75))
def test_non_causal_attention_restatement_equals_autograd_in_float64(T):
    case = BR.AttnCase(False, T, T, "a", 64 ** -0.25)
    x = BR.attn_inputs(case)
    sc = case.qk_scale
    # autograd w.r.t. the UNSCALED projections: the kernel is given q, k pre-scaled and multiplies dq, dk by the scale
    qu, ku = (x["q"].double() / sc).requires_grad_(True), (x["k"].double() / sc).requires_grad_(True)
    v = x["v"].double().requires_grad_(True)
    s = torch.einsum("bqhd,bkhd->bhqk", qu * sc, ku * sc)
    out = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)
    (out * x["d_out"].double()).sum().backward()
    o, lse = BR.attn_forward(x["q"], x["k"], x["v"], False)
    dq, dk, dv, _ = BR.attn_backward(x["q"], x["k"], x["v"], o, lse, x["d_out"], False, sc)
    for got, ref in ((dq, qu.grad), (dk, ku.grad), (dv, v.grad)):  # absolute: with one key dq and dk are zero
        assert float((got - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


def test_float64_encoder_restatement_follows_the_oracle():
    """E.encoder_forward64 (the float64 reference behind the features' float32 floor) is the oracle's encoder: its result agrees
    with the oracle's float32 evaluation to float32 round-off, at a short context and with the dead conv rows in play"""
    W = R.synthetic_weights(MICRO, seed=7)
    mel = torch.rand(2, 3000, 80, generator=torch.Generator().manual_seed(1)) * 2 - 1
    for N in (1, 33, 75):
        with torch.no_grad():
            x32 = R.encoder_forward(W, MICRO, mel[:, : 2 * N])
        x64 = E.encoder_forward64(W, MICRO, mel[:, : 2 * N])
        assert x64.dtype == torch.float64 and tuple(x64.shape) == (2, N, 128)
        assert float((x32.double() - x64).abs().max()) < 2e-5


def test_stem_floors_are_under_the_constants():
    worst, worst_dx = {}, 0.0
    for case in E.STEM_CASES:
        for k, v in E.stem_floor32(case).items():
            worst[k] = max(worst.get(k, 0.0), v)
        worst_dx = max(worst_dx, E.conv2_dx_floor32(case))
    print("\nstem floors", {k: f"{v:.2e}" for k, v in worst.items()}, f"conv2_dx alone {worst_dx:.2e}")
    assert set(worst) == set(E.STEM_FLOOR)
    for k, v in worst.items():
        assert v <= E.STEM_FLOOR[k] <= 2.5 * v, (k, v)  # the constant is the floor rounded up, not a loosened one
        assert E.STEM_BOUND[k] == E.STEM_MARGIN * E.STEM_FLOOR[k]
    assert worst_dx <= E.CONV2_DX_FLOOR <= 2.5 * worst_dx and E.CONV2_DX_BOUND == E.STEM_MARGIN * E.CONV2_DX_FLOOR


def test_attention_floors_at_encoder_shapes_are_under_the_constants():
    exact, split = {}, {}
    for case in E.ENC_ATTN_CASES:
        for k, v in BR.attn_floor32(case).items():
            exact[k] = max(exact.get(k, 0.0), v)
        for k, v in E.attn_split_floor32(case).items():
            split[k] = max(split.get(k, 0.0), v)
    print("\nattention floors at encoder shapes: exact", {k: f"{v:.2e}" for k, v in exact.items()},
          "split", {k: f"{v:.2e}" for k, v in split.items()})
    for floors, const, bound in ((exact, E.ENC_ATTN_FLOOR, E.ENC_ATTN_BOUND), (split, E.ENC_ATTN_SPLIT_FLOOR, E.ENC_ATTN_SPLIT_BOUND)):
        for k, v in floors.items():
            assert v <= const[k] <= 2.5 * v, (k, v, const[k])
            assert bound[k] == BR.ATTN_MARGIN * const[k]
    # cutting the operands to bf16 terms costs something, but stays within a small factor of float32: the split floor is no licence
    assert all(exact[k] <= split[k] <= 4 * exact[k] for k in ("dq", "dk", "dv")) and split["dvec"] == exact["dvec"]
