"""GPU tests of LoRA fine-tuning end to end: DecoderTrainer(model, lora=...), Whisper.set_adapter, the adapter files and the scripts,
against the CPU oracle on W + s B A (torch autograd with lora_A / lora_B as leaves).  The MICRO dimensions of test_gpu_training.py
(d = 128, 2 + 2 layers), three clips, a dozen tokens.  ``pytest -m gpu``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from parity_util import norm64

pytestmark = pytest.mark.gpu

MICRO = R.ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 2)
EOT = 50257
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _tokens(lengths=(9, 5, 7), seed=5):
    rng = np.random.default_rng(seed)
    sot = [50258, 50259, 50359, 50363]
    seqs = [sot + rng.integers(0, 50257, size=n).tolist() + [EOT] for n in lengths]
    L = max(len(s) for s in seqs)
    return torch.tensor([s + [EOT] * (L - len(s)) for s in seqs], dtype=torch.int64)


@pytest.fixture(scope="module")
def setup():
    W = R.synthetic_weights(MICRO, seed=7)
    torch.manual_seed(0)
    xa = torch.randn(3, 1500, 128) * 0.7
    return W, xa, _tokens()


def _model(W, dtype=torch.float32):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**MICRO.__dict__), dtype=dtype, f32_split=False)  # exact f32 products: the bounds below are theirs
    m.load_weights({k: v.clone() for k, v in W.items()})
    return m


def _random_adapter(cfg, seed=1):
    """lora_A as the init draws it, lora_B random and nonzero (the init's zero B makes every lora_A gradient vanish)"""
    from whisper_ipa_amd import lora

    g = torch.Generator().manual_seed(seed)
    ad = lora.init_adapter(MICRO, cfg)
    return {n: (t if n.endswith("lora_A") else 0.05 * torch.randn(t.shape, generator=g)) for n, t in ad.items()}


def _merged(W, adapter, scale):
    """W + s B A, stated here: differentiable in the adapter tensors"""
    out = dict(W)
    for n in adapter:
        if n.endswith(".lora_A"):
            pre = n[: -len("lora_A")]
            out[pre + "weight"] = W[pre + "weight"] + scale * (adapter[pre + "lora_B"] @ adapter[n])
    return out


def _oracle_grads(W, adapter, scale, xa, tokens):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in adapter.items()}
    loss = R.loss_from_features(_merged(W, leaves, scale), MICRO, xa, tokens, EOT)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return float(loss.detach()), dict(zip(names, grads))


CONFIGS = [((t,), 8) for t in ALL] + [(("query", "value"), 4), (("query", "value"), 16)]


@pytest.mark.parametrize("targets,rank", CONFIGS, ids=[f"{'+'.join(t)}-r{r}" for t, r in CONFIGS])
def test_loss_and_every_adapter_gradient_match_autograd_through_the_oracle(setup, targets, rank):
    from whisper_ipa_amd.lora import LoRAConfig
    from whisper_ipa_amd.training import DecoderTrainer

    W, xa, tokens = setup
    cfg = LoRAConfig(rank=rank, alpha=2.0 * rank, targets=targets)
    adapter = _random_adapter(cfg)
    ref_loss, ref = _oracle_grads(W, adapter, cfg.scale, xa, tokens)
    m = _model(W)
    tr = DecoderTrainer(m, lora=cfg, f32_split=False)
    tr.load_adapter(adapter)
    before = {k: v.clone() for k, v in m.flat_parameters().items()}
    loss, _, n_valid = tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    print(f"\n{targets} r{rank}: loss {float(loss):.6f} against {ref_loss:.6f}")
    assert abs(float(loss) - ref_loss) < 1e-3, (float(loss), ref_loss)
    assert int(n_valid) == int(R.loss_mask(tokens[:, 1:], EOT).sum())
    assert set(tr.names) == set(ref) and tr.flat_p.numel() == sum(v.numel() for v in adapter.values())
    worst = max(((_rel(tr.g(n), ref[n]), n) for n in tr.names))
    print(f"worst adapter gradient: {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 2e-3, worst
    assert min(float(ref[n].abs().max()) for n in ref) > 0  # every adapter tensor has a gradient to match
    for k, v in m.flat_parameters().items():  # the base is never written
        assert torch.equal(v, before[k]), k


def test_fresh_adapter_gives_the_loss_of_a_trainer_without_one(setup):
    from whisper_ipa_amd.lora import LoRAConfig
    from whisper_ipa_amd.training import DecoderTrainer

    W, xa, tokens = setup
    plain = DecoderTrainer(_model(W), f32_split=False)
    loss0, _, _ = plain.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
    tr = DecoderTrainer(_model(W), lora=LoRAConfig(rank=8, targets=ALL), f32_split=False)
    loss1, _, _ = tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    assert float(loss1) == float(loss0)  # lora_B = 0: every adapted linear adds exactly zero
    # and only lora_B has a gradient then
    assert all(not tr.g(n).any() for n in tr.names if n.endswith("lora_A")) and any(tr.g(n).any() for n in tr.names if n.endswith("lora_B"))


@pytest.mark.parametrize("clip_scope", ["reference", "all"])
def test_two_train_steps_match_oracle_clip_and_adamw_and_leave_the_base_alone(setup, clip_scope):
    """the tolerances of test_gpu_training.test_train_step_matches_oracle_clip_and_adamw (exact f32 products).  Adapter names hold a block
    index: "reference" clips none of them, "all" clips each by its own norm (lora_B is scaled up so that norms above 1 occur)."""
    from whisper_ipa_amd.lora import LoRAConfig
    from whisper_ipa_amd.training import DecoderTrainer

    W, xa, tokens = setup
    cfg = LoRAConfig(rank=8, alpha=16.0, targets=("query", "value", "mlp1"))
    ad = {k: (v if k.endswith("lora_A") else 4 * v) for k, v in _random_adapter(cfg).items()}
    m = _model(W)
    base = {k: v.clone() for k, v in m.flat_parameters().items()}
    tr = DecoderTrainer(m, lr=1e-3, f32_split=False, clip_scope=clip_scope, lora=cfg)
    tr.load_adapter(ad)
    state, p_tol0 = {}, 2e-4
    seen_over = False
    for step in range(2):
        loss, _, _ = tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
        tr.apply_update()
        ref_loss, g_raw = _oracle_grads(W, ad, cfg.scale, xa, tokens)
        seen_over |= any(norm64(gk) > 1.0 for gk in g_raw.values())
        g = R.clip_gradients(g_raw, 1.0, clip_scope)
        if clip_scope == "reference":
            assert all(torch.equal(g[k], g_raw[k]) for k in g)
        p_tol = {k: p_tol0 * max(1.0, norm64(gk)) for k, gk in g.items()}
        for k, gk in g.items():
            mm, vv = state.get(k, (torch.zeros_like(gk), torch.zeros_like(gk)))
            ad[k], mm, vv = R.adamw_mlx(ad[k], gk, mm, vv, lr=1e-3)
            ad[k] = ad[k].detach()
            state[k] = (mm, vv)
        torch.cuda.synchronize()
        assert abs(float(loss) - ref_loss) < 1e-3, (step, float(loss), ref_loss)
        for n in tr.names:
            assert _rel(tr.g(n), g[n]) < 3e-3, (step, "clipped grad", n)
            assert (tr.p(n).cpu() - ad[n]).abs().max() < p_tol[n], (step, "param", n)
    assert seen_over, "no adapter gradient norm above 1: the two clip scopes would not differ"
    assert tr.step_count == 2 and tr.flat_p.numel() == sum(v.numel() for v in ad.values()) == tr.n_params
    for k, v in m.flat_parameters().items():
        assert torch.equal(v, base[k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_set_adapter_runs_the_merged_model_and_restores_the_base_bit_for_bit(setup, dtype):
    from whisper_ipa_amd.decoding import greedy_decode_tokens
    from whisper_ipa_amd.lora import LoRAConfig

    W, xa, tokens = setup
    cfg = LoRAConfig(rank=8, alpha=16.0, targets=ALL)
    ad = {k: (v if k.endswith("lora_A") else 4 * v) for k, v in _random_adapter(cfg).items()}
    other = _random_adapter(LoRAConfig(rank=4, targets=("query",)), seed=3)
    m = _model(W, dtype)
    feats = xa.cuda()
    tok_in = tokens[:, :-1].cuda()
    base = {k: v.clone() for k, v in m.flat_parameters().items()}
    with torch.no_grad():
        lg0 = m.logits(tok_in, feats).clone()
        m.set_adapter(ad, cfg)
        lg1 = m.logits(tok_in, feats).clone()
        merged1 = {k: v.clone() for k, v in m.flat_parameters().items()}
        m.set_adapter(other, LoRAConfig(rank=4, targets=("query",)))  # another adapter: merged from the bases again
        m.set_adapter(ad, cfg)
        lg2 = m.logits(tok_in, feats).clone()
        for k, v in m.flat_parameters().items():
            assert torch.equal(v, merged1[k]), k
        assert torch.equal(lg1, lg2)  # the same adapter twice: the same bits
        assert not torch.equal(lg1, lg0)
        if dtype == torch.float32:
            Wm = _merged(W, ad, cfg.scale)
            ref = R.decoder_forward(Wm, MICRO, tokens[:, :-1], xa)
            err = float((lg1.float().cpu() - ref).abs().max())
            print(f"\nmerged logits: {err:.2e} off the oracle on W + s B A")
            assert err < 1e-3
            sp = R.SpecialTokens.multilingual()
            always, first = R.suppress_lists(sp)
            init = list(sp.sot_sequence_including_notimestamps(0))
            ids = greedy_decode_tokens(m, feats, init, always, first, sp.eot, max_new_tokens=12, stop_on_eot=False).tokens
            want = R.greedy_decode(Wm, MICRO, xa, init, always, first, sp.eot, sample_len=12, stop_on_eot=False)
            gate = np.cumprod(want.margins > 1e-3, axis=1).astype(bool)  # ids the oracle itself decides by more than round-off
            assert gate.all(), "a greedy margin under 1e-3: pick another adapter seed"
            assert (np.asarray(ids) == want.tokens).all(), (ids.tolist(), want.tokens.tolist())
            base_ids = R.greedy_decode(W, MICRO, xa, init, always, first, sp.eot, sample_len=12, stop_on_eot=False).tokens
            assert not (base_ids == want.tokens).all(), "the adapter does not change the greedy ids: the check is vacuous"
        m.set_adapter(None)
        lg3 = m.logits(tok_in, feats)
    assert torch.equal(lg3, lg0)
    for k, v in m.flat_parameters().items():
        assert v.dtype == base[k].dtype and torch.equal(v, base[k]), k


def _dp_inputs():
    W = R.synthetic_weights(MICRO, seed=7)
    torch.manual_seed(0)
    xa = torch.randn(4, 1500, 128) * 0.7
    return W, xa, _tokens((9, 3, 7, 5), seed=9)


def _dp_trainer(W):
    from whisper_ipa_amd.lora import LoRAConfig
    from whisper_ipa_amd.training import DecoderTrainer

    cfg = LoRAConfig(rank=8, targets=ALL)
    tr = DecoderTrainer(_model(W), lora=cfg, f32_split=False)
    tr.load_adapter(_random_adapter(cfg))
    return tr


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # one GPU box: gloo moves the CUDA tensors
    try:
        W, xa, tokens = _dp_inputs()
        tr = _dp_trainer(W)
        lo, hi = rank * 2, rank * 2 + 2
        loss, s, n = tr.loss_and_grads(xa[lo:hi].cuda(), tokens[lo:hi].cuda(), EOT)
        torch.cuda.synchronize()
        q.put((rank, float(loss), float(n), tr.flat_g.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks_equal_single_process_on_every_adapter_gradient():
    """modelled on test_gpu_training.test_data_parallel_two_ranks_equal_single_process: the reducer gets adapter segments only"""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 90
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    W, xa, tokens = _dp_inputs()
    tr = _dp_trainer(W)
    loss, s, n = tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
    torch.cuda.synchronize()
    full = tr.flat_g.cpu().numpy()
    assert full.size == tr.n_params and sum(hi - lo for _, lo, hi in tr.segments) == full.size
    for r in res:
        assert abs(r[1] - float(loss)) < 1e-5 and r[2] == float(n)
        assert np.abs(r[3] - full).max() < 1e-5 * (np.abs(full).max() + 1e-9) + 1e-7
    assert np.array_equal(res[0][3], res[1][3])
    for name in tr.names:  # every adapter gradient is there to compare
        assert np.abs(full[tr.offsets[name]: tr.offsets[name] + tr.g(name).numel()]).max() > 0, name


def test_train_script_end_to_end_adapter_artefacts(tmp_path, capsys):
    """scripts/train_whisper_ipa.py with LoRA on a tiny local model + generated WAV clips, two steps, rank 4: adapter files in every
    checkpoint directory, the settings in training_config.json, load_model(base, adapter=DIR) == the trainer under adapter_applied()."""
    import wave

    from whisper_ipa_amd import lora
    from whisper_ipa_amd.load_models import load_model, load_safetensors, save_model
    from whisper_ipa_amd.training import DecoderTrainer
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import train_whisper_ipa as T

    dims = R.ModelDimensions(80, 1500, 64, 1, 1, 51865, 448, 64, 1, 1)
    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.float32)
    m.load_weights(R.synthetic_weights(dims, seed=4))
    model_dir = tmp_path / "whisper-micro"
    save_model(m, str(model_dir))
    entries = []
    rng = np.random.default_rng(0)
    for i in range(4):
        pcm = (0.1 * rng.standard_normal(16000 * 2) * 32767).astype("<i2")
        p = tmp_path / f"c{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
        entries.append({"audio_path": str(p), "ipa_transcription": "kæt " + "ab" * (i + 1), "speaker_id": f"s{i}"})
    (tmp_path / "train.json").write_text(json.dumps(entries))
    (tmp_path / "test.json").write_text(json.dumps(entries[:2]))
    out = tmp_path / "out"
    T.train(str(model_dir), str(tmp_path / "train.json"), str(tmp_path / "test.json"), str(out), num_steps=2, batch_size=2,
            learning_rate=1e-2, validate_every=1, save_every=1, seed=0, allow_byte_fallback=True,
            lora=dict(rank=4, alpha=8.0, targets=("query", "value"), seed=0))
    text = capsys.readouterr().out
    assert "LoRA: rank 4" in text and "Step 2/2 | Loss:" in text
    cfg = json.load(open(out / "training_config.json"))
    assert cfg["training_args"]["lora"] == {"rank": 4, "alpha": 8.0, "targets": ["query", "value"], "seed": 0}
    for d in ("checkpoint-1", "checkpoint-2", "best-checkpoint"):
        assert (out / d / "adapter_model.safetensors").exists() and (out / d / "adapter_config.json").exists()
        assert (out / d / "training_state.json").exists() and not (out / d / "model.safetensors").exists()
    conf = json.load(open(out / "checkpoint-2" / "adapter_config.json"))
    assert conf["format"] == "wipa-lora-1" and conf["r"] == 4 and conf["base_model"] == str(model_dir) and conf["audio_ctx"] is None
    assert os.path.getsize(out / "checkpoint-2" / "adapter_model.safetensors") < 64 * 1024  # 8 tensors of 4 x 64 floats
    tensors, lcfg, _ = lora.load_adapter(str(out / "checkpoint-2"))
    assert any(t.any() for n, t in tensors.items() if n.endswith("lora_B")), "two steps at lr 1e-2 left lora_B at zero"
    # load_model(base, adapter=DIR) reproduces a trainer that holds these tensors, under adapter_applied(), bit for bit
    fresh = load_model(str(model_dir))
    tr = DecoderTrainer(fresh, lora=lcfg)
    tr.load_adapter(tensors)
    tok = torch.tensor([[50258, 50259, 50359, 50363, 11, 12, 13]]).cuda()
    feats = torch.randn(1, 1500, 64, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        base_lg = fresh.logits(tok, feats).clone()
        with tr.adapter_applied():
            want = fresh.logits(tok, feats).clone()
        again = fresh.logits(tok, feats).clone()
        got = load_model(str(model_dir), adapter=str(out / "checkpoint-2")).logits(tok, feats)
    assert torch.equal(got, want) and torch.equal(again, base_lg) and not torch.equal(want, base_lg)
    base = load_safetensors(str(model_dir / "weights.safetensors"))
    assert torch.equal(fresh.flat_parameters()["decoder.blocks.0.attn.query.weight"].cpu(), base["decoder.blocks.0.attn.query.weight"])
    # transcribe_single --adapter and evaluate_model --adapter run
    import transcribe_single as TS
    TS.main(["--adapter", str(out / "checkpoint-2"), "--base-model", str(model_dir), "--audio", entries[0]["audio_path"],
             "--allow-byte-fallback"])
    text = capsys.readouterr().out
    assert "LoRA adapter applied: rank 4" in text and "Prediction:" in text
    import evaluate_model as EM
    res = EM.main(["--adapter", str(out / "best-checkpoint"), "--base-model", str(model_dir), "--test-data", str(tmp_path / "test.json"),
                   "--num-samples", "0", "--n-mels", "80", "--batch-size", "2", "--skip-base", "--allow-byte-fallback"])
    assert "LoRA adapter applied" in capsys.readouterr().out and res["trained"]["num_samples"] == 2


def test_refusals_by_name(setup):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.lora import LoRAConfig
    from whisper_ipa_amd.training import DecoderTrainer

    W, xa, tokens = setup
    cfg = LoRAConfig(rank=4)
    m = _model(W)
    with pytest.raises(_lib.WipaError, match="train_encoder_layers"):
        DecoderTrainer(m, lora=cfg, train_encoder_layers=1)
    with pytest.raises(_lib.WipaError, match="LoRAConfig"):
        DecoderTrainer(m, lora={"rank": 4})
    tr = DecoderTrainer(m, lora=cfg)
    with pytest.raises(_lib.WipaError, match="leaves on a LoRA trainer"):
        tr.leaves()
    with pytest.raises(_lib.WipaError, match="differentiable_logits on a LoRA trainer"):
        tr.differentiable_logits(tokens[:, :-1].cuda(), xa.cuda())
    with pytest.raises(_lib.WipaError, match="unknown target"):
        LoRAConfig(targets=("embedding",))
    with pytest.raises(_lib.WipaError, match="rank"):
        LoRAConfig(rank=66)
    with tr.adapter_applied():
        with pytest.raises(_lib.WipaError, match="adapter applied"):
            tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)
        with pytest.raises(_lib.WipaError, match="load_weights while an adapter is applied"):
            m.load_weights(W)
    tr.loss_and_grads(xa.cuda(), tokens.cuda(), EOT)  # and steps again once it is removed
    plain = DecoderTrainer(_model(W))
    with pytest.raises(_lib.WipaError, match="needs a trainer built with lora"):
        plain.adapter()
    bf = _model(W, torch.bfloat16)
    bf.quantize_weights()
    with pytest.raises(_lib.WipaError, match="fp8"):
        bf.set_adapter(_random_adapter(cfg), cfg)
    with pytest.raises(_lib.WipaError, match="missing"):
        _model(W).set_adapter({}, cfg)
