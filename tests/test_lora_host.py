"""CPU tests of the low-rank adapter host code (whisper_ipa_amd/lora.py) and of tests/lora_ref.py: layout, names, initialisation,
adapter files, the merged weight against float64, every refusal by name, and the float32 floors of the GPU test's case table against the
constants committed in tests/test_gpu_lora_kernels.py.  No GPU."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import lora_ref as LR
import test_gpu_lora_kernels as G
from whisper_ipa_amd import _lib, lora
from whisper_ipa_amd.lora import LoRAConfig
from whisper_ipa_amd.whisper import ModelDimensions

DIMS = ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 3)  # d = 128, three decoder blocks
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")


def test_targets_expand_to_the_names_the_issue_gives():
    cfg = LoRAConfig(rank=8)
    assert cfg.targets == ("query", "value") and cfg.scale == 4.0
    assert cfg.sites() == ("attn.query", "attn.value", "cross_attn.query", "cross_attn.value")
    names = lora.adapter_names(DIMS, cfg)
    assert names[:2] == ["decoder.blocks.0.attn.query.lora_A", "decoder.blocks.0.attn.query.lora_B"]
    assert len(names) == 3 * 4 * 2 and len(set(names)) == len(names)
    assert LoRAConfig(targets=("attn.query", "cross_attn.value", "mlp2")).sites() == ("attn.query", "cross_attn.value", "mlp2")
    assert LoRAConfig(targets=ALL).sites() == lora.SITES
    assert LoRAConfig(targets="mlp1").targets == ("mlp1",)
    assert lora.adapter_shape(DIMS, cfg, "decoder.blocks.1.attn.query.lora_A") == (8, 128)
    assert lora.adapter_shape(DIMS, cfg, "decoder.blocks.1.mlp1.lora_B") == (512, 8)
    assert lora.adapter_shape(DIMS, cfg, "decoder.blocks.1.mlp2.lora_A") == (8, 512)
    assert lora.adapted_weights({n: None for n in names})[0] == "decoder.blocks.0.attn.query.weight"


@pytest.mark.parametrize("targets", [("query", "value"), ALL, ("cross_attn.key",)])
def test_layout_has_no_gaps_and_follows_the_backwards_order(targets):
    cfg = LoRAConfig(rank=12, targets=targets)
    lay = lora.adapter_layout(DIMS, cfg)
    assert lay["names"] == lora.adapter_names(DIMS, cfg)
    off = 0
    for n, sz in zip(lay["names"], lay["sizes"]):
        assert lay["offsets"][n] == off and sz % 4 == 0 and sz == int(np.prod(lora.adapter_shape(DIMS, cfg, n)))
        off += sz
    assert off == lay["total"]
    # segments: the last block first, block 0 last; contiguous, disjoint, covering the buffer; each holds exactly its block's tensors
    assert [s[0] for s in lay["segments"]] == ["decoder.blocks.2", "decoder.blocks.1", "decoder.blocks.0"]
    assert sorted((lo, hi) for _, lo, hi in lay["segments"]) == [(i * off // 3, (i + 1) * off // 3) for i in range(3)]
    for label, lo, hi in lay["segments"]:
        inside = [n for n in lay["names"] if lo <= lay["offsets"][n] < hi]
        assert inside and all(n.startswith(label + ".") for n in inside)


def test_init_is_reproducible_with_b_zero_and_a_within_its_bound():
    cfg = LoRAConfig(rank=8, targets=ALL, seed=3)
    a, b = lora.init_adapter(DIMS, cfg), lora.init_adapter(DIMS, cfg)
    other = lora.init_adapter(DIMS, LoRAConfig(rank=8, targets=ALL, seed=4))
    assert list(a) == lora.adapter_names(DIMS, cfg)
    for n, t in a.items():
        assert t.dtype == torch.float32 and tuple(t.shape) == lora.adapter_shape(DIMS, cfg, n)
        assert t.numpy().tobytes() == b[n].numpy().tobytes()
        if n.endswith("lora_B"):
            assert not t.any()
        else:
            assert float(t.abs().max()) <= t.shape[1] ** -0.5 and float(t.abs().max()) > 0.5 * t.shape[1] ** -0.5 and float(t.std()) > 0
            assert not torch.equal(t, other[n])


def test_save_load_round_trip_is_bit_equal(tmp_path):
    cfg = LoRAConfig(rank=4, alpha=6.0, targets=("out", "mlp1"), seed=9)
    g = torch.Generator().manual_seed(1)
    adapter = {n: torch.randn(t.shape, generator=g) for n, t in lora.init_adapter(DIMS, cfg).items()}
    lora.save_adapter(str(tmp_path / "a"), adapter, cfg, {"base_model": "whisper-micro", "audio_ctx": 300})
    conf = json.load(open(tmp_path / "a" / "adapter_config.json"))
    assert conf["format"] == "wipa-lora-1" and conf["r"] == 4 and conf["lora_alpha"] == 6.0 and conf["target_modules"] == ["out", "mlp1"]
    assert conf["base_model"] == "whisper-micro" and conf["audio_ctx"] == 300
    assert (tmp_path / "a" / "adapter_model.safetensors").exists()
    back, cfg2, conf2 = lora.load_adapter(str(tmp_path / "a"))
    assert cfg2 == cfg and conf2 == conf and set(back) == set(adapter)
    for n in adapter:
        assert back[n].numpy().tobytes() == adapter[n].numpy().tobytes()
    lora.check_adapter(DIMS, cfg2, back)
    with pytest.raises(FileNotFoundError, match="adapter_config.json"):
        lora.load_adapter(str(tmp_path / "missing"))
    conf["format"] = "peft"
    json.dump(conf, open(tmp_path / "a" / "adapter_config.json", "w"))
    with pytest.raises(_lib.WipaError, match="format 'peft'"):
        lora.load_adapter(str(tmp_path / "a"))


def test_merged_weights_agree_with_float64():
    cfg = LoRAConfig(rank=8, alpha=4.0, targets=("query", "mlp2"))
    g = torch.Generator().manual_seed(2)
    adapter = {n: torch.randn(t.shape, generator=g) * 0.1 for n, t in lora.init_adapter(DIMS, cfg).items()}
    W = {wn: torch.randn(*lora.site_shape(DIMS, wn.split(".", 3)[-1][: -len(".weight")]), generator=g) for wn in lora.adapted_weights(adapter)}
    W["decoder.ln.weight"] = torch.ones(128)
    out = lora.merged_weights(W, adapter, cfg)
    assert out["decoder.ln.weight"] is W["decoder.ln.weight"] and set(out) == set(W)
    for wn in lora.adapted_weights(adapter):
        pre = wn[: -len("weight")]
        ref = LR.merge(W[wn].numpy(), adapter[pre + "lora_A"].numpy(), adapter[pre + "lora_B"].numpy(), 0.5)
        assert tuple(out[wn].shape) == tuple(W[wn].shape) and LR.err_rms(out[wn].numpy(), ref) < 1e-6
        assert LR.err_rms(W[wn].numpy(), ref) > 1e-2  # the adapter moved the weight


def test_config_refusals_carry_their_name():
    for bad in (0, 2, 6, 68, 128, -4, 8.0, True):
        with pytest.raises(_lib.WipaError, match="rank"):
            LoRAConfig(rank=bad)
    for bad in (("qeury",), ("query", "embedding"), ("attn.mlp1",), ("encoder.query",)):
        with pytest.raises(_lib.WipaError, match="unknown target"):
            LoRAConfig(targets=bad)
    with pytest.raises(_lib.WipaError, match="targets is empty"):
        LoRAConfig(targets=())
    cfg = LoRAConfig(rank=4)
    good = lora.init_adapter(DIMS, cfg)
    with pytest.raises(_lib.WipaError, match="missing"):
        lora.check_adapter(DIMS, cfg, {k: v for k, v in list(good.items())[1:]})
    with pytest.raises(_lib.WipaError, match="unexpected"):
        lora.check_adapter(DIMS, cfg, dict(good, **{"decoder.blocks.0.mlp1.lora_A": torch.zeros(4, 128)}))
    with pytest.raises(_lib.WipaError, match="has shape"):
        lora.check_adapter(DIMS, LoRAConfig(rank=8), good)


def test_kernel_entry_points_refuse_by_argument_name_before_any_launch():
    """fake (never dereferenced) pointers: every check comes before the first launch"""
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def fwd(x=p, ldx=64, A=p, Bm=p, y=p, ldy=64, u=p, M=8, K=64, N=64, r=8):
        rc = L.wipa_lora_fwd(x, ldx, A, Bm, y, ldy, u, M, K, N, r, 1.0, None)
        return rc, L.wipa_last_error().decode()

    def bwd(dy=p, ldy=64, x=p, ldx=64, u=p, dA=p, dB=p, dx=p, lddx=64, M=8, K=64, N=64, r=8, ws=p, ws_bytes=1 << 30):
        rc = L.wipa_lora_bwd(dy, ldy, x, ldx, u, p, p, dA, dB, dx, lddx, 0, M, K, N, r, 1.0, ws, ws_bytes, None)
        return rc, L.wipa_last_error().decode()

    def merge(W=p, ldw=64, dtype=_lib.WIPA_F32, base=p, ldb=64, N=64, K=64, r=8):
        rc = L.wipa_lora_merge(W, ldw, dtype, base, ldb, p, p, N, K, r, 1.0, None)
        return rc, L.wipa_last_error().decode()

    for call, kw, word in ((fwd, dict(r=6), "r = 6"), (fwd, dict(r=68), "r = 68"), (fwd, dict(r=0), "r = 0"), (fwd, dict(K=66), "K = 66"),
                           (fwd, dict(N=62), "N = 62"), (fwd, dict(M=0), "M = 0"), (fwd, dict(ldx=66), "ldx = 66"), (fwd, dict(ldx=60), "ldx = 60"),
                           (fwd, dict(ldy=70), "ldy = 70"), (fwd, dict(x=odd), "x:"), (fwd, dict(y=odd), "y:"), (fwd, dict(u=None), "u:"),
                           (fwd, dict(Bm=odd), "Bm:"),
                           (bwd, dict(r=12, K=30), "K = 30"), (bwd, dict(r=2), "r = 2"), (bwd, dict(lddx=62), "lddx = 62"), (bwd, dict(dx=odd), "dx:"),
                           (bwd, dict(dA=None), "dA:"), (bwd, dict(dB=odd), "dB:"), (bwd, dict(ws=None), "workspace:"),
                           (bwd, dict(ws_bytes=16), "workspace_bytes = 16"), (bwd, dict(ldy=32), "ldy = 32"),
                           (merge, dict(r=5), "r = 5"), (merge, dict(dtype=7), "dtype = 7"), (merge, dict(ldw=32), "ldw = 32"),
                           (merge, dict(ldb=66), "ld_base = 66"), (merge, dict(W=odd), "W:"), (merge, dict(K=6), "K = 6")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("wipa_lora_") and word in msg, (kw, rc, msg)
    assert L.wipa_lora_workspace_bytes(4500, 128, 128, 8) == 4 * (4500 * 8 + 71 * 8 * 256)  # du, then 71 chunks of 64 rows
    assert L.wipa_lora_workspace_bytes(48000, 768, 768, 16) == 4 * (48000 * 16 + 128 * 16 * 1536)  # at most 128 chunks
    assert L.wipa_lora_workspace_bytes(1, 64, 64, 4) == 4 * (4 + 4 * 128)


def test_case_table_is_the_issues():
    assert [(c.M, c.K, c.N, c.r) for c in LR.CASES] == [(1, 64, 64, 4), (17, 128, 192, 8), (64, 128, 128, 16), (65, 512, 128, 16),
                                                        (130, 128, 512, 64), (4500, 128, 128, 8)]
    assert LR.CASES[1].ldx > LR.CASES[1].K
    big = LR.CASES[-1]
    assert big.ldy == 256 and big.dx_null and all(not c.dx_null for c in LR.CASES[:-1])
    assert {c.accumulate_dx for c in LR.CASES if not c.dx_null} == {0, 1}
    gains = {c.gain for c in LR.CASES}
    assert 1.0 in gains and LR.QK_SCALE in gains and min(gains) < 0
    for c in LR.CASES:
        assert float(np.abs(LR.inputs(c)["Bm"]).min()) > 0  # a zero Bm makes du and dA vanish and shows nothing


def test_reference_equals_float64_autograd():
    c = LR.CASES[1]
    x, ref = LR.inputs(c), LR.reference(c)
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in x.items()}
    xx, A, Bm = t["x"].requires_grad_(True), t["A"].requires_grad_(True), t["Bm"].requires_grad_(True)
    y = t["y0"] + c.gain * (xx @ A.T) @ Bm.T
    y.backward(t["dy"])
    assert LR.err_rms(y.detach().numpy(), ref["y"]) < 1e-12 and LR.err_rms((xx @ A.T).detach().numpy(), ref["u"]) < 1e-12
    # the backward reads u rounded to float32: dB differs from autograd's by that rounding alone
    assert LR.err_rms(ref["dA"], A.grad.numpy()) < 1e-12 and LR.err_rms(ref["dB"], Bm.grad.numpy()) < 1e-6
    assert LR.err_rms(ref["dx"], (xx.grad + t["dx0"]).numpy()) < 1e-12


def test_float32_floors_lie_under_the_committed_constants():
    worst = {}
    for c in LR.CASES:
        f = LR.floor32(c)
        print(f"\n{c.id}: " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\nworst float32 floors:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert set(worst) == set(G.FLOOR) == set(LR.OUTPUTS)
    for k, v in worst.items():
        assert v <= G.FLOOR[k], (k, v, G.FLOOR[k])
        assert G.BOUND[k] == LR.MARGIN * G.FLOOR[k]
    assert LR.MARGIN == 4.0


def test_merge_bound_is_the_chains_and_a_float32_evaluation_meets_it():
    for N, K, r, s in LR.MERGE_CASES:
        x = LR.merge_inputs(N, K, r)
        ref, bound = LR.merge(x["base"], x["A"], x["Bm"], s), LR.merge_bound(x["base"], x["A"], x["Bm"], s, r)
        got = LR.merge(x["base"], x["A"], x["Bm"], s, np.float32)
        assert float((np.abs(got - ref) / bound).max()) <= 1.0
        assert N % 4 == 0 and K % 4 == 0 and r % 4 == 0
