"""CPU tests of the adapter bank: tests/lora_bank_ref.py (addressing, the float32 floors behind the GPU test's constant), lora.AdapterBank
(stacking, the ids mapping, every refusal by name), the layouts of wipa_lora_bank_desc, wipa_adapter_bank and the new last field of
wipa_decode_call against a compiled C program, and the refusals of wipa_lora_bank_apply, of a decode call with a bank and of
wipa_decoder_adapt_cross, which all come before any launch (fake pointers).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import lora_bank_ref as BR
import test_gpu_lora_bank_kernels as G
from whisper_ipa_amd import _lib, lora
from whisper_ipa_amd.lora import LoRAConfig
from whisper_ipa_amd.whisper import ModelDimensions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = ModelDimensions(80, 1500, 128, 2, 2, 51865, 448, 128, 2, 3)  # d = 128, three decoder blocks
ALL = ("query", "key", "value", "out", "mlp1", "mlp2")
FAKE = 0x1000  # 16-byte aligned, never dereferenced


def _adapter(cfg: LoRAConfig, seed: int):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn(t.shape, generator=g) for n, t in lora.init_adapter(DIMS, cfg).items()}


# ---------------------------------------------------------------------------------------------------- the reference
def test_case_table_is_the_issues():
    assert [(c.M, c.K, c.N, c.r, c.n, c.rows_per_id) for c in BR.CASES] == [
        (1, 64, 64, 4, 1, 1), (5, 128, 192, 8, 3, 1), (64, 128, 384, 16, 7, 1), (8, 512, 128, 64, 2, 4), (111, 128, 128, 16, 3, 37),
        (17, 128, 512, 8, 3, 1)]
    c = BR.CASES
    assert -1 in c[1].ids and (c[1].ld or c[1].N) > c[1].N
    assert c[2].rg_in == 1 and c[2].cg_in == 128 and c[2].c_offset_dev
    assert c[4].rows_per_id % 16 and c[5].act == 1
    for case in c:
        assert len(case.ids) == -(-case.M // case.rows_per_id) and all(-1 <= i < case.n for i in case.ids)
        assert len(case.seg_adapted) == len(case.col_scale) == case.n_seg and case.N % (4 * case.n_seg) == 0


@pytest.mark.parametrize("case", BR.CASES, ids=lambda c: c.id)
def test_addressing_is_injective_and_matches_the_layouts(case):
    off = BR.offsets(case)
    assert off.shape == (case.M, case.N) and len(np.unique(off)) == off.size and int(off.min()) >= 0 and not (off % 4)[:, ::4].any()
    if case is BR.CASES[2]:  # [3][64 rows][8 positions][128] at position 3
        buf = np.arange(3 * 64 * 8 * 128).reshape(3, 64, 8, 128)
        assert off[5, 128 + 7] == buf[1, 5, 3, 7] and off[63, 2 * 128 + 127] == buf[2, 63, 3, 127]
    if case is BR.CASES[4]:  # 8 elements in front of [clip][K | V][H = 1][37 frames][64]
        buf = 8 + np.arange(3 * 2 * 37 * 64).reshape(3, 2, 1, 37, 64)
        assert off[37 + 36, 64 + 5] == buf[1, 1, 0, 36, 5] and off[2 * 37, 0] == buf[2, 0, 0, 0, 0]


def test_reference_against_a_merged_weight_and_its_own_rules():
    """a row's output is what the merged weight of its adapter gives; -1 rows and segments without an adapter keep y; the GELU is exact"""
    case = BR.CASES[1]
    x, ref = BR.inputs(case), BR.reference(case)
    sn = case.N // case.n_seg
    for m, i in enumerate(case.ids):
        for s in range(case.n_seg):
            cols = slice(s * sn, (s + 1) * sn)
            if i < 0 or not case.seg_adapted[s]:
                assert np.array_equal(ref["out"][m, cols], x["y0"][m, cols].astype(np.float64))
            else:
                dW = case.col_scale[s] * float(x["gain"][i]) * (x["B"][s, i].astype(np.float64) @ x["A"][s, i].astype(np.float64))
                assert np.allclose(ref["out"][m, cols], x["y0"][m, cols] + dW @ x["x"][m].astype(np.float64), rtol=1e-12, atol=1e-12)
    assert BR.written(case).sum() == 4 * 2 * sn
    g = BR.CASES[5]
    r = BR.reference(g)
    assert np.allclose(r["out"], torch.nn.functional.gelu(torch.from_numpy(r["pre"])).numpy(), rtol=1e-12, atol=1e-14)
    assert BR.written(g).all()
    v = np.asarray([1.0, 1.00390625, 1.01171875, -3.0e-5], dtype=np.float32)
    assert np.array_equal(BR.bf16_round(v), torch.from_numpy(v).to(torch.bfloat16).float().numpy())


def test_float32_floors_stay_below_the_committed_constant():
    floors = {(c.id, bf): BR.floor32(c, bf) for c in BR.CASES + BR.EXTRA_CASES for bf in (False, True)}
    worst = max(floors.values())
    print("\nfloat32 numpy floors: " + "  ".join(f"{k[0]}{'/bf16' if k[1] else ''} {v:.2e}" for k, v in floors.items()))
    assert 0 < worst <= G.FLOOR <= 2 * worst, (worst, G.FLOOR)  # at or above the floor wherever this runs, and not inflated


# ---------------------------------------------------------------------------------------------------- lora.AdapterBank
def test_bank_stacks_in_mapping_order_with_a_gain_per_adapter():
    cfgs = dict(tr=LoRAConfig(rank=8, alpha=16.0, targets=ALL, seed=1), de=LoRAConfig(rank=8, alpha=4.0, targets=ALL, seed=2),
                ku=LoRAConfig(rank=8, alpha=8.0, targets=ALL, seed=3))
    ad = {k: (_adapter(c, 10 + i), c) for i, (k, c) in enumerate(cfgs.items())}
    bank = lora.AdapterBank(DIMS, ad, device="cpu")
    assert bank.names == ("tr", "de", "ku") and len(bank) == 3 and bank.rank == 8 and bank.sites == lora.SITES and bank.n_layer == 3
    assert bank.gain.dtype == torch.float32 and bank.gain.tolist() == [2.0, 0.5, 1.0]
    assert set(bank.A) == set(bank.B) == {(l, s) for l in range(3) for s in lora.SITES}
    for (l, s), A in bank.A.items():
        B = bank.B[(l, s)]
        n_out, n_in = lora.site_shape(DIMS, s)
        assert A.shape == (3, 8, n_in) and B.shape == (3, n_out, 8) and A.is_contiguous() and B.is_contiguous() and A.dtype == B.dtype == torch.float32
        for i, k in enumerate(bank.names):
            assert torch.equal(A[i], ad[k][0][f"decoder.blocks.{l}.{s}.lora_A"]) and torch.equal(B[i], ad[k][0][f"decoder.blocks.{l}.{s}.lora_B"])
    assert bank.ids(["tr", None, "de", "ku", "de", "tr"]) == [0, -1, 1, 2, 1, 0]
    assert bank.ids([]) == []
    with pytest.raises(_lib.WipaError, match=r"row 1: no adapter 'fr' in the bank \(tr, de, ku\)"):
        bank.ids(["tr", "fr"])


def test_bank_refuses_by_name():
    c8, c4 = LoRAConfig(rank=8, seed=1), LoRAConfig(rank=4, seed=1)
    with pytest.raises(_lib.WipaError, match="adapter 'b' has rank 4, adapter 'a' has rank 8"):
        lora.AdapterBank(DIMS, dict(a=(_adapter(c8, 1), c8), b=(_adapter(c4, 2), c4)), device="cpu")
    cq = LoRAConfig(rank=8, targets=("query",))
    with pytest.raises(_lib.WipaError, match="adapter 'b' sits on .* one set of sites per bank"):
        lora.AdapterBank(DIMS, dict(a=(_adapter(c8, 1), c8), b=(_adapter(cq, 2), cq)), device="cpu")
    with pytest.raises(_lib.WipaError, match="0 adapters: a bank holds 1..64"):
        lora.AdapterBank(DIMS, {}, device="cpu")
    with pytest.raises(_lib.WipaError, match="65 adapters"):
        one = _adapter(c4, 1)
        lora.AdapterBank(DIMS, {f"a{i}": (one, c4) for i in range(65)}, device="cpu")
    broken = _adapter(c8, 1)
    broken.pop("decoder.blocks.1.attn.query.lora_B")
    with pytest.raises(_lib.WipaError, match="adapter: tensors do not match"):
        lora.AdapterBank(DIMS, dict(a=(broken, c8)), device="cpu")
    # alpha may differ, and so may the spelling of the same sites
    both = LoRAConfig(rank=8, alpha=3.0, targets=("attn.query", "cross_attn.query", "attn.value", "cross_attn.value"))
    bank = lora.AdapterBank(DIMS, dict(a=(_adapter(c8, 1), c8), b=(_adapter(both, 2), both)), device="cpu")
    assert bank.gain.tolist() == [4.0, 0.375]


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_bank_desc_layout_matches_c(tmp_path):
    import __graft_entry__ as g

    g.build()
    fields = ("x", "y", "out", "A", "B", "gain", "ids", "ids_host", "c_offset_dev", "ldx", "ld", "rg_stride", "cg_stride", "c_offset", "col_scale",
              "M", "K", "N", "r", "n", "rows_per_id", "n_seg", "ids_stride", "x_dtype", "y_dtype", "rg_in", "cg_in", "act")
    assert tuple(f[0] for f in _lib.LoraBankDesc._fields_) == fields
    prog = tmp_path / "lay.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wipa.h"\nint main(){\n'
                    'printf("%zu %d %d\\n", sizeof(wipa_lora_bank_desc), WIPA_LORA_BANK_MAX_ADAPTERS, WIPA_LORA_BANK_MAX_SEG);\n'
                    + "".join(f'printf("%zu\\n", offsetof(wipa_lora_bank_desc, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in out[0].split()] == [C.sizeof(_lib.LoraBankDesc), _lib.LORA_BANK_MAX_ADAPTERS, _lib.LORA_BANK_MAX_SEG]
    assert [int(v) for v in out[1:1 + len(fields)]] == [getattr(_lib.LoraBankDesc, f).offset for f in fields]


def _desc(**over):
    d = _lib.LoraBankDesc(x=FAKE, y=FAKE, out=FAKE, gain=FAKE, ids=FAKE, ldx=128, ld=192, M=5, K=128, N=192, r=8, n=3, rows_per_id=1, n_seg=3,
                          x_dtype=_lib.WIPA_F32, y_dtype=_lib.WIPA_F32)
    for s in (0, 2):
        d.A[s], d.B[s] = FAKE, FAKE
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_apply_refuses_before_any_launch_and_names_the_argument():
    import __graft_entry__ as g

    g.build()
    L = _lib.lib()
    for over, word in ((dict(r=6), "r = 6"), (dict(r=68), "r = 68"), (dict(r=0), "r = 0"), (dict(n=65), "n = 65"), (dict(n=0), "n = 0"),
                       (dict(M=0), "M = 0"), (dict(K=126), "K = 126"), (dict(ldx=124), "ldx = 124"), (dict(ldx=130), "ldx = 130"),
                       (dict(ld=198), "ld = 198"), (dict(ld=64), "ld = 64"), (dict(cg_in=6), "cg_in = 6"), (dict(n_seg=4), "n_seg = 4"),
                       (dict(n_seg=0), "n_seg = 0"), (dict(N=190), "N = 190"), (dict(rows_per_id=0), "rows_per_id = 0"), (dict(ids_stride=-1), "ids_stride = -1"),
                       (dict(act=2), "act = 2"), (dict(x_dtype=_lib.WIPA_FP8_E4M3), "x_dtype = 2"), (dict(y_dtype=_lib.WIPA_BF16), "y_dtype = 1"),
                       (dict(c_offset=2), "c_offset = 2"), (dict(rg_stride=6), "rg_stride = 6"), (dict(cg_stride=-2), "cg_stride = -2"),
                       (dict(x=0x1004), "x: a 16-byte aligned"), (dict(y=0), "y: a 16-byte aligned"),
                       (dict(out=0x1008), "out: a 16-byte aligned"), (dict(gain=0), "gain and ids"), (dict(ids=0), "gain and ids")):
        rc = L.wipa_lora_bank_apply(C.byref(_desc(**over)), None)
        msg = L.wipa_last_error().decode()
        assert rc == -1 and msg.startswith("wipa_lora_bank_apply: ") and word in msg, (over, msg)
    assert L.wipa_lora_bank_apply(None, None) == -1 and b"d is NULL" in L.wipa_last_error()
    d = _desc()
    d.B[2] = None
    assert L.wipa_lora_bank_apply(C.byref(d), None) == -1 and b"A[2] and B[2]: both or neither" in L.wipa_last_error()
    d = _desc()
    d.A[0] = 0x1004
    assert L.wipa_lora_bank_apply(C.byref(d), None) == -1 and b"A[0] and B[0]: 16-byte aligned" in L.wipa_last_error()
    d = _desc()
    for s in (0, 2):
        d.A[s], d.B[s] = None, None
    assert L.wipa_lora_bank_apply(C.byref(d), None) == -1 and b"no segment carries an adapter" in L.wipa_last_error()
    for bad, at in (((0, 2, -1, 3, 0), 3), ((0, -2, 1, 1, 1), 1)):
        d = _desc(ids_host=(C.c_int32 * 5)(*bad))
        assert L.wipa_lora_bank_apply(C.byref(d), None) == -1 and f"ids_host[{at}] = {bad[at]}".encode() in L.wipa_last_error()


# ---------------------------------------------------------------------------------------------------- the bank on a decode call
def test_adapter_bank_struct_and_the_calls_last_field_match_c(tmp_path):
    import __graft_entry__ as g

    g.build()
    fields = ("n", "rank", "site_mask", "A", "B", "gain", "ids_dev")
    assert tuple(f[0] for f in _lib.AdapterBankC._fields_) == fields and _lib.DecodeCall._fields_[-1][0] == "bank"
    prog = tmp_path / "lay.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wipa.h"\nint main(){\n'
                    'printf("%zu %zu %zu %d\\n", sizeof(wipa_adapter_bank), sizeof(wipa_decode_call), offsetof(wipa_decode_call, bank), WIPA_BANK_SITES);\n'
                    + "".join(f'printf("%zu\\n", offsetof(wipa_adapter_bank, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in out[0].split()] == [C.sizeof(_lib.AdapterBankC), C.sizeof(_lib.DecodeCall), _lib.DecodeCall.bank.offset, _lib.BANK_SITES]
    assert _lib.DecodeCall.bank.offset + 8 == C.sizeof(_lib.DecodeCall)  # the last field
    assert [int(v) for v in out[1:1 + len(fields)]] == [getattr(_lib.AdapterBankC, f).offset for f in fields]
    assert len(lora.SITES) == _lib.BANK_SITES


QV, CK = 0b0001010101, 1 << 5  # attn.query, attn.value, cross_attn.query, cross_attn.value | cross_attn.key


def _bank(**over):
    tab = (C.c_void_p * (2 * _lib.BANK_SITES))()
    b = _lib.AdapterBankC(**{**dict(n=3, rank=8, site_mask=0b0000010101, A=tab, B=tab, gain=FAKE, ids_dev=FAKE), **over})
    b._keep = tab
    return b


def test_decode_call_refuses_a_bank_it_cannot_serve_by_name(monkeypatch):
    import __graft_entry__ as g
    from decode_call_util import fp8_cfg, refusal, small_cfg

    g.build()
    for k in ("WIPA_DECODE_TAIL", "WIPA_DECODE_FUSED"):
        monkeypatch.delenv(k, raising=False)
    cfg, cached = small_cfg(_lib), small_cfg(_lib, dec_cross_absorbed=0)
    ok = _bank()
    for entry in ("run", "prefill"):
        assert "call.bank is not served on fp8 decoder tables" in refusal(_lib, entry, fp8_cfg(_lib), bank=C.pointer(ok))
        msg = refusal(_lib, entry, cfg, bank=C.pointer(_bank(site_mask=QV)))
        assert "call.bank targets cross_attn.key / cross_attn.value" in msg and "cfg.dec_cross_absorbed" in msg
        assert "cross_attn.key / cross_attn.value" in refusal(_lib, entry, cfg, bank=C.pointer(_bank(site_mask=CK)))
        for over, word in ((dict(n=0), "n = 0"), (dict(n=65), "n = 65"), (dict(rank=6), "rank = 6"), (dict(rank=68), "rank = 68"),
                           (dict(site_mask=0), "site_mask = 0x0"), (dict(site_mask=1 << 10), "site_mask = 0x400"), (dict(gain=0), "gain and ids_dev"),
                           (dict(ids_dev=0), "gain and ids_dev")):
            msg = refusal(_lib, entry, cached, bank=C.pointer(_bank(**over)))
            assert "call.bank" in msg and word in msg, (over, msg)
        with monkeypatch.context() as mp:
            mp.setenv("WIPA_DECODE_TAIL", "0")
            assert "call.bank needs the unfused step with the fused tail" in refusal(_lib, entry, cfg, bank=C.pointer(ok))
        with monkeypatch.context() as mp:
            mp.setenv("WIPA_DECODE_FUSED", "1")
            assert "call.bank needs the unfused step with the fused tail" in refusal(_lib, entry, cached, bank=C.pointer(ok))
    beam = dict(beam=FAKE, beam_bytes=1 << 40, beam_max_candidates=2)
    assert "call.bank is not served with call.beam" in refusal(_lib, "run", cached, **beam, bank=C.pointer(ok))


def test_adapt_cross_refusals_come_before_any_launch():
    import __graft_entry__ as g
    from decode_call_util import fp8_cfg, small_cfg

    g.build()
    L = _lib.lib()
    tab, fake = (C.c_void_p * 64)(), C.c_void_p(FAKE)
    call = lambda cfg, bank, n_rows=4, slots=None, state_bytes=1 << 40, B=4: (
        L.wipa_decoder_adapt_cross(C.byref(cfg), tab, fake, state_bytes, B, fake, n_rows, slots, C.byref(bank) if bank is not None else None, None),
        L.wipa_last_error().decode())
    cached = small_cfg(_lib, dec_cross_absorbed=0)
    for cfg, bank, kw, word in ((small_cfg(_lib), _bank(site_mask=QV), {}, "targets cross_attn.key / cross_attn.value"),
                                (fp8_cfg(_lib), _bank(site_mask=QV), {}, "fp8 decoder tables"),
                                (cached, None, {}, "bank are required"),
                                (cached, _bank(site_mask=QV, rank=5), {}, "rank = 5"),
                                (cached, _bank(site_mask=QV), dict(n_rows=3), "n_rows=3"),
                                (cached, _bank(site_mask=QV), dict(n_rows=5, slots=(C.c_int32 * 5)(0, 1, 2, 3, 0)), "n_rows=5"),
                                (cached, _bank(site_mask=QV), dict(n_rows=2, slots=(C.c_int32 * 2)(0, 4)), "slots_host[1]=4"),
                                (cached, _bank(site_mask=QV), dict(state_bytes=1024), "state blob")):
        rc, msg = call(cfg, bank, **kw)
        assert rc == -1 and msg.startswith("wipa_decoder_adapt_cross: ") and word in msg, (word, msg)
    # a bank without the two sites has nothing to add: no launch, no error (the fake pointers are never used)
    assert call(cached, _bank())[0] == 0


def test_row_adapters_is_refused_by_name_where_it_is_not_served_and_sits_before_the_sampling_fields():
    from dataclasses import fields

    from whisper_ipa_amd.decoding import DecodingOptions
    names = [f.name for f in fields(DecodingOptions)]
    assert names.index("row_adapters") == names.index("prompts") + 1 and DecodingOptions().row_adapters is None
    # transcribe_batches / TranscribePipeline (and every other path that decodes one row per clip) refuse the option by name
    from whisper_ipa_amd.decoding import _refuse_unsupported

    with pytest.raises(NotImplementedError, match="row_adapters .* is served by decode\\(\\) and decode_continuous\\(\\) only"):
        _refuse_unsupported(DecodingOptions(row_adapters=["tr"]))
    # transcribe() without a model that has a bank: refused before any audio is read
    from whisper_ipa_amd.transcribe import transcribe

    with pytest.raises(NotImplementedError, match="served by the model's own decoder on a model with an adapter bank"):
        transcribe(None, np.zeros(16000, dtype=np.float32), decode_fn=lambda *a, **k: [], row_adapters=["tr"])


def test_evaluate_model_adapter_bank_argument_and_the_samples_adapters():
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("evaluate_model_script", os.path.join(ROOT, "scripts", "evaluate_model.py"))
    ev = importlib.util.module_from_spec(spec)
    sys.modules["evaluate_model_script"] = ev
    spec.loader.exec_module(ev)
    assert ev.parse_adapter_bank("fi=/a/fi, de=/b/de") == {"fi": "/a/fi", "de": "/b/de"} and list(ev.parse_adapter_bank("tr=x,fi=y")) == ["tr", "fi"]
    for bad, word in (("fi", "is not lang=DIR"), ("fi=", "is not lang=DIR"), ("fi=a,fi=b", "given twice"), (" , ", "no lang=DIR pair")):
        with pytest.raises(ValueError, match=word):
            ev.parse_adapter_bank(bad)
    samples = [dict(locale="fi"), dict(locale="ta"), dict(language="de"), dict()]
    assert ev.sample_adapters(samples, {"fi": "a", "de": "b"}) == ["fi", None, "de", None]
