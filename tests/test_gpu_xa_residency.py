"""The xa residency policy of the absorbed cross-attention's streaming kernels is a cache hint: the first groups of every frame
split load with the default policy, the rest nt -- the same bytes in the same order into the same LDS image.  So every setting
of WIPA_XA_RESIDENT_MB must give the same BITS: all groups default policy (-1), all groups nt (0), and budgets that put the
boundary inside a split and inside a wave's stride of three groups.  The variable is read once per process: one fresh process
per setting, their outputs compared with equality."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ("-1", "0", "2", "3")

WORKER = r'''
import ctypes as C
import os
import sys
import torch
import whisper_ipa_amd as wipa
from whisper_ipa_amd import _lib
from whisper_ipa_amd.runtime import ptr
from oracle import whisper_ref as R

L = _lib.lib()
out = {}
B = 3
g = torch.Generator().manual_seed(11)
for d in (768, 512, 1024):  # independent waves (3 per workgroup) at 768 and 512, the channel-split form at 1024
    H = d // 64
    _lib.check(L.wipa_cross_absorbed_init(d))
    q = (torch.randn(B, d, generator=g) * 0.3).bfloat16().cuda()
    wkT = (torch.randn(d, d, generator=g) * 0.05).bfloat16().cuda()
    wv = (torch.randn(d, d, generator=g) * 0.05).bfloat16().cuda()
    bv = torch.zeros(d).cuda()
    for Tk in (1500, 1496, 40):  # 1496 and 40: the last 16-frame group hangs over the end of the clip
        xa = torch.randn(B, Tk, d, generator=g).bfloat16().cuda()
        for splits in (1, 2, 4):
            S = L.wipa_cross_absorbed_splits(splits, Tk)
            nbytes = L.wipa_cross_absorbed_scratch_bytes(B, d, Tk)
            scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            o = torch.empty(B, d, dtype=torch.bfloat16, device="cuda")
            _lib.check(L.wipa_cross_absorbed_attention(ptr(q), d, ptr(wkT), ptr(xa), ptr(wv), ptr(bv), ptr(o), d, ptr(scratch), nbytes,
                                                       B, H, d, Tk, 64 ** -0.25, splits, None))
            torch.cuda.synchronize()
            parts = scratch[B * 16 * d * 2:].clone()
            parts[: B * S * 16 * (2 + d) * 4] = 0  # the streaming launch alone must rewrite all of it
            scratch[B * 16 * d * 2:] = parts
            _lib.check(L.wipa_cross_absorbed_stream(ptr(xa), ptr(scratch), nbytes, B, H, d, Tk, splits, None))
            torch.cuda.synchronize()
            f = scratch[B * 16 * d * 2: B * 16 * d * 2 + B * S * 16 * (2 + d) * 4].view(torch.float32).cpu()
            n = B * S * 16
            key = f"{d}_{Tk}_{splits}"
            out[key + "_m"], out[key + "_l"], out[key + "_o"] = f[:n].clone(), f[n:2 * n].clone(), f[2 * n:].clone()
            out[key + "_out"] = o.cpu()
            out[key + "_rg"] = torch.tensor([L.wipa_cross_absorbed_resident_groups(B, d, Tk, splits), 2 * ((((Tk + 31) // 32) + S - 1) // S)])

# a short greedy decode through the pipeline, two passes in flight (whisper-small's width, two layers)
from whisper_ipa_amd.whisper import ModelDimensions, Whisper
dims = R.ModelDimensions(80, 1500, 768, 12, 2, 51865, 448, 768, 12, 2)
m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.bfloat16)
m.load_weights(R.synthetic_weights(dims, seed=5))
gen = torch.Generator().manual_seed(2)
batches = [torch.randn(3, 1500, 768, generator=gen).bfloat16().cuda() for _ in range(4)]
opts = wipa.DecodingOptions(language="en", without_timestamps=True)
res = list(wipa.transcribe_batches(m, batches, opts, passes_in_flight=2, max_new_tokens=6, stop_on_eot=False))
out["ids"] = torch.stack([torch.as_tensor(r.tokens) for r in res])
torch.save(out, sys.argv[1])
print("OK")
'''


def _run(setting, path):
    env = dict(os.environ, WIPA_XA_RESIDENT_MB=setting, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", WORKER, path], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "OK" in r.stdout, f"WIPA_XA_RESIDENT_MB={setting}\n" + r.stderr[-3000:] + r.stdout[-500:]
    return torch.load(path)


def test_partials_and_pipeline_ids_are_bit_identical_for_every_residency_setting(tmp_path):
    runs = {s: _run(s, str(tmp_path / f"xa_res_{s.replace('-', 'm')}.pt")) for s in SETTINGS}
    base = runs["-1"]
    keys = sorted(base)
    assert len([k for k in keys if k.endswith("_o")]) == 27 and "ids" in keys
    # the settings are what they claim: every group / no group / a boundary inside the split, off the three-wave stride
    inside = off_stride = 0
    for k in keys:
        if not k.endswith("_rg"):
            continue
        gps = int(base[k][1])
        assert int(base[k][0]) == gps and int(runs["0"][k][0]) == 0, k
        for s in ("2", "3"):
            rg = int(runs[s][k][0])
            assert 0 <= rg <= gps
            if k.startswith("768_") and 0 < rg < gps:
                inside += 1
                off_stride += rg % 3 != 0
    assert inside >= 12 and off_stride >= 8, (inside, off_stride)  # d = 768, Tk 1500 / 1496, three split counts, two budgets
    for s in SETTINGS[1:]:
        for k in keys:
            if k.endswith("_rg"):
                continue
            a, b = base[k], runs[s][k]
            assert a.dtype == b.dtype and a.shape == b.shape, (s, k)
            same = torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16) if a.dtype == torch.bfloat16 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16) if b.dtype == torch.bfloat16 else b)
            assert same, f"WIPA_XA_RESIDENT_MB={s}: {k} differs from the all-default-policy run"
    # not vacuous: the partials are finite numbers that differ between shapes, and the decode produced ids
    assert torch.isfinite(base["768_1500_2_o"]).all() and base["768_1500_2_o"].abs().max() > 0
    assert not torch.equal(base["768_1500_2_l"], base["768_1496_2_l"])
    assert base["ids"].shape[0] == 4 and base["ids"].shape[1] == 3
