"""The xa residency rule of the absorbed cross-attention (csrc/cross_absorbed.hip): how many 16-frame groups of every frame
split keep the default cache policy, from a byte budget per pass.  Host arithmetic only: no GPU."""
import os
import subprocess
import sys

import pytest

from whisper_ipa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(B, d, Tk, S) for B in (1, 3, 64, 256) for d in (384, 512, 768, 1024) for Tk in (40, 100, 1496, 1500) for S in (0, 1, 2, 3, 4)]


def _groups_per_split(Tk, S):
    tiles = (Tk + 31) // 32
    return 2 * ((tiles + S - 1) // S)


def test_rule_is_zero_at_zero_whole_at_minus_one_and_at_the_pass_size_and_monotone():
    L = _lib.lib()
    rule = L.wipa_cross_absorbed_resident_groups_for
    for B, d, Tk, want in SHAPES:
        S = L.wipa_cross_absorbed_splits(want, Tk)
        gps = _groups_per_split(Tk, S)
        xa = B * Tk * d * 2
        assert rule(B, d, Tk, want, 0) == 0
        assert rule(B, d, Tk, want, -1) == gps
        assert rule(B, d, Tk, want, xa) == gps and rule(B, d, Tk, want, 4 * xa) == gps and rule(B, d, Tk, want, 1 << 40) == gps
        unit = B * S * 16 * d * 2  # one more group in every split of every clip
        prev = 0
        for k in range(0, 64):
            budget = xa * k // 60
            got = rule(B, d, Tk, want, budget)
            assert prev <= got <= gps, (B, d, Tk, want, budget)  # monotone, never more than the split has
            if budget < xa:
                assert got == min(gps, budget // unit)
            prev = got
        assert rule(B, d, Tk, want, unit - 1) == 0 and rule(B, d, Tk, want, unit) == min(gps, 1)
        # the resolved split count and the request that resolves to it give the same answer
        assert rule(B, d, Tk, S, xa // 3) == rule(B, d, Tk, want, xa // 3)


def test_rule_never_exceeds_a_short_inputs_groups():
    L = _lib.lib()
    for B in (1, 3, 64):
        for d in (384, 768, 1024):
            for want in range(5):
                S = L.wipa_cross_absorbed_splits(want, 40)
                assert S == 1  # two 32-frame tiles: one split
                for budget in (-1, 0, 1, 10 ** 5, 10 ** 6, 10 ** 9):
                    assert 0 <= L.wipa_cross_absorbed_resident_groups_for(B, d, 40, want, budget) <= 4


def test_rule_depends_on_the_calls_shape_only():
    """Same arguments, same answer, whatever was asked before (no state), and the process-wide form is the rule at the process's
    budget: a function of (B, d, Tk, n_splits)."""
    L = _lib.lib()
    first = [L.wipa_cross_absorbed_resident_groups(*s) for s in SHAPES]
    mid = [L.wipa_cross_absorbed_resident_groups_for(*s, 10 ** 7) for s in SHAPES]
    assert [L.wipa_cross_absorbed_resident_groups(*s) for s in reversed(SHAPES)] == first[::-1]
    assert [L.wipa_cross_absorbed_resident_groups_for(*s, 10 ** 7) for s in SHAPES] == mid


@pytest.mark.parametrize("mb", ["-1", "0", "48", "148"])
def test_environment_budget_is_the_rule_at_that_many_megabytes(mb):
    """WIPA_XA_RESIDENT_MB is read once per process: a fresh process per value."""
    code = r'''
import os
from whisper_ipa_amd import _lib
L = _lib.lib()
mb = int(os.environ["WIPA_XA_RESIDENT_MB"])
for B, d, Tk, S in ((64, 768, 1500, 2), (64, 768, 1500, 4), (64, 768, 1500, 0), (3, 512, 1496, 1), (256, 1024, 1500, 2), (5, 384, 40, 0)):
    want = L.wipa_cross_absorbed_resident_groups_for(B, d, Tk, S, -1 if mb < 0 else mb * 10 ** 6)
    assert L.wipa_cross_absorbed_resident_groups(B, d, Tk, S) == want, (B, d, Tk, S)
print("OK", L.wipa_cross_absorbed_resident_groups(64, 768, 1500, 2))
'''
    env = dict(os.environ, WIPA_XA_RESIDENT_MB=mb, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:] + r.stdout[-500:]
    got = int(r.stdout.split()[-1])
    assert got == {"-1": 48, "0": 0, "48": 15, "148": 48}[mb]  # 64 clips x 2 splits x 24 KiB = 3.1 MB per group index
