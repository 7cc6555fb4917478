"""CPU: the host half of device-side PER / PFER scoring (whisper_ipa_amd/scoring.py, scripts/evaluate_ipa.py with
scoring="device"): the feature code, the packer, the argument checks of wipa_edit_distance_batch that precede its launch, the
closed form of the diagnostic counts, and the refusal to run without a GPU.  The kernel itself: tests/test_gpu_scoring.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    return _lib


@pytest.fixture()
def ev():
    import evaluate_ipa

    yield evaluate_ipa
    evaluate_ipa.set_feature_table(None)


class _Table:
    """seeded 24-feature table over single-character phones; phones outside it are unknown (zero vector)"""

    def __init__(self, phones, seed=0):
        rng = np.random.default_rng(seed)
        self.v = {p: rng.integers(-1, 2, 24).tolist() for p in phones}
        self.lookups = []

    def word_to_vector_list(self, word, numeric=True):
        self.lookups.append(word)
        return [self.v[word]] if word in self.v else []


def _int_distances(pack):
    """the kernel's two recurrences restated in numpy on a pack's ids and codes"""
    from whisper_ipa_amd.scoring import decode_features

    feats = np.array([decode_features(int(c)) for c in pack.codes])
    per, pf = [], []
    for k in range(pack.P):
        r = pack.ref_ids[pack.ref_off[k]: pack.ref_off[k + 1]]
        h = pack.hyp_ids[pack.hyp_off[k]: pack.hyp_off[k + 1]]
        a, b = np.arange(len(h) + 1), 24 * np.arange(len(h) + 1)
        for i, x in enumerate(r, 1):
            na, nb = [i], [24 * i]
            for j, y in enumerate(h, 1):
                na.append(min(a[j] + 1, na[-1] + 1, a[j - 1] + int(x != y)))
                nb.append(min(b[j] + 24, nb[-1] + 24, b[j - 1] + int((feats[x] != feats[y]).sum())))
            a, b = na, nb
        per.append(a[-1])
        pf.append(b[-1] if pack.has_features else 24 * a[-1])
    return np.array(per, dtype=np.int64), np.array(pf, dtype=np.int64)


def test_encode_features_round_trips_and_refuses_other_values():
    from whisper_ipa_amd.scoring import decode_features, encode_features

    rng = np.random.default_rng(1)
    for _ in range(50):
        v = rng.integers(-1, 2, 24).tolist()
        code = encode_features(v)
        assert 0 <= code < 1 << 48 and decode_features(code) == v
        assert encode_features(np.array(v, dtype=np.float64)) == code  # PFERCalculator hands out float zeros for unknown phones
    assert encode_features([0] * 24) == 0
    # two codes differ in a feature's bit pair exactly where the values differ: what the kernel's popcount counts
    a, b = rng.integers(-1, 2, 24), rng.integers(-1, 2, 24)
    x = encode_features(a) ^ encode_features(b)
    assert bin((x | x >> 1) & 0x555555555555).count("1") == int((a != b).sum())
    for bad in ([0] * 23 + [2], [0] * 23, [0] * 25, [0.5] + [0] * 23):
        with pytest.raises(ValueError):
            encode_features(bad)


def test_pack_ids_offsets_and_order_of_a_hand_written_batch():
    from whisper_ipa_amd.scoring import MAX_LEN, ScorePack

    calls = []

    def features(phone):
        calls.append(phone)
        return [1 if phone == "a" else 0] * 24

    refs = [["a", "b", "a"], ["c"], ["a"] * (MAX_LEN + 1), ["b", "b", "c", "d"], ["a"] * MAX_LEN]
    hyps = [["b", "a"], [], ["a"], ["d", "b", "b"], ["e"]]
    pack = ScorePack(refs, hyps, features, pin=False)
    assert pack.n_total == 5 and pack.P == 4 and pack.kept.tolist() == [0, 1, 3, 4]  # pair 2 is over the cap: left out
    assert pack.vocab == ["a", "b", "c", "d", "e"] and calls == pack.vocab  # first appearance; ONE lookup per distinct phone
    assert pack.ref_off.tolist() == [0, 3, 4, 8, 8 + MAX_LEN] and pack.hyp_off.tolist() == [0, 2, 2, 5, 6]
    assert pack.ref_ids[:8].tolist() == [0, 1, 0, 2, 1, 1, 2, 3] and (pack.ref_ids[8:] == 0).all()
    assert pack.hyp_ids.tolist() == [1, 0, 3, 1, 1, 4]
    assert pack.order.tolist() == [3, 2, 0, 1]  # m n = 6, 0, 12, 1024 -> descending
    assert pack.n_phones == 5 and pack.codes.tolist() == [0x555555555555, 0, 0, 0, 0]
    # the views are the buffer: one copy carries everything
    raw = pack.buffer.numpy()
    o = pack.offsets
    assert raw[o["hyp_off"]: o["hyp_off"] + 20].view(np.int32).tolist() == pack.hyp_off.tolist()
    assert raw[o["codes"]:].view(np.uint64).tolist() == pack.codes.tolist() and o["codes"] % 8 == 0
    # PER only: no lookups, codes stay zero; an empty call packs to nothing
    calls.clear()
    assert not ScorePack(refs, hyps, None, pin=False).has_features and not calls
    empty = ScorePack([], [], features, pin=False)
    assert empty.P == 0 and empty.n_phones == 1 and empty.ref_off.tolist() == [0]
    with pytest.raises(ValueError):
        ScorePack(refs, hyps[:2], None, pin=False)


def test_entry_point_checks_the_host_offsets_before_any_launch(built):
    """null device pointers: every refusal below happens before the library would touch them"""
    lib = built.lib()
    cap = built.SCORE_MAX_LEN

    def call(ref_off, hyp_off, n_pairs=None, n_phones=3):
        r, h = (C.c_int32 * len(ref_off))(*ref_off), (C.c_int32 * len(hyp_off))(*hyp_off)
        n = len(ref_off) - 1 if n_pairs is None else n_pairs
        rc = lib.wipa_edit_distance_batch(None, None, None, None, None, n, None, n_phones, r, h, None, None, None)
        return rc, lib.wipa_last_error().decode()

    rc, msg = call([0, 3, 2], [0, 1, 2])
    assert rc == -1 and "pair 1" in msg and "decreasing" in msg  # WIPA_ERR_ARG
    rc, msg = call([0, 3, 4], [0, 5, 4])
    assert rc == -1 and "pair 1" in msg
    rc, msg = call([1, 3], [0, 1])
    assert rc == -1 and "pair 0" in msg and "not 0" in msg
    rc, msg = call([0, 2, 2 + cap + 1], [0, 1, 2])
    assert rc == -1 and "pair 1" in msg and str(cap) in msg
    rc, msg = call([0, 1], [0, cap + 1])
    assert rc == -1 and "pair 0" in msg
    assert call([0], [0], n_pairs=-1)[0] == -1 and call([0, 1], [0, 1], n_phones=0)[0] == -1
    assert call([0], [0], n_pairs=0, n_phones=1)[0] == 0  # nothing to do: success without a launch
    rc, msg = call([0, cap], [0, cap])  # valid lengths: only now are the (null) device pointers looked at
    assert rc == -1 and "null pointer" in msg


def _seeded_strings(rng, alphabet, n_pairs, max_len):
    refs, hyps = [], []
    for _ in range(n_pairs):
        r = "".join(rng.choice(alphabet, int(rng.integers(0, max_len + 1))))
        h = [c for c in r if rng.random() > 0.1]
        h = [str(rng.choice(alphabet)) if rng.random() < 0.25 else c for c in h]
        for _ in range(int(rng.integers(0, 3))):
            h.insert(int(rng.integers(0, len(h) + 1)), str(rng.choice(alphabet)))
        refs.append(r)
        hyps.append("".join(h))
    return refs, hyps


def _check_closed_form(ev, refs, hyps):
    host = ev.evaluate_batch(refs, hyps)
    for key in ("pfer_unknown_phones", "pfer_base_fallback_phones"):
        total = {}
        for r, h in zip(refs, hyps):
            r, h = ev.tokenize_ipa(r), ev.tokenize_ipa(h)
            if r:
                for p, k in ev.pair_lookup_counts(r, h, set(host[key])).items():
                    total[p] = total.get(p, 0) + k
        assert total == host[key], key
    return host


def test_closed_form_lookup_counts_equal_the_host_loops(ev, tmp_path):
    rng = np.random.default_rng(5)
    known = list("abcdefghijkl")
    ev.set_feature_table(_Table(known))
    refs, hyps = _seeded_strings(rng, np.array(known + list("wxyz")), 24, 14)
    host = _check_closed_form(ev, refs, hyps)
    assert set(host["pfer_unknown_phones"]) == set("wxyz") and not host["pfer_base_fallback_phones"]
    # a phone outside the flagged set, or one the DP never compares with a different phone, is not reported
    assert ev.pair_lookup_counts(list("wa"), list("wa"), {"w", "q"}) == {"w": 2}
    assert ev.pair_lookup_counts(list("ww"), list("w"), {"w"}) == {} and ev.pair_lookup_counts(list("w"), [], {"w"}) == {}

    rows = [["ipa"] + [f"f{i}" for i in range(24)]] + [[p] + list(rng.choice(["+", "-", "0"], 24)) for p in "pbta"]
    path = tmp_path / "ipa_all.csv"
    path.write_text("\n".join(",".join(r) for r in rows) + "\n", encoding="utf-8")
    ev.set_feature_table(ev.CsvFeatureTable(str(path)))
    alphabet = np.array(["p", "b", "t", "a", "pʼ", "bʰ", "ã", "z", "q"])  # three base fallbacks, two unknown
    refs, hyps = [], []
    for _ in range(16):
        refs.append("".join(rng.choice(alphabet, int(rng.integers(0, 10)))))
        hyps.append("".join(rng.choice(alphabet, int(rng.integers(0, 10)))))
    host = _check_closed_form(ev, refs, hyps)
    assert set(host["pfer_base_fallback_phones"]) == {"pʼ", "bʰ", "ã"} and set(host["pfer_unknown_phones"]) == {"z", "q"}


def test_device_path_host_half_equals_host_scoring_with_the_kernel_restated(ev, monkeypatch):
    """evaluate_batch(scoring="device") with the launch replaced by the same integer recurrences in numpy: everything around
    the kernel -- empty-reference rule, one lookup per distinct phone, counters cleared and refilled by the closed form, pairs over
    the cap scored by the host functions, the final divisions -- gives the host's result dict."""
    import torch
    from whisper_ipa_amd import scoring

    def fake_launch(refs, hyps=None, features=None):
        return scoring.ScoreHandle(scoring.ScorePack(refs, hyps, features, pin=False), None, None, None)

    def fake_collect(handle):
        per, pf = np.full(handle.pack.n_total, -1, dtype=np.int64), np.full(handle.pack.n_total, -1, dtype=np.int64)
        per[handle.pack.kept], pf[handle.pack.kept] = _int_distances(handle.pack)
        return per, pf

    monkeypatch.setattr(scoring, "score_launch", fake_launch)
    monkeypatch.setattr(scoring, "score_collect", fake_collect)
    monkeypatch.setattr(scoring, "MAX_LEN", 12)  # a cap the seeded batch crosses, so that the fallback is exercised cheaply
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    rng = np.random.default_rng(9)
    known = list("abcdefghijkl")
    table = _Table(known)
    ev.set_feature_table(table)
    refs, hyps = _seeded_strings(rng, np.array(known + list("wxyz")), 24, 16)
    refs, hyps = refs + ["", "", "abc"], hyps + ["", "ab", ""]
    host = ev.evaluate_batch(refs, hyps)
    table.lookups.clear()
    dev = ev.evaluate_batch(refs, hyps, scoring="device")
    assert dev["device_fallback_pairs"] == sum(1 for r, h in zip(refs, hyps) if r and max(len(r), len(h)) > 12) > 0
    assert dev["per_scores"] == host["per_scores"] and dev["per"] == host["per"] and dev["per_std"] == host["per_std"]
    assert np.abs(np.array(dev["pfer_scores"]) - np.array(host["pfer_scores"])).max() < 1e-9
    assert abs(dev["pfer"] - host["pfer"]) < 1e-9 and abs(dev["pfer_std"] - host["pfer_std"]) < 1e-9
    for key in ("num_samples", "pfer_is_per_fallback", "pfer_unknown_phones", "pfer_base_fallback_phones"):
        assert dev[key] == host[key], key
    assert set(dev) == set(host) | {"device_fallback_pairs"}
    # no table: PER in the pfer slot, as on the host
    ev.set_feature_table(None)
    if ev.evaluate_batch([], [])["pfer_is_per_fallback"]:  # no panphon / WIPA_PANPHON_CSV in this environment
        dev = ev.evaluate_batch(refs, hyps, scoring="device")
        assert dev["pfer_is_per_fallback"] and dev["pfer_scores"] == dev["per_scores"] == ev.evaluate_batch(refs, hyps)["per_scores"]
    # a table with a value outside -1 / 0 / +1 cannot be encoded: the whole call is scored on the host
    odd = _Table(known)
    odd.v["a"] = [2] + [0] * 23
    ev.set_feature_table(odd)
    dev = ev.evaluate_batch(refs, hyps, scoring="device")
    assert "device_fallback_pairs" not in dev and dev["pfer_scores"] == ev.evaluate_batch(refs, hyps)["pfer_scores"]


def test_device_scoring_without_a_gpu_is_an_error(ev, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError):
        ev.evaluate_batch(["kæt"], ["kat"], scoring="device")
    with pytest.raises(ValueError):
        ev.evaluate_batch(["kæt"], ["kat"], scoring="gpu")
    assert ev.evaluate_batch(["kæt"], ["kat"], scoring="host") == ev.evaluate_batch(["kæt"], ["kat"])
