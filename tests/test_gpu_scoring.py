"""GPU: device-side PER / PFER scoring (csrc/score.hip through whisper_ipa_amd.scoring and evaluate_batch(scoring="device"))
against the project's host functions -- ``edit_distance`` and ``PFERCalculator`` of scripts/evaluate_ipa.py.  ``pytest -m gpu``
on an MI355X.

Tolerances: the kernel works in integers, so PER (the host's own expression on the same integer) must be bit-equal.  The host
PFER sums k/24 terms in float64 along the DP; against the exact pfer24 / 24 / m * 100 that leaves rounding of order 1e-14 at
these lengths, and the tests use the 1e-9 absolute that tests/test_host_logic.py uses for the same values."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
KNOWN = [chr(0x100 + i) for i in range(90)]       # single-codepoint letters: one phone each under the Unicode rule
UNKNOWN = [chr(0x100 + 90 + i) for i in range(4)]  # not in the table: zero vector
CAP = 1024


class _Table:
    """seeded 24-feature table; phones outside it are unknown"""

    def __init__(self, phones, seed=0):
        rng = np.random.default_rng(seed)
        self.v = {p: rng.integers(-1, 2, 24).tolist() for p in phones}

    def word_to_vector_list(self, word, numeric=True):
        return [self.v[word]] if word in self.v else []


@pytest.fixture()
def ev():
    """scripts/evaluate_ipa.py with the seeded table of 90 phones installed"""
    import evaluate_ipa

    evaluate_ipa.set_feature_table(_Table(KNOWN))
    yield evaluate_ipa
    evaluate_ipa.set_feature_table(None)


def _phones(rng, n, alphabet=None):
    return [str(p) for p in rng.choice(np.array(KNOWN + UNKNOWN if alphabet is None else alphabet), n)]


def _noisy(rng, ref, n=None):
    """a hypothesis for ``ref``: about 15 % substitutions / deletions / insertions, then cut or extended to ``n`` phones"""
    hyp = []
    for p in ref:
        u = rng.random()
        if u < 0.05:
            continue
        hyp.append(_phones(rng, 1)[0] if u < 0.12 else p)
        if u > 0.97:
            hyp.append(_phones(rng, 1)[0])
    if n is not None:
        hyp = hyp[:n] + _phones(rng, max(0, n - len(hyp)))
    return hyp


def _device(ev, refs, hyps, features=True):
    from whisper_ipa_amd import scoring

    per, pf = scoring.score_pairs(refs, hyps, ev.get_pfer_calculator().get_phone_features if features else None)
    assert per.dtype == np.int64 and pf.dtype == np.int64 and len(per) == len(pf) == len(refs)
    return per, pf


def _assert_results_equal(dev, host):
    assert dev["per_scores"] == host["per_scores"]  # bit-equal
    assert dev["per"] == host["per"] and dev["per_std"] == host["per_std"] and dev["num_samples"] == host["num_samples"]
    assert len(dev["pfer_scores"]) == len(host["pfer_scores"])
    if host["pfer_scores"]:
        assert np.abs(np.array(dev["pfer_scores"]) - np.array(host["pfer_scores"])).max() < 1e-9
    assert abs(dev["pfer"] - host["pfer"]) < 1e-9 and abs(dev["pfer_std"] - host["pfer_std"]) < 1e-9
    assert dev["pfer_is_per_fallback"] == host["pfer_is_per_fallback"]
    assert dev["pfer_unknown_phones"] == host["pfer_unknown_phones"]
    assert dev["pfer_base_fallback_phones"] == host["pfer_base_fallback_phones"]


def test_random_pairs_equal_host_evaluate_batch(ev):
    rng = np.random.default_rng(11)
    refs, hyps = [], []
    for k in range(64):
        ref = _phones(rng, int(rng.integers(0, 41)))
        hyp = _noisy(rng, ref) if k % 2 else _phones(rng, int(rng.integers(0, 41)))
        refs.append("".join(ref))
        hyps.append("".join(hyp))
    refs[5], hyps[5] = "", ""  # the reference's empty-reference rule, both ways
    refs[6] = ""
    assert hyps[6]
    host = ev.evaluate_batch(refs, hyps)
    dev = ev.evaluate_batch(refs, hyps, scoring="device")
    _assert_results_equal(dev, host)
    assert dev["device_fallback_pairs"] == 0 and set(dev) == set(host) | {"device_fallback_pairs"}
    assert set(host["pfer_unknown_phones"]) == set(UNKNOWN) and host["pfer"] > 0 and host["pfer"] < host["per"]


def test_lane_chunk_boundaries_against_the_host_functions(ev):
    """lengths around the 64-column chunks of the kernel, an empty hypothesis, identical sequences, nothing in common"""
    rng = np.random.default_rng(12)
    refs, hyps = [], []
    for m, n in ((1, 1), (1, 64), (64, 1), (63, 63), (64, 64), (65, 65), (64, 129), (129, 64), (128, 128)):
        ref = _phones(rng, m)
        refs.append(ref)
        hyps.append(_noisy(rng, ref, n))
    refs.append(_phones(rng, 5))
    hyps.append([])
    same = _phones(rng, 70)
    refs.append(same)
    hyps.append(list(same))
    refs.append(_phones(rng, 66, KNOWN[:40]))
    hyps.append(_phones(rng, 70, KNOWN[40:]))
    per, pf = _device(ev, refs, hyps)
    calc = ev.get_pfer_calculator()
    for k, (ref, hyp) in enumerate(zip(refs, hyps)):
        assert per[k] == ev.edit_distance(ref, hyp), (k, len(ref), len(hyp))
        want = calc.phone_feature_error_rate("".join(ref), "".join(hyp))
        assert abs(pf[k] / 24.0 / len(ref) * 100.0 - want) < 1e-9, (k, len(ref), len(hyp))
    assert (per[9], pf[9]) == (5, 120) and (per[10], pf[10]) == (0, 0) and per[11] == 70
    # PER only: no codes on the device, pfer24 = 24 per_dist
    per0, pf0 = _device(ev, refs, hyps, features=False)
    assert np.array_equal(per0, per) and np.array_equal(pf0, 24 * per)


def test_pairs_at_the_length_cap(ev):
    from whisper_ipa_amd import scoring

    assert scoring.MAX_LEN == CAP
    rng = np.random.default_rng(13)
    table = ev.get_pfer_calculator().ft.v
    dist = lambda a, b: sum(x != y for x, y in zip(table[a], table[b]))  # noqa: E731
    ref = _phones(rng, CAP, KNOWN)
    free = _phones(rng, CAP, KNOWN)  # unrelated to ref: PER against the host's edit_distance
    # ref with k substitutions at spread positions (each by a phone at a known feature distance 1..24) and t deletions at the end:
    # the alignment that pays exactly those is optimal here -- any other shifts ~1000 unrelated phones against each other
    k_subs, t_del = 37, 9
    subst, want = list(ref), 0
    for pos in np.linspace(3, CAP - t_del - 5, k_subs).astype(int):
        other = next(p for p in _phones(rng, 50, KNOWN) if p != ref[pos])
        assert 1 <= dist(ref[pos], other) <= 24
        subst[pos] = other
        want += dist(ref[pos], other)
    refs = [ref, ref, ref, ref]
    hyps = [free, [ref[0]], subst, subst[:CAP - t_del]]
    per, pf = _device(ev, refs, hyps)
    assert per[0] == ev.edit_distance(ref, free)      # 1024 x 1024
    assert (per[1], pf[1]) == (CAP - 1, 24 * (CAP - 1))  # 1024 x 1: one match, the rest deleted
    assert (per[2], pf[2]) == (k_subs, want)           # 1024 x 1024, known answer
    assert (per[3], pf[3]) == (k_subs + t_del, want + 24 * t_del)
    assert 0 < pf[0] <= 24 * per[0]
    # one phone over the cap: the pair stays off the device and is scored by the host functions
    long_ref, short = "".join(ref + [KNOWN[0]]), "".join(ref[:2] + [UNKNOWN[0]])
    refs_s, hyps_s = ["".join(ref[:30]), long_ref, short], ["".join(subst[:28]), short, long_ref]
    host = ev.evaluate_batch(refs_s[:2], hyps_s[:2])
    dev = ev.evaluate_batch(refs_s[:2], hyps_s[:2], scoring="device")
    assert dev["device_fallback_pairs"] == 1
    _assert_results_equal(dev, host)
    per, pf = scoring.score_pairs([list(r) for r in refs_s], [list(h) for h in hyps_s], None)
    assert per[0] >= 0 and per[1] == pf[1] == -1 and per[2] == pf[2] == -1  # either side over the cap


def test_no_feature_table_gives_per_in_the_pfer_slot(ev, monkeypatch):
    monkeypatch.setattr(ev, "_ft", None)
    monkeypatch.setattr(ev, "_ft_loaded", True)  # discovery done, nothing found
    monkeypatch.setattr(ev, "_pfer_calc", None)
    rng = np.random.default_rng(14)
    refs = ["".join(_phones(rng, int(rng.integers(1, 30)))) for _ in range(12)]
    hyps = ["".join(_noisy(rng, list(r))) for r in refs]
    host = ev.evaluate_batch(refs, hyps)
    dev = ev.evaluate_batch(refs, hyps, scoring="device")
    assert dev["pfer_is_per_fallback"] is True and dev["pfer_scores"] == dev["per_scores"] == host["per_scores"]
    assert dev["pfer"] == dev["per"] == host["per"] and dev["pfer_unknown_phones"] == {} and max(dev["per_scores"]) > 0


def test_more_pairs_than_one_grid_wave_and_any_order(ev):
    """1100 short pairs in one launch (more workgroups than compute units), and the same pairs shuffled: a pair's integers do
    not depend on where it sits in the batch"""
    rng = np.random.default_rng(15)
    refs = [_phones(rng, int(rng.integers(0, 9)), KNOWN[:12]) for _ in range(1100)]
    hyps = [_phones(rng, int(rng.integers(0, 9)), KNOWN[:12]) for _ in range(1100)]
    per, pf = _device(ev, refs, hyps)
    assert per.tolist() == [ev.edit_distance(r, h) for r, h in zip(refs, hyps)]
    assert (pf <= 24 * per).all() and (pf >= 0).all() and (pf < 24 * per).any()
    perm = rng.permutation(1100)
    per_s, pf_s = _device(ev, [refs[i] for i in perm], [hyps[i] for i in perm])
    assert np.array_equal(per_s, per[perm]) and np.array_equal(pf_s, pf[perm])
    # and longer pairs of mixed lengths, whose launch order (m n descending) changes with the shuffle
    refs = [_phones(rng, int(rng.integers(1, 150))) for _ in range(40)]
    hyps = [_noisy(rng, r) for r in refs]
    per, pf = _device(ev, refs, hyps)
    perm = rng.permutation(40)
    per_s, pf_s = _device(ev, [refs[i] for i in perm], [hyps[i] for i in perm])
    assert np.array_equal(per_s, per[perm]) and np.array_equal(pf_s, pf[perm]) and per.max() > 0


def _tiny_eval_setup(tmp_path):
    """a one-layer local model and four 2 s WAV clips with IPA references, as the end-to-end training test builds them"""
    from whisper_ipa_amd.load_models import save_model
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    dims = R.ModelDimensions(80, 1500, 64, 1, 1, 51865, 448, 64, 1, 1)
    m = Whisper(ModelDimensions(**dims.__dict__), dtype=torch.float32)
    m.load_weights(R.synthetic_weights(dims, seed=4))
    model_dir = tmp_path / "whisper-micro"
    save_model(m, str(model_dir))
    rng = np.random.default_rng(0)
    entries = []
    for i in range(4):
        pcm = (0.1 * rng.standard_normal(16000 * 2) * 32767).astype("<i2")
        p = tmp_path / f"c{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
        entries.append({"audio_path": str(p), "ipa_transcription": "kæt " + "ab" * (i + 1), "speaker_id": f"s{i}"})
    (tmp_path / "test.json").write_text(json.dumps(entries))
    return model_dir


def test_evaluate_model_scoring_modes_agree(tmp_path, capsys, monkeypatch):
    """scripts/evaluate_model.py end to end with --scoring device and --scoring host.  The untrained model writes an id placeholder
    per token, so at the default 224 new tokens every hypothesis is longer than the kernel's 1024 phones and the device run scores
    all four pairs through its host fallback; with the decode cut to 12 tokens all four go through the kernel."""
    import evaluate_ipa
    import evaluate_model as EM

    model_dir = _tiny_eval_setup(tmp_path)
    options = EM.DecodingOptions
    # give some of the hypotheses' characters features and leave the rest unknown
    evaluate_ipa.set_feature_table(_Table(list("kætab<|id>01234")))
    try:
        for sample_len, on_host in ((None, 4), (12, 0)):
            monkeypatch.setattr(EM, "DecodingOptions", lambda **kw: options(sample_len=sample_len, **kw))
            res = {}
            for mode in ("device", "host"):
                out = EM.main(["--checkpoint", str(tmp_path / "no-checkpoint"), "--base-model", str(model_dir), "--test-data",
                               str(tmp_path / "test.json"), "--num-samples", "0", "--n-mels", "80", "--batch-size", "2", "--skip-base",
                               "--scoring", mode, "--results-json", str(tmp_path / f"{mode}.json"), "--allow-byte-fallback"])
                res[mode] = out["trained"]
                text = capsys.readouterr().out
                assert "Trained Checkpoint - Overall Results" in text and "PFER (Phone Feature Error Rate):" in text
                assert json.load(open(tmp_path / f"{mode}.json"))["trained"]["per"] == res[mode]["per"]
            _assert_results_equal(res["device"], res["host"])
            assert res["device"]["num_samples"] == 4 and res["device"]["device_fallback_pairs"] == on_host and res["host"]["per"] > 0
            assert "device_fallback_pairs" not in res["host"] and not res["host"]["pfer_is_per_fallback"]
            assert res["host"]["pfer_unknown_phones"] and res["host"]["pfer"] < res["host"]["per"]
    finally:
        evaluate_ipa.set_feature_table(None)
