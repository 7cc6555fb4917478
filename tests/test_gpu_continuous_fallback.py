"""GPU: the temperature fallback on the continuous schedule -- a TEMPERATURE PER ROW (include/wipa.h: the sampling record with a row
part, wipa_sample_rows_set, wipa_decode_call.sample_rows and the rows_tail_continuous kernels;
whisper_ipa_amd.continuous.decode_continuous(temperatures=, attempts=); transcribe(schedule="continuous", seed=S)) against the CPU
restatements of tests/timestamp_ref.py (greedy rows) and tests/prompt_ref.py / tests/sampling_ref.py (sampled rows) with every clip
decoded ALONE -- slots, refill, neighbours at other temperatures, admission columns and shifts do not exist there.  ``pytest -m gpu`` on
an MI355X.

Fixtures: those of tests/test_gpu_continuous_rules.py, rebuilt here (MICRO, weight seed 7, eight mixes of the two fixture clips, limits
5, 27, 12, 19, 1, 22, 23, 26, 3 slots, a check every 4 steps, f32, with rules)."""
import json
import warnings
import wave

import numpy as np
import pytest
import torch

import prompt_ref as PR
import sampling_ref as SR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP = PR.MICRO, PR.W384, PR.SP
V, TB, NT, EOT = 51865, SP.timestamp_begin, SP.no_timestamps, SP.eot
INIT = [SP.sot, SP.lang_first, SP.transcribe]  # tok.sot_sequence
LENS = [5, 27, 12, 19, 1, 22, 23, 26]
SEED = 3
TEMPERATURES = [0, .2, .6, 0, 1., .4, .8, 0]
ATTEMPTS = [0, 1, 3, 0, 5, 2, 4, 0]
LENS_BF16 = [3, 20, 1, 9, 20, 11]
TEMPERATURES_BF16 = [0, .4, 1., .2, 0, .8]
ATTEMPTS_BF16 = [0, 2, 5, 1, 0, 4]
RETRY = (0, 0.8, 2)  # the C ABI test: clip 0 a second time, at this temperature and attempt


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def _weights(dims, seed, scripted):
    W = R.synthetic_weights(dims, seed=seed)
    if scripted:
        W["decoder.positional_embedding"] = TR.scripted_positional_table(W, TR.timestamp_script(dims.n_text_ctx, TB, EOT, seed=3))
    return W


def mixed_features(xa: torch.Tensor, n: int) -> torch.Tensor:
    """n different feature tensors from the two fixture clips: clip i is (1 - i / (n - 1)) xa[0] + i / (n - 1) xa[1]"""
    w = torch.linspace(0.0, 1.0, n)[:, None, None]
    return ((1 - w) * xa[0:1] + w * xa[1:2]).contiguous()


def _cut(row):
    row = [int(t) for t in row]
    return row[: row.index(EOT)] if EOT in row else row


def _rules(max_init=50):
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(TB, NT, max_init)


def _options(**kw):
    from whisper_ipa_amd.decoding import DecodingOptions

    return DecodingOptions(language="en", without_timestamps=False, fp16=False, **kw)


def _sum(r):
    return r.avg_logprob * (len(r.tokens) + 1)


def cpu_row(W, feats, i, temperature, attempt):
    """clip i alone on the CPU, to its own limit: (ids before EOT, sum_logprobs, the smallest deciding margin) -- the loop with rules at
    temperature 0, the sampling restatement on stream (i, 0) above it"""
    if temperature == 0:
        always, first = R.suppress_lists(SP)
        g = TR.greedy_with_rules(R, W, MICRO, feats[i: i + 1], INIT, always, first, EOT, TB, NT, LENS[i])
        return _cut(g.tokens[0, len(INIT):]), float(g.sum_logprobs[0]), min(float(g.margins.min()), float(g.mass_gaps.min()))
    loop = PR.sample_row_loop(W, MICRO, feats[i: i + 1], INIT, LENS[i], SEED, temperature, (i, 0), attempt=attempt, with_rules=True)
    return _cut(loop.tokens[len(INIT):]), float(loop.sum_logprob), float(loop.key_margins.min())


@pytest.fixture(scope="module")
def refs():
    """the "lively" weights, the eight clips' features and every clip alone on the CPU at ITS temperature and attempt, computed once;
    plus clip RETRY[0] at RETRY's temperature and attempt for the C ABI test, and softmax(logits at SOT)[no_speech] per clip"""
    W = _weights(MICRO, 7, False)
    with torch.no_grad():
        xa = R.encoder_forward(W, MICRO, PR.clip_mels())
    feats = mixed_features(xa, len(LENS))
    rows = [cpu_row(W, feats, i, TEMPERATURES[i], ATTEMPTS[i]) for i in range(len(LENS))]
    retry = cpu_row(W, feats, *RETRY)
    for i, (ids, slp, margin) in enumerate(rows + [retry]):
        print(f"clip {i if i < len(LENS) else RETRY}: {len(ids)} ids, sum_logprobs {slp:.5f}, smallest margin {margin:.4f}")
        # before any GPU result is compared: the restatement decides every token by more than the f32 logit error can move -- the bound
        # tests/test_gpu_continuous.py and tests/test_gpu_continuous_rules.py ask of their references
        assert margin > 5e-3, (i, margin)
    with torch.no_grad():
        sot = torch.full((feats.shape[0], 1), SP.sot, dtype=torch.long)
        no_speech = torch.softmax(R.decoder_forward(W, MICRO, sot, feats)[:, 0].float(), dim=-1)[:, SP.no_speech].numpy()
    return W, feats, rows, retry, no_speech


@pytest.fixture(scope="module")
def model(refs):
    W, feats, _, _, _ = refs
    return _model(MICRO, W, torch.float32), feats.cuda()


@pytest.fixture(scope="module")
def mixed(model):
    """the mixed-row decodes: 3 slots, 3 slots with column_limit = 40 (forced shifts), 8 slots (no refill)"""
    from whisper_ipa_amd.continuous import decode_continuous

    m, dev = model
    got = {}
    for run, kw in (("slots3", dict(slots=3)), ("shifted", dict(slots=3, column_limit=40)), ("slots8", dict(slots=8))):
        stats = []
        res = decode_continuous(m, dev, _options(seed=SEED), sample_lens=LENS, check_every=4, stats_out=stats, temperatures=TEMPERATURES,
                                attempts=ATTEMPTS, **kw)
        got[run] = (res, stats[0])
    return got


def test_mixed_rows_equal_every_clip_alone_at_its_own_temperature(refs, mixed):
    """8 clips through 3 slots, temperatures 0, .2, .6, 0, 1, .4, .8, 0 at attempts 0, 1, 3, 0, 5, 2, 4, 0, seed 3: a greedy clip's ids
    equal the CPU loop with rules on that clip alone, a sampled clip's ids the CPU draw on that clip alone at its temperature and attempt
    on stream (clip, 0); sum_logprobs within the 1e-2 of the existing continuous tests.  Greedy and sampled rows, and sampled rows at
    different temperatures, share launches: with 3 slots the first group is clips 0 (greedy), 1 (0.2) and 2 (0.6)."""
    _, _, rows, _, _ = refs
    res, stats = mixed["slots3"]
    assert len(res) == len(LENS) and stats.shifts == []
    assert [clip for _, clip, _ in stats.admissions] == list(range(8))
    assert [col for _, _, col in stats.admissions[:3]] == [0, 0, 0] and any(col > 0 for _, _, col in stats.admissions)
    for i, (r, (ids, slp, _)) in enumerate(zip(res, rows)):
        print(f"clip {i} (T {TEMPERATURES[i]}, attempt {ATTEMPTS[i]}): sum_logprobs {_sum(r):.5f} vs {slp:.5f}; ids {r.tokens}")
        assert r.tokens == ids, (i, r.tokens, ids)
        assert abs(_sum(r) - slp) < 1e-2, (i, _sum(r), slp)
        assert r.temperature == TEMPERATURES[i]


def test_mixed_rows_forced_shifts_and_the_slot_count_change_no_id(mixed):
    plain, _ = mixed["slots3"]
    shifted, stats = mixed["shifted"]
    many, stats8 = mixed["slots8"]
    assert stats.shifts and all(x > 0 for x in stats.shifts)
    assert all(0 <= col <= 40 for _, _, col in stats.admissions)
    assert all(col == 0 for _, _, col in stats8.admissions)
    for i, (x, y, z) in enumerate(zip(plain, shifted, many)):
        assert x.tokens == y.tokens, (i, x.tokens, y.tokens)
        assert x.tokens == z.tokens, (i, x.tokens, z.tokens)


def test_mixed_rows_no_speech_prob_from_the_tail(refs, mixed):
    """the no-speech store of the rules tails is kept: within 1e-3 absolute and 1e-2 relative of the CPU value, the bounds of
    tests/test_gpu_continuous_rules.py, for greedy and sampled rows alike"""
    want = refs[4]
    for run in ("slots3", "shifted"):
        for i, r in enumerate(mixed[run][0]):
            assert np.isfinite(r.no_speech_prob) and abs(r.no_speech_prob - float(want[i])) < 1e-3, (run, i, r.no_speech_prob, float(want[i]))
            assert abs(r.no_speech_prob / float(want[i]) - 1.0) < 1e-2, (run, i, r.no_speech_prob, float(want[i]))


def test_uniform_rows_equal_the_existing_paths_bit_for_bit(model):
    """same slots, same clips: every temperature 0 through the new entry point gives the ids and sum_logprobs of decode_continuous(options)
    (the rules tail), every clip at 0.6 and attempt 0 those of decode_continuous(temperature=0.6, seed=3) (the sampling rules tail) --
    the code, the logits and the order of the sums are the same, so the comparison is ==, not a tolerance"""
    from whisper_ipa_amd.continuous import decode_continuous

    m, dev = model
    n = len(LENS)
    kw = dict(slots=3, sample_lens=LENS, check_every=4)
    for name, old, new in (
            ("greedy", decode_continuous(m, dev, _options(), **kw),
             decode_continuous(m, dev, _options(seed=SEED), temperatures=[0.0] * n, **kw)),
            ("0.6", decode_continuous(m, dev, _options(temperature=0.6, seed=SEED), **kw),
             decode_continuous(m, dev, _options(seed=SEED), temperatures=[0.6] * n, attempts=[0] * n, **kw))):
        for i, (x, y) in enumerate(zip(old, new)):
            print(f"{name} clip {i}: sum_logprobs {_sum(x)!r} vs {_sum(y)!r}")
            assert x.tokens == y.tokens, (name, i, x.tokens, y.tokens)
            assert x.avg_logprob == y.avg_logprob, (name, i, x.avg_logprob, y.avg_logprob)
            assert x.no_speech_prob == y.no_speech_prob, (name, i)


def test_admit_set_rows_run_and_shift_through_the_c_abi(refs, model):
    """DeviceStepper with a row record drives admit + wipa_sample_rows_set, steps, a second admission of THE SAME clip into THE SAME slot
    at a later column with another temperature and attempt, a shift and more steps with wipa_decode_call.sample_rows, 3 slots:
    each occupancy's columns equal that clip decoded alone at that temperature and attempt, and the no-speech probability is written
    again at the retry's first column"""
    from whisper_ipa_amd.continuous import DeviceStepper
    from whisper_ipa_amd.runtime import on_stream

    _, _, rows, retry, want_ns = refs
    m, dev = model
    always, first = R.suppress_lists(SP)
    B, n_init = 3, len(INIT)

    def draw(i, temperature=None, attempt=None):
        t = TEMPERATURES[i] if temperature is None else temperature
        k = ATTEMPTS[i] if attempt is None else attempt
        return (t, k, (i, 0)) if t else None

    with on_stream() as s:
        st = DeviceStepper(m, B, lambda clip: dev[clip], lambda clip: INIT, n_init, LENS, EOT, always, first, None, s, rules=_rules(),
                           no_speech_token=SP.no_speech, row_seed=SEED)
        words = st.rows.cpu().numpy().view(np.uint32)
        assert words[:4].tolist() == [SEED, 0, B, 0] and (words[7::4] == 0).all()  # every row greedy until a clip is admitted
        st.admit([(0, 2, LENS[2], draw(2)), (2, 0, LENS[0], draw(0))])  # clip 2 at 0.6 / attempt 3, clip 0 greedy, at column 0
        words = st.rows.cpu().numpy().view(np.uint32)
        assert words[4:7].tolist() == [2, 0, ATTEMPTS[2]] and words[7:8].view(np.float32)[0] == np.float32(1.0) / np.float32(0.6)
        assert words[15] == 0  # slot 2: greedy
        st.run(9)                    # column 9: clip 0 has its 5 tokens (columns 3 .. 7) and has taken eot twice
        assert _cut(st.st.tokens[2, 3:8].cpu().tolist()) == rows[0][0]
        assert abs(st.no_speech[2].item() - want_ns[0]) < 1e-3
        st.no_speech[2:3].fill_(float("nan"))  # in stream order: the retry must write it again
        # clip 0 AGAIN into slot 2, at column 9, at 0.8 / attempt 2; clip 5 at 0.4 / attempt 2 into the idle slot
        st.admit([(2, 0, LENS[0], draw(*RETRY)), (1, 5, LENS[5], draw(5))])
        words = st.rows.cpu().numpy().view(np.uint32)
        assert words[12:15].tolist() == [0, 0, RETRY[2]] and words[15:16].view(np.float32)[0] == np.float32(1.0) / np.float32(RETRY[1])
        st.run(4)                    # column 13
        assert st.starts.cpu().tolist() == [0, 9, 9, LENS[2], LENS[5], LENS[0]]
        st.run(2)                    # column 15: clip 2 has its 12 tokens (columns 3 .. 14)
        assert _cut(st.st.tokens[0, 3:15].cpu().tolist()) == rows[2][0]
        assert abs(st.st.sum_logprobs[0].item() - rows[2][1]) < 1e-2
        st.shift(9)                  # the live rows start at 9
        assert st.pos == 6 and st.st.pos.cpu().item() == 6
        assert st.starts.cpu().tolist() == [0, 0, 0, 0, LENS[5], LENS[0]]
        st.run(24)                   # clips 5 (22 tokens) and 0 (5 tokens) from column 3 on
        assert _cut(st.st.tokens[1, 3:3 + LENS[5]].cpu().tolist()) == rows[5][0]
        assert _cut(st.st.tokens[2, 3:3 + LENS[0]].cpu().tolist()) == retry[0]
        assert retry[0] != rows[0][0]  # the second occupancy drew something else than the greedy first
        assert abs(st.st.sum_logprobs[1].item() - rows[5][1]) < 1e-2 and abs(st.st.sum_logprobs[2].item() - retry[1]) < 1e-2
        ns = st.no_speech.cpu().numpy()
        assert abs(ns[2] - want_ns[0]) < 1e-3 and abs(ns[1] - want_ns[5]) < 1e-3 and abs(ns[0] - want_ns[2]) < 1e-3


def test_bf16_d384_mixed_rows_follow_rules_and_draws_on_their_own_logits():
    """W384, bf16 (the absorbed form), scripted table, weight seed 1, 6 clips through 2 slots at temperatures 0, .4, 1, .2, 0, .8 and
    attempts 0, 2, 5, 1, 0, 4, seed 3.  Every clip's own history is replayed through forced_decode_logits; on those logits the device's
    token equals the restatement's -- TR.apply_rules for a greedy row wherever the top-2 margin and the mass gap both exceed 1e-3,
    SR.sample_row with that step's noise for a sampled row wherever the key margin exceeds 1e-3 / T -- and at most 10 % of the steps are
    left out: the cap and the form of test_bf16_d384_follows_the_rules_on_its_own_logits.  (The f32 restatement of this configuration
    leaves out 0 of 40 sampled steps; its smallest key margin is 0.20.)"""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import forced_decode_logits

    W = _weights(W384, 1, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, W384, PR.clip_mels())
    feats = mixed_features(xa, len(LENS_BF16))
    always, first = R.suppress_lists(SP)
    m_always, m_first = TR.vocab_mask(V, always), TR.vocab_mask(V, list(always) + list(first))
    rules = dict(tb=TB, nt=NT, eot=EOT, max_init=50)
    m = _model(W384, W, torch.bfloat16)
    assert m.use_absorbed()
    dev = feats.cuda().to(torch.bfloat16)
    stats = []
    res = decode_continuous(m, dev, _options(seed=SEED), slots=2, sample_lens=LENS_BF16, check_every=4, stats_out=stats,
                            temperatures=TEMPERATURES_BF16, attempts=ATTEMPTS_BF16)
    assert len(stats[0].admissions) == 6 and stats[0].admissions[2][2] > 0
    n_init = len(INIT)
    checked = left_out = total = 0
    for i, n in enumerate(LENS_BF16):
        T, attempt = TEMPERATURES_BF16[i], ATTEMPTS_BF16[i]
        ids = res[i].tokens
        row = ids + [EOT] * (n - len(ids))  # the device's row up to the clip's limit
        hist = np.array([INIT + row], dtype=np.int64)
        trace, _ = forced_decode_logits(m, dev[i: i + 1], hist, n_init, always, first, EOT, rules=_rules())
        trace = trace.cpu().numpy()
        for k in range(n):
            seq = row[:k]
            if k > 0 and seq[-1] == EOT:
                continue
            total += 1
            mask = m_first if k == 0 else m_always
            if T == 0:
                st = TR.apply_rules(trace[0, k], seq, TB, NT, EOT, k == 0, 50, mask)
                sure, want = st.margin > 1e-3 and st.mass_gap > 1e-3, st.next
            else:
                noise = SR.gumbel_noise(SEED, [(i, 0)], attempt, n_init - 1 + k, V)[0]  # the row's OWN position in the counter
                st = SR.sample_row(trace[0, k], T, noise, mask, rules, seq, k == 0)
                sure, want = st.key_margin > 1e-3 / T, st.next
            if sure:
                assert row[k] == want, (i, k, T, row[k], want)
                checked += 1
            else:
                left_out += 1
    print(f"bf16 d=384, mixed rows: {checked} steps checked, {left_out} of {total} left out")
    assert left_out <= 0.1 * total


# ---------------------------------------------------------------- transcribe(seed=S) on both schedules
def _files():
    long = np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0)[: 10 * 16000]])          # 40 s
    short = R.synthetic_clip(1, 5.0)[: 5 * 16000]                                                        # 5 s
    longer = np.concatenate([R.synthetic_clip(3, 30.0), R.synthetic_clip(4, 30.0), R.synthetic_clip(5, 30.0)[: 5 * 16000]])  # 65 s
    mid = R.synthetic_clip(6, 30.0)[: 12 * 16000]                                                        # 12 s
    return [long, short, longer, mid]


TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def test_transcribe_with_a_seed_continuous_equals_rounds():
    """a 40 s, a 5 s, a 65 s and a 12 s file, "scripted" weights, sample_len = 20, f32, slots = 2, check_every = 8, seed 3.
    logprob_threshold is the midpoint of the two middle window avg_logprob values of a first rounds run without a threshold, so about
    half the windows retry.  Both schedules then give the same segments with the same temperatures, no needs_fallback anywhere, and the
    continuous run's retries are the retried windows' attempts 1, 2, ... in order."""
    import whisper_ipa_amd as wipa

    m = _model(MICRO, _weights(MICRO, 7, True), torch.float32)
    files = _files()
    kw = dict(language="en", sample_len=20, fp16=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        probe = wipa.transcribe(m, files, logprob_threshold=None, **kw)
        per_window = sorted({(i, s["seek"]): s["avg_logprob"] for i, r in enumerate(probe) for s in r["segments"]}.values())
        assert len(per_window) >= 4
        mid = len(per_window) // 2
        threshold = 0.5 * (per_window[mid - 1] + per_window[mid])
        print(f"{len(per_window)} windows, avg_logprob {per_window[0]:.4f} .. {per_window[-1]:.4f}; logprob_threshold {threshold:.4f}")
        stats = []
        rounds = wipa.transcribe(m, files, logprob_threshold=threshold, seed=SEED, **kw)
        cont = wipa.transcribe(m, files, logprob_threshold=threshold, seed=SEED, schedule="continuous", slots=2, check_every=8,
                               stats_out=stats, **kw)
    kept = {(i, s["seek"]): s["temperature"] for i, r in enumerate(rounds) for s in r["segments"]}
    assert any(t == 0.0 for t in kept.values()) and any(t > 0.0 for t in kept.values()), kept
    assert len(rounds) == len(cont) == 4
    for i, (x, y) in enumerate(zip(cont, rounds)):
        assert x["text"] == y["text"] and x["language"] == y["language"], (i, x["text"], y["text"])
        assert len(x["segments"]) == len(y["segments"]), (i, len(x["segments"]), len(y["segments"]))
        for s, t in zip(x["segments"], y["segments"]):
            for k in ("seek", "start", "end", "tokens", "text", "temperature", "id"):
                assert s[k] == t[k], (i, k, s[k], t[k])
            print(f"file {i} seek {s['seek']}: temperature {s['temperature']}, avg_logprob {s['avg_logprob']:.6f} vs {t['avg_logprob']:.6f}")
            assert abs(s["avg_logprob"] - t["avg_logprob"]) * 21 < 1e-2  # sample_len = 20: len + 1 <= 21, the existing test's bound
            assert abs(s["no_speech_prob"] - t["no_speech_prob"]) < 1e-3
            assert "needs_fallback" not in s and "needs_fallback" not in t
    st = stats[0]
    want = [(i, seek, k) for (i, seek), t in sorted(kept.items()) for k in range(1, TEMPS.index(t) + 1)]
    assert sorted(st.retries) == want, (st.retries, want)
    for window in {(i, seek) for i, seek, _ in st.retries}:  # a window's attempts come in order
        ks = [k for i, seek, k in st.retries if (i, seek) == window]
        assert ks == list(range(1, len(ks) + 1))
    decoded = [clip for g in st.groups for clip in g]
    assert len(decoded) == len(set(decoded)) and set(kept) <= set(decoded)  # every window once: fresh windows only
    assert st.rows == 2 and st.waited == [2, 3]


def test_evaluate_model_runs_the_base_leg_on_the_continuous_schedule_with_a_seed(tmp_path, capsys):
    """scripts/evaluate_model.py --decode continuous --base-decode transcribe --seed S runs through (it ended in the refusal of ``seed``):
    a one-layer local model and four 2 s clips, as tests/test_gpu_scoring.py builds them; the base leg scores all four files"""
    import evaluate_model as EM
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
        path = tmp_path / f"c{i}.wav"
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(pcm.tobytes())
        entries.append({"audio_path": str(path), "ipa_transcription": "kæt " + "ab" * (i + 1), "speaker_id": f"s{i}"})
    (tmp_path / "test.json").write_text(json.dumps(entries))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = EM.main(["--checkpoint", str(tmp_path / "no-checkpoint"), "--base-model", str(model_dir), "--test-data", str(tmp_path / "test.json"),
                       "--num-samples", "0", "--n-mels", "80", "--batch-size", "2", "--decode", "continuous", "--base-decode", "transcribe",
                       "--seed", str(SEED), "--allow-byte-fallback"])
    text = capsys.readouterr().out
    assert "Base Whisper Model - Overall Results" in text and "Evaluation Complete" in text
    assert out["base"]["num_samples"] == 4 and np.isfinite(out["base"]["per"])
