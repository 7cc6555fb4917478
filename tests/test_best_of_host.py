"""CPU: best-of-N sampling's host side -- option validation (upstream's _verify_options), the candidate-stream rule, the penalty
table, the restated ranker of tests/best_of_ref.py on hand-worked groups, and transcribe()'s handling of best_of around the
temperature schedule (stub decoders).  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import best_of_ref as BR

T, EOT = 50364, 50257


# ---------------------------------------------------------------- the options
def test_best_of_options_are_checked_as_upstream_checks_them():
    import torch

    from whisper_ipa_amd.decoding import DecodingOptions, best_of_group, decode

    assert best_of_group(DecodingOptions()) == 1
    assert best_of_group(DecodingOptions(temperature=0.4, seed=1)) == 1
    assert best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=5)) == 5
    assert best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=1)) == 1
    assert best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=3, length_penalty=0.6)) == 3
    with pytest.raises(ValueError, match=r"best_of with greedy sampling \(T=0\) is not compatible"):
        best_of_group(DecodingOptions(best_of=5))
    with pytest.raises(ValueError, match="best_of with greedy sampling"):
        best_of_group(DecodingOptions(best_of=5, seed=1))
    with pytest.raises(NotImplementedError, match="seed"):
        best_of_group(DecodingOptions(temperature=0.4, best_of=5))
    with pytest.raises(ValueError, match="beam_size and best_of"):
        best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=5, beam_size=5))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="length_penalty"):
            best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=2, length_penalty=bad))
    for ok in (0.0, 1.0, None):
        best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=2, length_penalty=ok))
    # without best_of nothing new is checked: a decode that ignored length_penalty / patience goes on ignoring them
    assert best_of_group(DecodingOptions(length_penalty=1.5, patience=2.0)) == 1
    assert best_of_group(DecodingOptions(temperature=0.4, seed=1, length_penalty=-1.0, patience=2.0)) == 1
    with pytest.raises(NotImplementedError, match="patience"):
        best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=2, patience=1.0))
    with pytest.raises(ValueError, match="best_of"):
        best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=0))
    # the candidate index lives above bit 24 of the stream's high word
    best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=2, sample_streams=[(7, (1 << 24) - 1)]))
    best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=1, sample_streams=[(7, 1 << 24)]))  # one candidate: any stream
    with pytest.raises(ValueError, match=r"2\*\*24"):
        best_of_group(DecodingOptions(temperature=0.4, seed=1, best_of=2, sample_streams=[(7, 1 << 24)]))
    # decode() checks them before it touches the model or the features
    feats = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="best_of with greedy sampling"):
        decode(None, feats, DecodingOptions(best_of=5))
    with pytest.raises(ValueError, match=r"2\*\*24"):
        decode(None, feats, DecodingOptions(temperature=0.4, seed=1, best_of=2, sample_streams=[(0, 0), (7, 1 << 24)]))
    with pytest.raises(NotImplementedError, match="beam_size"):
        decode(None, feats, DecodingOptions(beam_size=5))
    with pytest.raises(NotImplementedError, match="patience"):
        decode(None, feats, DecodingOptions(temperature=0.4, seed=1, best_of=2, patience=1.0))


# ---------------------------------------------------------------- the streams
def test_candidate_k_draws_from_the_rows_stream_plus_k_in_the_high_bits():
    from whisper_ipa_amd.decoding import candidate_streams

    assert BR.candidate_stream((40, 1), 0) == (40, 1)
    assert BR.candidate_stream((40, 1), 2) == (40, 1 + (2 << 24))
    streams = [(40, 1), (3000, 0)]
    want = [(40, 1), (40, 1 + (1 << 24)), (40, 1 + (2 << 24)), (3000, 0), (3000, 1 << 24), (3000, 2 << 24)]
    assert BR.candidate_streams(streams, 3) == want
    assert candidate_streams(streams, 3) == want
    assert candidate_streams(streams, 1) == streams  # candidate 0 is the row's own draw
    assert len(set(candidate_streams([(s, f) for s in (0, 3000) for f in range(4)], 5))) == 40  # windows and candidates never collide
    with pytest.raises(ValueError):
        candidate_streams([(1, 1 << 24)], 2)


# ---------------------------------------------------------------- the penalty
def test_the_penalty_table_is_upstreams_arithmetic():
    from whisper_ipa_amd.decoding import length_penalty_table

    t = length_penalty_table(4, None)
    assert t.dtype == np.float64 and t.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    t = length_penalty_table(7, 1.0)
    assert t.tolist() == [5 / 6, 1.0, 7 / 6, 8 / 6, 9 / 6, 10 / 6, 11 / 6, 2.0]
    t = length_penalty_table(3, 0.5)
    assert t.tolist() == [(5 / 6) ** 0.5, 1.0, (7 / 6) ** 0.5, (8 / 6) ** 0.5]
    assert length_penalty_table(2, 0.0).tolist() == [1.0, 1.0, 1.0]
    for lp in (None, 0.3, 1.0):
        assert length_penalty_table(9, lp).tolist() == [BR.penalty(n, lp) for n in range(10)]


# ---------------------------------------------------------------- the ranker, by hand
def _rows(bodies, n, pad=7):
    """token rows [B, 3 + n]: three prompt columns, then the body, then filler"""
    out = np.full((len(bodies), 3 + n), pad, dtype=np.int64)
    out[:, :3] = [1, 2, 3]
    for b, body in enumerate(bodies):
        out[b, 3:3 + len(body)] = body
    return out


def test_the_restated_ranker_on_hand_worked_groups():
    n = 6
    # lengths 3 and 1: -6 / 3 = -2 beats -4 / 1; with length_penalty = 1.0 the penalties are 8/6 and 1: -4.5 loses to -4
    toks = _rows([[10, 11, 12, EOT], [10, EOT]], n)
    sums = np.array([-6.0, -4.0], dtype=np.float32)
    w, ls, sc = BR.rank(toks, sums, 2, 3, n, EOT)
    assert w.tolist() == [0] and ls.tolist() == [[3, 1]] and sc == [[-2.0, -4.0]]
    w, ls, sc = BR.rank(toks, sums, 2, 3, n, EOT, length_penalty=1.0)
    assert w.tolist() == [1] and sc == [[-6.0 / (8 / 6), -4.0]]
    # a tie: the first maximum, like np.argmax
    toks = _rows([[10, 11, EOT], [20, 21, EOT], [30, EOT]], n)
    w, ls, sc = BR.rank(toks, np.array([-3.0, -3.0, -9.0], dtype=np.float32), 3, 3, n, EOT)
    assert w.tolist() == [0] and sc[0][0] == sc[0][1] == -1.5 and int(np.argmax(sc[0])) == 0
    # a row without EOT has all n tokens; an EOT in the first column has none and never wins
    toks = _rows([[EOT], [10, 11, 12, 13, 14, 15], [10, 11, 12, 13, 14, EOT]], n)
    w, ls, sc = BR.rank(toks, np.array([-0.1, -12.0, -11.0], dtype=np.float32), 3, 3, n, EOT)
    assert ls.tolist() == [[0, 6, 5]] and sc[0][0] == float("-inf") and w.tolist() == [1]  # -2.0 against -2.2
    # tokens after the first EOT are not counted, whatever they are
    toks = _rows([[10, EOT, 11, EOT], [10, 11, EOT]], n)
    w, ls, sc = BR.rank(toks, np.array([-1.0, -1.5], dtype=np.float32), 2, 3, n, EOT)
    assert ls.tolist() == [[1, 2]] and w.tolist() == [1]
    # every candidate empty: candidate 0
    w, ls, sc = BR.rank(_rows([[EOT], [EOT]], n), np.array([-1.0, -0.5], dtype=np.float32), 2, 3, n, EOT)
    assert w.tolist() == [0]
    # two clips are ranked apart; the f32 sum is widened, not re-rounded
    toks = _rows([[10, EOT], [10, 11, EOT], [10, 11, 12, EOT], [10, EOT]], n)
    sums = np.array([-0.7, -1.1, -2.0, -0.9], dtype=np.float32)
    w, ls, sc = BR.rank(toks, sums, 2, 3, n, EOT)
    assert w.tolist() == [1, 0] and sc[0][1] == float(np.float32(-1.1)) / 2.0 and sc[1][0] == float(np.float32(-2.0)) / 3.0


# ---------------------------------------------------------------- transcribe()
class _Tok:
    timestamp_begin, eot = T, EOT

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)


def _res(tokens, avg_logprob, temperature=0.0):
    return SimpleNamespace(tokens=tokens, avg_logprob=avg_logprob, no_speech_prob=0.1, compression_ratio=1.2, temperature=temperature,
                           language="en")


def _stubs(calls):
    def decode_fn(windows, languages, **kw):
        calls.append(("decode", dict(kw)))
        return [_res([T + 0, 1000, T + 100], avg_logprob=-1.5) for _ in languages]  # fails the log-probability threshold

    def fallback_fn(results, languages, *, temperature, attempt, streams, seed, **kw):
        calls.append(("retry", temperature, attempt, list(streams), dict(kw)))
        ok = attempt >= 2
        return [_res([T + 0, 1001, T + 100], avg_logprob=-0.2 if ok else -1.4, temperature=temperature) for _ in results]

    return decode_fn, fallback_fn


def test_transcribe_drops_best_of_at_temperature_zero_and_passes_it_to_every_retry():
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(16000 * 3, dtype=np.float32)
    calls = []
    decode_fn, fallback_fn = _stubs(calls)
    out = transcribe(None, audio, language="en", decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), seed=11, best_of=5)
    assert calls[0] == ("decode", {})  # as upstream's decode_with_fallback: no best_of at temperature 0
    retries = [c for c in calls if c[0] == "retry"]
    assert [(r[1], r[2]) for r in retries] == [(0.2, 1), (0.4, 2)]
    assert all(r[4] == {"best_of": 5} for r in retries)
    assert all(r[3] == [(0, 0)] for r in retries)  # the streams stay (seek, file index): candidates are derived from them
    assert [s["temperature"] for s in out["segments"]] == [0.4]
    # without best_of the retries are called as ever
    calls = []
    decode_fn, fallback_fn = _stubs(calls)
    transcribe(None, audio, language="en", decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), seed=11)
    assert all(c[-1] == {} for c in calls)
    # without a seed only temperature 0 runs: best_of is dropped with it
    calls = []
    decode_fn, fallback_fn = _stubs(calls)
    with pytest.warns(RuntimeWarning):
        transcribe(None, audio, language="en", decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), best_of=5)
    assert calls == [("decode", {})]
    # beams stay refused, and so does best_of where nothing could draw the candidates
    with pytest.raises(NotImplementedError, match="beam_size"):
        transcribe(None, audio, decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), seed=11, beam_size=5)
    with pytest.raises(NotImplementedError, match="best_of"):
        transcribe(None, audio, decode_fn=decode_fn, tokenizer=_Tok(), seed=11, best_of=5)


def test_the_models_retry_forwards_best_of_to_decode(monkeypatch):
    """the built-in decode_fn / fallback_fn: DecodingOptions of the first decode carry no best_of, those of a retry do"""
    import torch

    import whisper_ipa_amd.audio as A
    import whisper_ipa_amd.decoding as D
    from whisper_ipa_amd.transcribe import _model_decoder

    seen = []

    def fake_decode(model, mel, options):
        seen.append(options)
        return [SimpleNamespace(audio_features=torch.zeros(2, 2)) for _ in range(mel.shape[0])]

    monkeypatch.setattr(D, "decode", fake_decode)
    monkeypatch.setattr(A, "log_mel_spectrogram", lambda audio, n_mels: torch.zeros(audio.shape[0], 4, n_mels))
    model = SimpleNamespace(device="cpu", dims=SimpleNamespace(n_mels=80))
    run = _model_decoder(model, {"length_penalty": 0.5})
    res = run(np.zeros((2, 16), dtype=np.float32), ["en", "en"])
    assert seen[0].best_of is None and seen[0].temperature == 0.0 and seen[0].length_penalty == 0.5
    run.retry(res, ["en", "en"], temperature=0.4, attempt=2, streams=[(0, 0), (3000, 1)], seed=9, best_of=3)
    o = seen[1]
    assert (o.best_of, o.temperature, o.seed, o.sample_attempt, o.length_penalty) == (3, 0.4, 9, 2, 0.5)
    assert [tuple(s) for s in o.sample_streams] == [(0, 0), (3000, 1)]
    run.retry(res, ["en", "en"], temperature=0.4, attempt=2, streams=[(0, 0), (3000, 1)], seed=9)
    assert seen[2].best_of is None
