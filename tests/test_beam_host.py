"""CPU: the beam options' checks and refusals (decoding.beam_group, decode), and the numpy restatement of tests/beam_ref.py against
itself: a beam of one is the greedy oracle, the finished store never exceeds max_candidates, finalize fills up to beam_size, and every
(fixture clip, option set) of tests/test_gpu_beam.py clears the margin a device in f32 can be asked to resolve."""
import numpy as np
import pytest
import torch

import beam_cases as BC
import beam_ref as BM
import prompt_ref as PR
from oracle import whisper_ref as R
from whisper_ipa_amd.decoding import DecodingOptions, beam_group, decode


class _Model:  # what beam_group looks at: a loaded model has dims and packed()
    dims = PR.MICRO
    _fp8 = None

    def packed(self):
        raise AssertionError("not reached")


def test_beam_group_checks_the_options():
    m = _Model()
    assert beam_group(DecodingOptions(), m) is None
    assert beam_group(DecodingOptions(patience=2.0), m) is None  # patience without beam_size is ignored, as upstream ignores it
    assert beam_group(DecodingOptions(beam_size=5), m) == (5, 5)
    assert beam_group(DecodingOptions(beam_size=5, patience=2.0), m) == (5, 10)
    assert beam_group(DecodingOptions(beam_size=5, patience=0.5), m) == (5, round(2.5))
    assert beam_group(DecodingOptions(beam_size=1, patience=1.0), m) == (1, 1)  # a beam of one takes the beam path
    assert beam_group(DecodingOptions(beam_size=16, patience=4.0, length_penalty=1.0), m) == (16, 64)
    for kw in (dict(beam_size=0), dict(beam_size=17), dict(beam_size=2.5), dict(beam_size=True), dict(beam_size=5, patience=0.0),
               dict(beam_size=5, patience=-1.0), dict(beam_size=16, patience=4.1), dict(beam_size=2, patience=0.1),
               dict(beam_size=5, length_penalty=1.5), dict(beam_size=5, length_penalty=-0.1)):
        with pytest.raises(ValueError):
            beam_group(DecodingOptions(**kw), m)


def test_beam_group_refuses_by_name_what_beams_do_not_serve():
    m = _Model()
    fp8 = _Model()
    fp8._fp8 = object()
    for model, kw in ((None, {}), (object(), {}), (fp8, {}), (m, dict(temperature=0.2, seed=1)), (m, dict(prompt=[1, 2])), (m, dict(prefix="a")),
                      (m, dict(prompts=[[1]]))):
        with pytest.raises(NotImplementedError, match="beam_size"):
            beam_group(DecodingOptions(beam_size=5, **kw), model)
    feats = torch.zeros(1, PR.MICRO.n_audio_ctx, PR.MICRO.n_audio_state)
    with pytest.raises(NotImplementedError, match="beam_size"):
        decode(fp8, feats, DecodingOptions(beam_size=2))
    with pytest.raises(ValueError, match="beam_size and best_of"):
        decode(m, feats, DecodingOptions(beam_size=2, best_of=2, temperature=0.5, seed=1))


def test_a_beam_of_one_is_the_greedy_oracle():
    W, xa = BC.micro_fixture()
    sp = PR.SP
    initial, always, first, _ = BC.decode_inputs(False)
    with torch.no_grad():
        ref = R.greedy_decode(W, PR.MICRO, xa, initial, always, first, sp.eot, sample_len=BC.SAMPLE_LEN, stop_on_eot=False)
    for c, r in enumerate(BC.restated(1, 1.0, False, None)):
        body = ref.tokens[c, len(initial):].tolist()
        n = body.index(sp.eot) if sp.eot in body else len(body)
        assert r.tokens == body[:n]


def test_the_store_never_exceeds_max_candidates_and_finalize_fills_to_beam_size():
    rng = np.random.default_rng(0)
    G, maxc = 3, 4
    clip = BM.Clip(np.array([BC.INITIAL] * G, dtype=np.int64), np.zeros(G, dtype=np.float32))
    for i in range(6):  # EOT is every beam's best candidate from the second step on
        rows = [BC.crafted_rows(50 + i, G, 1, 0 if i else None)[j].astype(np.float64) for j in range(G)]
        BM.update(clip, rows, BC.EOT, maxc, i == 0)
        assert len(clip.finished) <= maxc
        assert clip.tokens.shape == (G, len(BC.INITIAL) + i + 1) and not (clip.tokens == BC.EOT).any()  # live beams never hold EOT
    assert len(clip.finished) == maxc and BM.complete(clip, maxc)
    scores = [float(s) for _, s in clip.finished[:2]]
    assert scores == sorted(scores, reverse=True)  # one step's finished sequences join in descending score
    empty = BM.Clip(np.array([BC.INITIAL + [11 + j] for j in range(G)], dtype=np.int64), np.array([-2.0, -1.0, -3.0], dtype=np.float32))
    BM.finalize(empty, BC.EOT)
    assert [seq[-2] for seq, _ in empty.finished] == [12, 11, 13] and all(seq[-1] == BC.EOT for seq, _ in empty.finished)
    one = BM.Clip(empty.tokens.copy(), empty.sums.copy(), finished=[([1, 2, 3, 9, BC.EOT], np.float32(-0.5))])
    BM.finalize(one, BC.EOT)
    assert len(one.finished) == G and one.finished[0][0][3] == 9
    assert BM.rank(one, 3, BC.EOT, None)[0] == 0 and BM.rank(one, 3, BC.EOT, 0.6)[0] == 0


@pytest.mark.parametrize("G,patience,timed", BC.MODEL_CASES)
def test_every_gpu_case_clears_the_required_margin(G, patience, timed):
    """2 x steps x 1e-3: two rows compared, each with at most ``steps`` accumulated adds of a log-probability off by the f32 logits tolerance"""
    for lp in BC.LENGTH_PENALTIES:
        res = BC.restated(G, patience, timed, lp)
        margin = BM.min_margin(res)
        print(f"G={G} patience={patience} timed={timed} length_penalty={lp}: margin {margin:.4f}, steps {[r.steps for r in res]}")
        assert max(r.steps for r in res) <= BC.SAMPLE_LEN
        assert margin > BC.required_margin(), (G, patience, timed, lp, margin)


# ---------------------------------------------------------------- transcribe(beam_size=)
class _Tok:
    timestamp_begin, eot, no_timestamps = 50364, 50257, 50363

    def decode(self, ids):
        return "".join(chr(97 + int(t) % 26) for t in ids)

    def encode(self, text):
        return [ord(c) for c in text]


def _fake_result(tokens, feats=None):
    from whisper_ipa_amd.decoding import DecodingResult

    return DecodingResult(audio_features=feats, language="en", tokens=list(tokens), text="ab", avg_logprob=-0.1, no_speech_prob=0.0, temperature=0.0,
                          compression_ratio=1.0)


def test_transcribe_hands_beams_to_a_decoder_that_has_them_and_refuses_the_rest_by_name():
    from whisper_ipa_amd import transcribe

    audio = np.zeros(16000, dtype=np.float32)
    calls = []

    def decode_fn(windows, languages):
        calls.append(len(windows))
        return [_fake_result([50364, 5, 6, 50364 + 40]) for _ in languages]

    with pytest.raises(NotImplementedError, match="beam_size"):  # no beams attribute: as before
        transcribe(None, audio, decode_fn=decode_fn, tokenizer=_Tok(), language="en", beam_size=2)
    decode_fn.beams = True
    out = transcribe(None, audio, decode_fn=decode_fn, tokenizer=_Tok(), language="en", beam_size=2, patience=2.0, length_penalty=0.6)
    assert calls and out["segments"]
    for kw in (dict(schedule="continuous"), dict(condition_on_previous_text=True), dict(initial_prompt="a"), dict(word_timestamps=True)):
        with pytest.raises(NotImplementedError, match="beam_size"):
            transcribe(None, audio, decode_fn=decode_fn, tokenizer=_Tok(), language="en", beam_size=2, align_fn=lambda *a, **k: None, **kw)


def test_the_models_retry_drops_the_beams_above_temperature_zero(monkeypatch):
    """upstream's decode_with_fallback: beam_size and patience belong to temperature 0, best_of to the temperatures above"""
    import whisper_ipa_amd.decoding as D
    from whisper_ipa_amd.transcribe import _model_decoder

    seen = []

    def fake_decode(model, feats, options):
        seen.append(options)
        return [_fake_result([1]) for _ in range(feats.shape[0])]

    monkeypatch.setattr(D, "decode", fake_decode)
    run = _model_decoder(object(), dict(beam_size=5, patience=2.0, length_penalty=0.6, sample_len=12))
    res = [_fake_result([1], torch.zeros(4, 8)) for _ in range(2)]
    run.retry(res, ["en", "en"], temperature=0.2, attempt=1, streams=[(0, 0), (0, 1)], seed=3, best_of=5)
    (opts,) = seen
    assert opts.beam_size is None and opts.patience is None and opts.best_of == 5 and opts.length_penalty == 0.6 and opts.temperature == 0.2
    assert opts.sample_len == 12


def test_the_transcribe_windows_clear_the_required_margin():
    out, margins = BC.restated_transcribe()
    print("window margins", margins)
    assert len(margins) >= 3 and min(margins) > BC.required_margin()
    assert len({s["seek"] for s in out[0]["segments"]}) >= 2
