"""CPU: the sampling restatement's generator against Random123's known answers, the reference's own distribution, the
``transcribe()`` temperature fallback on scripted decodes, and the option refusals.  Reference: mlx_whisper.transcribe's
decode_with_fallback over the default schedule (0.0, 0.2, ..., 1.0), as the reference's base-model evaluation leg runs it."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import sampling_ref as SR

T = 50364
a, b, c, d = 1000, 1001, 1002, 1003


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(counter, key, want):
    got = tuple(int(w) for w in SR.philox4x32_10(counter, key))
    assert got == want, [hex(w) for w in got]


def test_uniforms_are_exact_in_f32_and_the_noise_stays_in_range():
    words = np.array([0, 1 << 9, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)
    u = SR.uniform_from_words(words)
    assert (u.astype(np.float32).astype(np.float64) == u).all() and u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    g = -np.log(-np.log(u))
    assert -2.82 < g.min() and g.max() < 16.7
    # the noise of a row is a function of (seed, stream, attempt, p, c) alone: the same row inside another set of streams
    one = SR.gumbel_noise(9, [(5, 2)], 3, 17, 4099)
    many = SR.gumbel_noise(9, [(1, 0), (5, 2), (5, 3)], 3, 17, 4099)
    assert (one[0] == many[1]).all() and not (many[1] == many[2]).any()
    assert not (SR.gumbel_noise(9, [(5, 2)], 3, 18, 4099) == one).any()


def test_the_reference_draws_from_softmax_of_the_tempered_row():
    """the distribution test of tests/test_gpu_sampling.py on the reference alone: same row, streams, seed and bound"""
    l, mask, streams = SR.distribution_case()
    noise = SR.gumbel_noise(SR.DIST_SEED, streams, 0, 3, SR.DIST_V)
    toks = [SR.sample_row(l, SR.DIST_T, noise[i], mask).next for i in range(SR.DIST_ROWS)]
    stat, df, bound = SR.chi_square_vs_softmax(toks, l.astype(np.float64) + mask, SR.DIST_T)
    print(f"chi-square {stat:.1f} on {df} degrees of freedom (bound {bound:.1f})")
    assert not set(toks) & set(SR.DIST_DEAD)
    assert 20 <= df <= SR.DIST_V - 4 and stat < bound
    # the bound itself against tabulated quantiles: chi-square(10) 0.5 -> 9.342, 0.95 -> 18.307; chi-square(63) 0.95 -> 82.529; and the
    # Wilson-Hilferty approximation of the 1 - 1e-6 quantile (z = 4.7534) of chi-square(63), 131.7
    assert abs(SR.chi2_quantile(0.5, 10) - 9.342) < 1e-2 and abs(SR.chi2_quantile(0.95, 10) - 18.307) < 1e-2
    assert abs(SR.chi2_quantile(0.95, 63) - 82.529) < 1e-2 and abs(SR.chi2_quantile(1 - 1e-6, 63) - 131.7) < 1.0


# ---------------------------------------------------------------- the fallback loop
class _Tok:
    timestamp_begin, eot = T, 50257

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)


def _res(tokens, avg_logprob=-0.3, no_speech_prob=0.1, compression_ratio=1.2, temperature=0.0, tag=None):
    return SimpleNamespace(tokens=tokens, avg_logprob=avg_logprob, no_speech_prob=no_speech_prob, compression_ratio=compression_ratio,
                           temperature=temperature, language="en", tag=tag)


def _files():
    """four files, told apart by their first sample: 0 a 40 s file whose first window is too repetitive until 0.4, 1 never
    passes, 2 silent and unsure (upstream's silence exception: no retry, then skipped), 3 passes at once"""
    clips = [np.zeros(40 * 16000, dtype=np.float32)] + [np.zeros(10 * 16000, dtype=np.float32) for _ in range(3)]
    for i, x in enumerate(clips):
        x[0] = i + 1.0
    return clips


def _scripted(calls):
    def decode_fn(windows, languages):
        out = []
        for w in windows:
            kind = int(w[0])  # 0: the long file's second window
            out.append({0: _res([T + 0, d, T + 500], tag="w2"),
                        1: _res([T + 0, b, c, T + 500], compression_ratio=3.0, tag="rep"),
                        2: _res([T + 0, b], avg_logprob=-2.0, tag="low"),
                        3: _res([T + 0, d], avg_logprob=-1.5, no_speech_prob=0.9, tag="silent"),
                        4: _res([T + 0, a, T + 100], tag="fine")}[kind])
        calls.append(("decode", len(windows)))
        return out

    def fallback_fn(results, languages, *, temperature, attempt, streams, seed):
        assert len(results) == len(languages) == len(streams) and all(l == "en" for l in languages)
        calls.append(("retry", temperature, attempt, list(streams), seed, [r.tag for r in results]))
        out = []
        for r in results:
            if r.tag == "rep" and attempt >= 2:
                out.append(_res([T + 0, a, b], temperature=temperature, tag="rep-ok"))  # spans the window: seek moves 3000 frames
            elif r.tag == "rep":
                out.append(_res([T + 0, b, c, T + 500], compression_ratio=2.9, temperature=temperature, tag="rep"))
            else:
                out.append(_res([T + 0, c], avg_logprob=-1.2 - 0.1 * attempt, temperature=temperature, tag="low"))
        return out

    return decode_fn, fallback_fn


def test_fallback_retries_failing_rows_as_one_sub_batch_per_temperature():
    from whisper_ipa_amd.transcribe import transcribe

    calls = []
    decode_fn, fallback_fn = _scripted(calls)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = transcribe(None, _files(), language="en", decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), seed=11)
    assert not [x for x in w if "needs_fallback" in str(x.message)]
    # round 1: four windows; files 0 and 1 fail and go out together at 0.2 and 0.4; file 0 passes there, file 1 goes on alone to 1.0
    assert calls[0] == ("decode", 4)
    retries = [c0 for c0 in calls if c0[0] == "retry"]
    assert [(r[1], r[2]) for r in retries] == [(0.2, 1), (0.4, 2), (0.6, 3), (0.8, 4), (1.0, 5)]
    assert [r[3] for r in retries] == [[(0, 0), (0, 1)], [(0, 0), (0, 1)], [(0, 1)], [(0, 1)], [(0, 1)]]  # (seek, file index)
    assert [r[5] for r in retries] == [["rep", "low"], ["rep", "low"], ["low"], ["low"], ["low"]]  # the silent window is never retried
    assert all(r[4] == 11 for r in retries)
    # round 2: the long file's second window passes at 0.0: no retry
    assert calls[6:] == [("decode", 1)]
    segs = [o["segments"] for o in out]
    assert [(s["seek"], s["temperature"], s["text"]) for s in segs[0]] == [(0, 0.4, "ab"), (3000, 0.0, "d")]
    assert [(s["seek"], s["temperature"], s["text"]) for s in segs[1]] == [(0, 1.0, "c")]  # the last attempt is kept
    assert abs(segs[1][0]["avg_logprob"] + 1.7) < 1e-12
    assert segs[2] == [] and [(s["temperature"], s["text"]) for s in segs[3]] == [(0.0, "a")]
    assert not any("needs_fallback" in s for f in segs for s in f)


def test_a_files_streams_do_not_depend_on_the_files_it_is_transcribed_with():
    from whisper_ipa_amd.transcribe import transcribe

    def per_file(calls, index):
        return [(r[1], r[2], s) for r in calls if r[0] == "retry" for s in r[3] if s[1] == index]

    alone, listed = [], []
    transcribe(None, _files()[0], language="en", decode_fn=_scripted(alone)[0], fallback_fn=_scripted(alone)[1], tokenizer=_Tok(), seed=11)
    transcribe(None, _files(), language="en", decode_fn=_scripted(listed)[0], fallback_fn=_scripted(listed)[1], tokenizer=_Tok(), seed=11)
    assert per_file(alone, 0) == per_file(listed, 0) == [(0.2, 1, (0, 0)), (0.4, 2, (0, 0))]


def test_without_a_seed_or_without_a_fallback_fn_nothing_changes():
    from whisper_ipa_amd.transcribe import transcribe

    for kw in (dict(seed=None, with_fallback=True), dict(seed=11, with_fallback=False)):
        calls = []
        decode_fn, fallback_fn = _scripted(calls)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = transcribe(None, _files(), language="en", decode_fn=decode_fn, tokenizer=_Tok(), seed=kw["seed"],
                             fallback_fn=fallback_fn if kw["with_fallback"] else None)
        assert [c0[0] for c0 in calls] == ["decode", "decode"]
        assert len([x for x in w if "needs_fallback" in str(x.message)]) == 1
        assert [s.get("needs_fallback", False) for s in out[0]["segments"]] == [True, False]
        assert [s.get("needs_fallback", False) for s in out[1]["segments"]] == [True]
        assert all(s["temperature"] == 0.0 for o in out for s in o["segments"])


def test_a_schedule_must_still_start_at_zero():
    from whisper_ipa_amd.transcribe import transcribe

    with pytest.raises(NotImplementedError, match="temperature"):
        transcribe(None, np.zeros(16000, dtype=np.float32), decode_fn=lambda w, l: [], tokenizer=_Tok(), seed=3, temperature=0.2)


# ---------------------------------------------------------------- the options
def test_sampling_is_served_with_a_seed_only():
    from dataclasses import fields

    from whisper_ipa_amd.decoding import DecodingOptions, _refuse_unsupported

    assert [f.name for f in fields(DecodingOptions)][-3:] == ["seed", "sample_streams", "sample_attempt"]
    o = DecodingOptions()
    assert o.seed is None and o.sample_streams is None and o.sample_attempt == 0
    _refuse_unsupported(DecodingOptions(temperature=0.4, seed=1))
    _refuse_unsupported(DecodingOptions(temperature=0.4, seed=1, without_timestamps=False))
    with pytest.raises(NotImplementedError, match="seed"):
        _refuse_unsupported(DecodingOptions(temperature=0.4))
    for kw in (dict(best_of=5), dict(beam_size=5)):
        with pytest.raises(NotImplementedError):
            _refuse_unsupported(DecodingOptions(temperature=0.4, seed=1, **kw))


def test_the_record_helper_refuses_a_temperature_that_is_not_above_zero():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    L = _lib.lib()
    n = L.wipa_sample_record_bytes(3)
    assert n == 16 + 3 * 8
    buf = np.zeros(n, dtype=np.uint8)
    for t in (0.0, -0.5, float("nan"), float("inf")):
        assert L.wipa_sample_record_fill(buf.ctypes.data, n, 1, 0, t, None, 3) != 0 and b"temperature" in L.wipa_last_error()
    assert L.wipa_sample_record_fill(buf.ctypes.data, n - 1, 1, 0, 0.5, None, 3) != 0
    assert L.wipa_sample_record_fill(buf.ctypes.data, n, 1, 65536, 0.5, None, 3) != 0
    streams = (C.c_uint32 * 6)(7, 1, 8, 2, 9, 3)
    assert L.wipa_sample_record_fill(buf.ctypes.data, n, (5 << 32) | 6, 4, 0.5, streams, 3) == 0
    words = buf.view(np.uint32)
    assert words[:3].tolist() == [6, 5, 4] and buf.view(np.float32)[3] == 2.0 and words[4:].tolist() == [7, 1, 8, 2, 9, 3]
    assert L.wipa_sample_record_fill(buf.ctypes.data, n, 1, 0, 0.5, None, 3) == 0 and words[4:].tolist() == [0, 0, 1, 0, 2, 0]
    # a NULL record where one is required: refused before any launch
    fake = C.c_void_p(0x1000)
    assert L.wipa_sample_step(fake, 4100, 2, 4099, fake, fake, fake, 16, fake, 3, 3990, None, None, fake, fake, None) != 0
    assert b"sampling record" in L.wipa_last_error()
    assert L.wipa_sample_noise(None, 0, 0, 16, fake, None) != 0
