"""CPU: prompt conditioning on the host -- upstream's ``_get_initial_tokens`` (prompt / prefix assembly), the packer that right-aligns
per-row initial tokens to one prompt width, ``transcribe()``'s prompt bookkeeping on scripted decodes, and the argument refusals of the
ragged entry points (no launch).  Reference: mlx_whisper.transcribe with condition_on_previous_text / initial_prompt
(scripts/evaluate_model.py:112-119 of the reference calls it with upstream's defaults); openai-whisper's decoding.py / transcribe.py
state the algorithm."""
import ctypes as C
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

T = 50364
EOT = 50257


@pytest.fixture(scope="module")
def tok():
    from whisper_ipa_amd.tokenizer import get_tokenizer

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return get_tokenizer(True, language="en", task="transcribe")


# ---------------------------------------------------------------- prompt assembly
def test_initial_tokens_follow_upstream(tok):
    from whisper_ipa_amd.decoding import initial_tokens

    sot = list(tok.sot_sequence)
    n_ctx = 448
    assert initial_tokens(tok, sot, None, None, n_ctx, 224) == sot
    assert initial_tokens(tok, sot, [], None, n_ctx, 224) == sot  # an empty prompt is no prompt: no <|startofprev|>
    ids = tok.encode(" hello world")
    # a string becomes encode(" " + s.strip()); a list of ids is taken as it is
    assert initial_tokens(tok, sot, "  hello world ", None, n_ctx, 224) == [tok.sot_prev] + ids + sot
    assert initial_tokens(tok, sot, ids, None, n_ctx, 224) == [tok.sot_prev] + ids + sot
    # truncation to the LAST n_ctx // 2 - 1 = 223 tokens; <|startofprev|> comes first
    long = list(range(1000, 1300))
    got = initial_tokens(tok, sot, long, None, n_ctx, 224)
    assert got[0] == tok.sot_prev and got[1:224] == long[-223:] and got[224:] == sot and len(got) == 227
    # the prefix follows the sot_sequence; prefix_tokens[-(n_ctx // 2 - sample_len):] with a bound of 0 keeps everything
    pre = list(range(2000, 2010))
    assert initial_tokens(tok, sot, None, pre, n_ctx, 224) == sot + pre
    assert initial_tokens(tok, sot, None, pre, n_ctx, 220) == sot + pre[-4:]
    assert initial_tokens(tok, sot, None, " hello world", n_ctx, 224) == sot + ids
    assert initial_tokens(tok, sot, long, pre, n_ctx, 221) == [tok.sot_prev] + long[-223:] + sot + pre[-3:]


def test_prompt_and_prompts_together_are_refused():
    from whisper_ipa_amd.decoding import DecodingOptions, resolve_prompts

    with pytest.raises(ValueError, match="prompts"):
        resolve_prompts(DecodingOptions(prompt=[1, 2], prompts=[[1], [2]]), 2)
    with pytest.raises(ValueError, match="2 rows"):
        resolve_prompts(DecodingOptions(prompts=[[1]]), 2)
    assert resolve_prompts(DecodingOptions(prompt=[1, 2]), 2) == [[1, 2], [1, 2]]
    assert resolve_prompts(DecodingOptions(prompts=[None, [3]]), 2) == [None, [3]]
    assert resolve_prompts(DecodingOptions(prompts=[None, []]), 2) is None and resolve_prompts(DecodingOptions(), 3) is None


def test_prompts_are_served_by_decode_only():
    """transcribe_batches (and every other caller of _refuse_unsupported) keeps refusing prompts"""
    from whisper_ipa_amd.decoding import DecodingOptions, _refuse_unsupported

    with pytest.raises(NotImplementedError, match="prompts"):
        _refuse_unsupported(DecodingOptions(prompts=[[1]], without_timestamps=False))
    with pytest.raises(NotImplementedError, match="prompt"):
        _refuse_unsupported(DecodingOptions(prefix=[1], without_timestamps=False))


# ---------------------------------------------------------------- the packer
def test_packer_right_aligns_and_rounds_the_width():
    from whisper_ipa_amd.decoding import pack_prompts

    rows = [[7, 8, 9], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17], [5]]
    tokens, starts, P = pack_prompts(rows, 448, 224)
    assert P == 32 and tokens.shape == (3, 32) and tokens.dtype == np.int32 and starts.dtype == np.int32
    assert starts.tolist() == [29, 15, 31]
    for b, r in enumerate(rows):
        assert tokens[b, starts[b]:].tolist() == r and (tokens[b, : starts[b]] == 0).all()
    assert pack_prompts([[1] * 16], 448, 224)[2] == 16 and pack_prompts([[1] * 17], 448, 224)[2] == 32
    # longest = 227 with sample_len = 224: rounding to 240 would leave 208 < min(224, 221) columns: P stays exact
    t, s, P = pack_prompts([[1] * 227, [2] * 3], 448, 224)
    assert P == 227 and s.tolist() == [0, 224]
    # ... with 20 tokens to generate the rounded width leaves room
    assert pack_prompts([[1] * 227, [2] * 3], 448, 20)[2] == 240
    assert pack_prompts([[1] * 220], 448, 224)[2] == 224 and pack_prompts([[1] * 225], 448, 224)[2] == 225
    # pad_to: a row alone at the width of a batch
    t, s, P = pack_prompts([[4, 5]], 448, 224, pad_to=240)
    assert P == 240 and s.tolist() == [238] and t[0, 238:].tolist() == [4, 5]
    with pytest.raises(ValueError):
        pack_prompts([[1] * 30], 448, 224, pad_to=16)
    with pytest.raises(ValueError):
        pack_prompts([[1], []], 448, 224)
    with pytest.raises(ValueError):
        pack_prompts([[1] * 449], 448, 224)
    assert pack_prompts(None, 448, 224) is None  # no row has a prompt: no ragged path


# ---------------------------------------------------------------- transcribe(): upstream's prompt bookkeeping on scripted decodes
a, b, c, d, e, f = 1000, 1001, 1002, 1003, 1004, 1005


class _Tok:
    """what transcribe() needs of a tokenizer: ids 1000.. render as letters, and back"""
    timestamp_begin, eot = T, EOT

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)

    def encode(self, text):
        return [1000 + ord(ch) - ord("a") for ch in text if ch != " "]


def _res(tokens, temperature=0.0, avg_logprob=-0.3, no_speech_prob=0.1):
    return SimpleNamespace(tokens=tokens, avg_logprob=avg_logprob, no_speech_prob=no_speech_prob, compression_ratio=1.2,
                           temperature=temperature, language="en")


def _two_files():
    """70 s (windows at 0, 30, 60 s) and 40 s (0, 30 s); the first sample of every second names the file"""
    return [np.full(70 * 16000, 1.0, dtype=np.float32), np.full(40 * 16000, 2.0, dtype=np.float32)]


def _scripted(script):
    """decode_fn(windows, languages, prompts=None) that records its prompts and answers from ``script[file][window index]``"""
    rounds, seen = [], {1: 0, 2: 0}

    def decode_fn(windows, languages, prompts=None):
        rounds.append(None if prompts is None else [list(p) for p in prompts])
        out = []
        for w in windows:
            k = int(w[0])
            out.append(script[k][seen[k]])
            seen[k] += 1
        return out

    return decode_fn, rounds


def test_transcribe_conditions_every_file_on_its_own_previous_tokens():
    from whisper_ipa_amd.transcribe import transcribe

    # every window ends in a single timestamp: it is consumed whole
    A0, A2 = [T + 0, a, b, T + 1500], [T + 0, e, T + 500]
    B0, B1 = [T + 0, c, T + 1500], [T + 0, d, T + 500]
    script = {1: [_res(A0, temperature=0.4),                                   # 0.4: the next prompt goes on
                  _res([T + 0, f], avg_logprob=-1.5, no_speech_prob=0.9),      # no speech: skipped, appends nothing, resets nothing
                  _res(A2)],
              2: [_res(B0, temperature=0.6), _res(B1)]}                        # 0.6: the next prompt is reset
    decode_fn, rounds = _scripted(script)
    out = transcribe(None, _two_files(), language="en", decode_fn=decode_fn, tokenizer=_Tok(), condition_on_previous_text=True,
                     initial_prompt=" ab ")
    init = [a, b]
    assert len(rounds) == 3
    assert rounds[0] == [init, init]                      # round 1 carries the initial prompt's tokens
    assert rounds[1] == [init + A0, []]                   # the file's own earlier tokens, timestamps included; the 0.6 window reset B
    assert rounds[2] == [init + A0]                       # the finished file's row is gone; the skipped window left the prompt as it was
    assert out[0]["text"] == "abe" and out[1]["text"] == "cd"   # the initial prompt is not part of the text
    assert [s["seek"] for s in out[0]["segments"]] == [0, 6000] and [s["seek"] for s in out[1]["segments"]] == [0, 3000]


def test_initial_prompt_without_conditioning_reaches_the_first_window_only():
    from whisper_ipa_amd.transcribe import transcribe

    script = {1: [_res([T + 0, a, T + 1500]), _res([T + 0, b, T + 1500]), _res([T + 0, c, T + 500])],
              2: [_res([T + 0, d, T + 1500]), _res([T + 0, e, T + 500])]}
    decode_fn, rounds = _scripted(script)
    out = transcribe(None, _two_files(), language="en", decode_fn=decode_fn, tokenizer=_Tok(), initial_prompt="ab")
    assert rounds == [[[a, b], [a, b]], [[], []], [[]]]
    assert out[0]["text"] == "abc" and out[1]["text"] == "de"
    # without either option the decoder is called as ever, with no prompts argument
    decode_fn, rounds = _scripted(script={1: script[1], 2: script[2]})
    transcribe(None, _two_files(), language="en", decode_fn=decode_fn, tokenizer=_Tok())
    assert rounds == [None, None, None]


def test_the_fallback_retries_with_the_windows_prompt():
    from whisper_ipa_amd.transcribe import transcribe

    script = {1: [_res([T + 0, a, T + 1500]), _res([T + 0, b, T + 1500], avg_logprob=-2.0), _res([T + 0, c, T + 500])], 2: []}
    decode_fn, rounds = _scripted(script)
    retries = []

    def fallback_fn(results, languages, *, temperature, attempt, streams, seed, prompts=None):
        retries.append((temperature, [list(p) for p in prompts]))
        return [_res([T + 0, d, T + 1500], temperature=temperature) for _ in results]

    out = transcribe(None, _two_files()[0], language="en", decode_fn=decode_fn, fallback_fn=fallback_fn, tokenizer=_Tok(), seed=3,
                     condition_on_previous_text=True)
    first = [T + 0, a, T + 1500]
    assert retries == [(0.2, [first])]                      # the same prompt as the failed decode
    assert rounds == [[[]], [first], [first + [T + 0, d, T + 1500]]]  # 0.2 <= 0.5: the retried window feeds the next prompt
    assert out["text"] == "adc"


@pytest.mark.parametrize("kw,name", [(dict(condition_on_previous_text=True), "condition_on_previous_text"),
                                     (dict(initial_prompt="hello"), "initial_prompt")])
def test_a_decoder_without_a_prompts_parameter_is_refused(kw, name):
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(16000, dtype=np.float32)
    with pytest.raises(NotImplementedError, match=name):
        transcribe(None, audio, decode_fn=lambda windows, languages: [], tokenizer=_Tok(), **kw)
    with pytest.raises(NotImplementedError, match="fallback_fn"):
        transcribe(None, audio, decode_fn=lambda windows, languages, prompts=None: [],
                   fallback_fn=lambda results, languages, temperature, attempt, streams, seed: [], tokenizer=_Tok(), seed=1, **kw)
    for k in ("prompt", "prefix"):  # upstream's transcribe overwrites prompt itself: decode_options keeps refusing them
        with pytest.raises(NotImplementedError, match=k):
            transcribe(None, audio, decode_fn=lambda windows, languages, prompts=None: [], tokenizer=_Tok(), **{k: [1]})


# ---------------------------------------------------------------- the ragged entry points refuse bad arguments before any launch
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    return _lib


def _cfg(built, **kw):
    micro = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=2, n_vocab=51865, n_text_ctx=448,
                 n_text_state=128, n_text_head=2, n_text_layer=2, dtype=built.WIPA_F32)
    micro.update(kw)
    return built.ModelCfg(**micro)


def test_begin_ragged_refuses_bad_starts_and_widths(built):
    lib = built.lib()
    cfg = _cfg(built)
    fake = C.c_void_p(0x1000)  # never dereferenced: every check comes before the first copy
    lay = built.DecLayout()
    assert lib.wipa_decoder_layout(C.byref(cfg), 2, C.byref(lay)) == 0
    P = 8
    tokens = (C.c_int32 * (2 * P))(*([5] * (2 * P)))
    for starts, word in (([0, -1], b"start[1]"), ([8, 0], b"start[0]"), ([0, 9], b"start[1]")):
        rc = lib.wipa_decoder_begin_ragged(C.byref(cfg), fake, lay.total_bytes, 2, tokens, (C.c_int32 * 2)(*starts), P, fake, None)
        assert rc != 0 and word in lib.wipa_last_error(), lib.wipa_last_error()
    ok = (C.c_int32 * 2)(0, 7)
    for width in (0, 449):
        rc = lib.wipa_decoder_begin_ragged(C.byref(cfg), fake, lay.total_bytes, 2, tokens, ok, width, fake, None)
        assert rc != 0 and b"P=" in lib.wipa_last_error()
    bad = (C.c_int32 * (2 * P))(*([5] * (2 * P - 1) + [51865]))
    rc = lib.wipa_decoder_begin_ragged(C.byref(cfg), fake, lay.total_bytes, 2, bad, ok, P, fake, None)
    assert rc != 0 and b"tokens[1][7]" in lib.wipa_last_error()
    rc = lib.wipa_decoder_begin_ragged(C.byref(cfg), fake, lay.total_bytes - 1, 2, tokens, ok, P, fake, None)
    assert rc != 0 and b"state blob" in lib.wipa_last_error()
    rc = lib.wipa_decoder_begin_ragged(C.byref(cfg), fake, lay.total_bytes, 2, tokens, ok, P, None, None)
    assert rc != 0
    fp8 = _cfg(built, dtype=built.WIPA_BF16, dec_w_dtype=built.WIPA_FP8_E4M3)
    rc = lib.wipa_decoder_begin_ragged(C.byref(fp8), fake, 1 << 40, 2, tokens, ok, P, fake, None)
    assert rc != 0 and b"fp8" in lib.wipa_last_error() and b"dec_w_dtype" in lib.wipa_last_error()


def test_run_ragged_refuses_what_the_step_cannot_serve(built, monkeypatch):
    lib = built.lib()
    cfg = _cfg(built)
    fake = C.c_void_p(0x1000)
    tab = (C.c_void_p * 64)()
    lay = built.DecLayout()
    assert lib.wipa_decoder_layout(C.byref(cfg), 2, C.byref(lay)) == 0

    def run(cfg, n_init, n_steps, starts=0x1000):
        call = built.DecodeCall(n_init=n_init, eot=EOT, mask_first=0x1000, mask_always=0x1000, starts_dev=starts)
        rc = lib.wipa_decoder_run_ex(C.byref(cfg), tab, fake, lay.total_bytes, 2, C.byref(call), n_steps, 0, None)
        assert rc == 0 or lib.wipa_last_error().startswith(b"wipa_decoder_run_ex: ")
        return rc

    assert run(cfg, 227, 448) != 0 and b"n_steps" in lib.wipa_last_error() and b"n_text_ctx" in lib.wipa_last_error()
    assert run(cfg, 449, 1) != 0 and b"P=449" in lib.wipa_last_error()
    assert run(cfg, 0, 1) != 0 and b"P=0" in lib.wipa_last_error()
    fp8 = _cfg(built, dtype=built.WIPA_BF16, dec_w_dtype=built.WIPA_FP8_E4M3)
    assert run(fp8, 8, 1) != 0 and b"fp8" in lib.wipa_last_error() and b"starts_dev" in lib.wipa_last_error()
    monkeypatch.setenv("WIPA_DECODE_FUSED", "1")
    assert run(cfg, 8, 1) != 0 and b"WIPA_DECODE_FUSED" in lib.wipa_last_error() and b"starts_dev" in lib.wipa_last_error()
    monkeypatch.delenv("WIPA_DECODE_FUSED")
    monkeypatch.setenv("WIPA_DECODE_TAIL", "0")
    assert run(cfg, 8, 1) != 0 and b"WIPA_DECODE_TAIL" in lib.wipa_last_error()
