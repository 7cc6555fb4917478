"""CPU: the word-timestamp restatement (tests/alignment_ref.py) against the fixture recorded from transformers'
_median_filter / _dynamic_time_warping and the _extract_token_timestamps chain (tools/make_golden_alignment.py), the word
splitter on IPA, merge_punctuations, the ``transcribe(word_timestamps=True)`` plumbing on scripted decodes and alignments, and
the three input forms of ``Whisper.set_alignment_heads``.  Reference: openai-whisper timing.py, which mlx_whisper ports
([UPSTREAM-UNVERIFIED])."""
import base64
import gzip
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import alignment_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "alignment.npz")


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    return np.load(GOLDEN)


def _cases(g, kind):
    return sorted({k.split("/")[1] for k in g.files if k.startswith(kind + "/")})


def test_dtw_restatement_equals_the_recorded_paths(golden):
    names = _cases(golden, "dtw")
    assert len(names) >= 10
    shapes = set()
    for n in names:
        x = golden[f"dtw/{n}/x"]
        assert x.dtype == np.float32
        ti, tj, cost, _ = AR.dtw_f32(x)
        assert cost.dtype == np.float32
        assert ti.tolist() == golden[f"dtw/{n}/text"].tolist() and tj.tolist() == golden[f"dtw/{n}/time"].tolist(), n
        shapes.add(x.shape)
    # what the fixture has to hold: ties, one row, one column, more rows than columns
    assert any(n.startswith("ties_all_equal") for n in names) and any(n.startswith("ties_quarter") for n in names)
    assert any(s[0] == 1 and s[1] > 1 for s in shapes) and any(s[1] == 1 and s[0] > 1 for s in shapes) and any(s[0] > s[1] > 1 for s in shapes)


def test_weights_chain_restatement_equals_the_recorded_chain(golden):
    names = _cases(golden, "chain")
    frames = set()
    for n in names:
        nf = int(golden[f"chain/{n}/n_frames"])
        m = AR.weights_chain(golden[f"chain/{n}/qk"], nf, np.float64)
        assert m.dtype == np.float64 and m.shape == golden[f"chain/{n}/matrix"].shape
        assert np.abs(m - golden[f"chain/{n}/matrix"]).max() < 1e-12, n
        frames.add(nf)
    assert {3, 4, 7} <= frames  # no filter at 3 frames, the reflect padding at its smallest at 4, exactly one window at 7


def test_median_filter_edges():
    x = np.arange(3.0)[None]
    assert AR.median_filter(x) is x  # <= 3 frames: left as it is
    x = np.array([[5.0, 1.0, 4.0, 2.0]])  # reflect: 2 4 1 | 5 1 4 2 | 4 1 5
    assert AR.median_filter(x).tolist() == [[2.0, 4.0, 2.0, 4.0]]


def _tok(language="en"):
    from whisper_ipa_amd.tokenizer import get_tokenizer

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return get_tokenizer(True, language=language, task="transcribe")


@pytest.mark.parametrize("text", ["ðə kwɪk bɹaʊn fɑks", " tʰɪs ɪz ə tɛst, n̩ oʊˈkeɪ!", "ʃ", " (ɑ) \"ɛ\" ʒ-ʒ"])
def test_split_to_word_tokens_on_ipa(text):
    tok = _tok()
    ids = tok.encode(text)
    assert len(ids) > len(text.replace(" ", "")) or tok.byte_fallback is False  # characters straddle tokens in the byte vocabulary
    words, word_tokens = tok.split_to_word_tokens(ids + [tok.eot])
    assert [t for w in word_tokens for t in w] == ids + [tok.eot]
    assert word_tokens[-1] == [tok.eot]
    assert "".join(words[:-1]) == tok.decode(ids) == text
    assert all("�" not in w for w in words)
    for w, wt in zip(words[:-1], word_tokens[:-1]):
        assert tok.decode(wt) == w
    # a word opens at a space or at a punctuation piece; nothing else splits words
    import string

    for k, w in enumerate(words[:-1]):
        assert k == 0 or w[0] == " " or w[0] in string.punctuation, (k, w)
    # the unicode splitter alone: one piece per character that straddles tokens, each a whole character
    pieces, piece_tokens = tok.split_tokens_on_unicode(ids)
    assert "".join(pieces) == text and all("�" not in p for p in pieces)
    if tok.byte_fallback:
        assert any(len(t) > 1 for t in piece_tokens)  # a multi-byte IPA symbol took more than one token


def test_split_on_unicode_for_languages_without_spaces():
    tok = _tok("ja")
    ids = tok.encode("ɪ ʃ")
    words, word_tokens = tok.split_to_word_tokens(ids)
    assert "".join(words) == "ɪ ʃ" and [t for w in word_tokens for t in w] == ids
    assert len(words) >= 2 and all("\ufffd" not in w for w in words)  # cut at characters, not at spaces: "ɪ" stands alone
    assert words[0] == "ɪ"


def test_a_genuine_replacement_character_closes_its_piece():
    """a token that IS U+FFFD closes its piece (the full decoding has the character at the same place); a token that only
    decodes to U+FFFD because its character is incomplete does not"""
    from whisper_ipa_amd.tokenizer import Tokenizer

    table = {1: b"a", 2: "\ufffd".encode(), 3: "ʃ".encode()[:1], 4: "ʃ".encode()[1:], 5: b"b"}
    stub = SimpleNamespace(decode_with_timestamps=lambda ids: b"".join(table[int(i)] for i in ids).decode("utf-8", errors="replace"))
    pieces, piece_tokens = Tokenizer.split_tokens_on_unicode(stub, [1, 2, 3, 4, 5])
    assert pieces == ["a", "\ufffd", "ʃ", "b"] and piece_tokens == [[1], [2], [3, 4], [5]]


def _wt(word, tokens, start=0.0, end=0.0):
    from whisper_ipa_amd.timing import WordTiming

    return WordTiming(word, list(tokens), start, end, 1.0)


def test_merge_punctuations_both_passes():
    from whisper_ipa_amd.timing import merge_punctuations

    al = [_wt(" (", [1]), _wt("ab", [2, 3]), _wt(")", [4]), _wt(",", [5]), _wt(" cd", [6]), _wt(" \"", [7]), _wt(" '", [8]), _wt("ef", [9]),
          _wt(".", [10])]
    merge_punctuations(al)
    assert [(w.word, w.tokens) for w in al] == [("", []), (" (ab),", [1, 2, 3, 4, 5]), ("", []), ("", []), (" cd", [6]), ("", []), ("", []),
                                                 (" \" 'ef.", [7, 8, 9, 10]), ("", [])]
    # prepended: only with a leading space; appended: not after a word that ends in a space
    al = [_wt("(", [1]), _wt("ab ", [2]), _wt(".", [3])]
    merge_punctuations(al)
    assert [(w.word, w.tokens) for w in al] == [("(", [1]), ("ab ", [2]), (".", [3])]
    al = [_wt(" ab", [1]), _wt("!", [2])]
    merge_punctuations(al, prepended="", appended="")
    assert [w.word for w in al] == [" ab", "!"]
    merge_punctuations([])  # nothing to do, nothing to fail


def test_words_from_path_known_answer():
    from whisper_ipa_amd.timing import words_from_path

    tok = _tok()
    text = " pa ta"
    ids = tok.encode(text)  # byte vocabulary or merges: the word split is what counts
    words, word_tokens = tok.split_to_word_tokens(ids + [tok.eot])
    assert words[:-1] == [" pa", " ta"]
    n = len(ids) + 1
    # a staircase path: row r holds frames 10 r .. 10 r + 9
    ti = np.repeat(np.arange(n), 10)
    tj = np.arange(10 * n)
    probs = np.linspace(0.1, 0.9, len(ids))
    out = words_from_path(tok, ids, ti, tj, probs)
    starts, ends = AR.word_times(ti, tj, word_tokens)
    k = len(word_tokens[0])
    assert [w.word for w in out] == [" pa", " ta"] and [w.tokens for w in out] == word_tokens[:-1]
    assert [w.start for w in out] == pytest.approx([0.0, 0.2 * k]) and [w.end for w in out] == pytest.approx([0.2 * k, 0.2 * len(ids)])
    assert [w.start for w in out] == pytest.approx(starts.tolist()) and [w.end for w in out] == pytest.approx(ends.tolist())
    assert out[0].probability == pytest.approx(probs[:k].mean()) and out[1].probability == pytest.approx(probs[k:].mean())
    assert words_from_path(tok, [], [], [], []) == []


# ---------------------------------------------------------------- transcribe(word_timestamps=True) on scripts
T = 50364
a, b, c, d = 1000, 1001, 1002, 1003


class _Tok:
    timestamp_begin, eot = T, 50257

    def decode(self, ids):
        return "".join(chr(ord("a") + (int(i) - 1000)) for i in ids if int(i) < self.eot)


def _res(tokens):
    return SimpleNamespace(tokens=tokens, avg_logprob=-0.3, no_speech_prob=0.1, compression_ratio=1.2, temperature=0.0, language="en")


def test_transcribe_word_timestamps_deals_words_to_segments_and_applies_the_offset():
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(38 * 16000, dtype=np.float32)
    script = [_res([T + 0, a, b, T + 100, T + 100, c, T + 250, T + 250, d, T + 400, T + 400]),  # three segments, advance 8 s
              _res([T + 0, a, b])]                                                            # second window at 8 s: 30 s of content
    calls, aligned = [], []

    def decode_fn(windows, languages):
        calls.append(len(windows))
        return [script[len(calls) - 1]]

    def align_fn(results, text_tokens, num_frames, languages):
        aligned.append((list(results), [list(t) for t in text_tokens], list(num_frames), list(languages)))
        out = []
        for toks in text_tokens:  # one word per token, half a second each
            out.append([_wt(f" {chr(ord('a') + t - 1000)}", [t], 0.5 * k, 0.5 * k + 0.5) for k, t in enumerate(toks)])
        return out

    out = transcribe(None, audio, decode_fn=decode_fn, align_fn=align_fn, tokenizer=_Tok(), word_timestamps=True, language="en")
    plain_calls = []

    def plain_decode(windows, languages):
        plain_calls.append(len(windows))
        return [script[len(plain_calls) - 1]]

    plain = transcribe(None, audio, decode_fn=plain_decode, tokenizer=_Tok(), language="en")
    assert len(aligned) == 2  # one alignment call a round
    assert aligned[0][0] == [script[0]] and aligned[0][1] == [[a, b, c, d]] and aligned[0][2] == [3000] and aligned[0][3] == ["en"]
    assert aligned[1][1] == [[a, b]] and aligned[1][2] == [3000]
    segs = out["segments"]
    assert [[w["word"] for w in s["words"]] for s in segs] == [[" a", " b"], [" c"], [" d"], [" a", " b"]]
    assert [(w["start"], w["end"]) for w in segs[0]["words"]] == [(0.0, 0.5), (0.5, 1.0)]
    assert [(w["start"], w["end"]) for w in segs[1]["words"]] == [(1.0, 1.5)] and [(w["start"], w["end"]) for w in segs[2]["words"]] == [(1.5, 2.0)]
    assert [(w["start"], w["end"]) for w in segs[3]["words"]] == [(8.0, 8.5), (8.5, 9.0)]  # the second window starts at 8 s
    assert all(set(w) == {"word", "start", "end", "probability"} for s in segs for w in s["words"])
    # word_timestamps=False is what it was: the same segments without "words"
    assert [{k: v for k, v in s.items() if k != "words"} for s in segs] == plain["segments"] and out["text"] == plain["text"]
    assert all("words" not in s for s in plain["segments"])


def test_transcribe_word_timestamps_merges_punctuation_and_skips_emptied_words():
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(10 * 16000, dtype=np.float32)

    def align_fn(results, text_tokens, num_frames, languages):
        assert num_frames == [1000]
        return [[_wt(" (", [a], 0.0, 0.1), _wt("b", [b], 0.1, 0.4), _wt(")", [c], 0.4, 0.5)]]

    kw = dict(decode_fn=lambda w, l: [_res([T + 0, a, b, c, T + 50])], align_fn=align_fn, tokenizer=_Tok(), word_timestamps=True, language="en")
    out = transcribe(None, audio, **kw)
    assert [(w["word"], w["start"], w["end"]) for w in out["segments"][0]["words"]] == [(" (b)", 0.1, 0.4)]
    out = transcribe(None, audio, prepend_punctuations="", append_punctuations="", **kw)
    assert [w["word"] for w in out["segments"][0]["words"]] == [" (", "b", ")"]


def test_word_timestamps_without_a_model_needs_an_align_fn():
    from whisper_ipa_amd.transcribe import transcribe

    with pytest.raises(NotImplementedError, match="word_timestamps"):
        transcribe(None, np.zeros(16000, dtype=np.float32), decode_fn=lambda w, l: [], tokenizer=_Tok(), word_timestamps=True)


# ---------------------------------------------------------------- alignment heads
def test_set_alignment_heads_round_trips_its_three_forms():
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper.__new__(Whisper)  # the head list is host state: no GPU, no weights
    m.dims = ModelDimensions(80, 1500, 384, 6, 4, 51865, 448, 384, 6, 4)
    assert m.alignment_heads == [(l, h) for l in (2, 3) for h in range(6)]  # the last half of the layers
    pairs = [(3, 1), (1, 0), (2, 5)]
    m.set_alignment_heads(pairs)
    assert m.alignment_heads == pairs  # pairs keep their order: it is the order of the sum
    mask = np.zeros((4, 6), dtype=bool)
    for l, h in pairs:
        mask[l, h] = True
    m.set_alignment_heads(mask)
    assert m.alignment_heads == sorted(pairs)
    dump = base64.b85encode(gzip.compress(mask.tobytes()))
    m.set_alignment_heads(None)
    m.set_alignment_heads(dump)
    assert m.alignment_heads == sorted(pairs)
    m.set_alignment_heads(dump.decode())
    assert m.alignment_heads == sorted(pairs)
    back = np.zeros((4, 6), dtype=bool)
    for l, h in m.alignment_heads:
        back[l, h] = True
    assert (back == mask).all()
    for bad in ([(4, 0)], [(0, 6)], [(1, 1), (1, 1)], np.zeros((4, 6), dtype=bool), np.zeros((3, 6), dtype=bool),
                base64.b85encode(gzip.compress(np.zeros(5, dtype=bool).tobytes()))):
        with pytest.raises(ValueError):
            m.set_alignment_heads(bad)
    m.set_alignment_heads(None)
    assert len(m.alignment_heads) == 12


# ---------------------------------------------------------------- the entry points refuse bad sizes before any launch
def test_dtw_and_align_entry_points_check_the_host_sizes_first():
    """No GPU is touched: the host copies of the per-clip sizes are checked before the launch, and fp8 tables are refused."""
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from whisper_ipa_amd import _lib

    lib = _lib.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def dtw(n_rows, n_cols, first_row=0, rows_avail=448, ld=1500, ld_path=1948):
        return lib.wipa_dtw_batch(fake, rows_avail * ld, ld, first_row, rows_avail, fake, fake, i32(*n_rows), i32(*n_cols), len(n_rows), fake,
                                  1 << 30, fake, fake, ld_path, fake, None)

    for kw, word in ((dict(n_rows=[3, 449], n_cols=[5, 5]), b"clip 1"), (dict(n_rows=[-1], n_cols=[5]), b"clip 0"),
                     (dict(n_rows=[3], n_cols=[1501]), b"frames"), (dict(n_rows=[3], n_cols=[0]), b"frames"),
                     (dict(n_rows=[446], n_cols=[5], first_row=3), b"rows"), (dict(n_rows=[400], n_cols=[1500], ld_path=1899), b"path")):
        assert dtw(**kw) != 0 and word in lib.wipa_last_error(), (kw, lib.wipa_last_error())
    assert lib.wipa_dtw_batch(fake, 0, 0, 0, 0, fake, fake, None, None, 0, None, 0, fake, fake, 0, fake, None) == 0  # B = 0: nothing to do
    assert lib.wipa_dtw_scratch_bytes(2, 448) == 2 * 448 * 94 * 4

    small = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=768, n_audio_head=12, n_audio_layer=12, n_vocab=51865, n_text_ctx=448,
                 n_text_state=768, n_text_head=12, n_text_layer=12, dtype=_lib.WIPA_BF16)
    tab = (C.c_void_p * 4)()

    def align(cfg, heads, n_tok, n_fr, n_row, T=64, ws=1 << 40):
        return lib.wipa_decoder_align(C.byref(cfg), tab, fake, fake, i32(*[x for p in heads for x in p]), len(heads), fake, fake, fake,
                                      i32(*n_tok), i32(*n_fr), i32(*n_row), 3, 50257, fake, fake, fake, T + 1500, fake, fake, 0, fake, ws,
                                      len(n_tok), T, None)

    cfg = _lib.ModelCfg(**small)
    assert align(_lib.ModelCfg(**small, dec_w_dtype=_lib.WIPA_FP8_E4M3), [(6, 0)], [10], [1500], [6]) != 0 and b"fp8" in lib.wipa_last_error()
    assert align(cfg, [(12, 0)], [10], [1500], [6]) != 0 and b"alignment head" in lib.wipa_last_error()
    assert align(cfg, [(6, 0), (6, 0)], [10], [1500], [6]) != 0 and b"twice" in lib.wipa_last_error()
    assert align(cfg, [(6, 0)], [65], [1500], [6]) != 0 and b"tokens" in lib.wipa_last_error()
    assert align(cfg, [(6, 0)], [10], [1501], [6]) != 0 and b"frames" in lib.wipa_last_error()
    assert align(cfg, [(6, 0)], [10], [1500], [8]) != 0 and b"rows" in lib.wipa_last_error()
    assert align(cfg, [(6, 0)], [10], [1500], [6], ws=1024) != 0 and b"workspace" in lib.wipa_last_error()
    need = lib.wipa_decoder_align_workspace_bytes(C.byref(cfg), 64, 64, 72, 0)
    base = lib.wipa_decoder_logits_workspace_bytes(C.byref(cfg), 64, 64)
    assert base < need < base + (1 << 30) + (64 << 20) + 64 * 64 * 94 * 4 + 4096  # at most 1 GiB of logits on top of the pass


def test_align_refuses_long_audio_and_mismatched_transcripts():
    from whisper_ipa_amd.timing import align

    tok = _tok()
    with pytest.raises(ValueError, match="30 s"):
        align(None, np.zeros(31 * 16000, dtype=np.float32), " a", tokenizer=tok)
    with pytest.raises(ValueError, match="transcripts"):
        align(None, [np.zeros(16000, dtype=np.float32)], [" a", " b"], tokenizer=tok)


def test_an_emptied_segment_is_aligned_with_its_tokens_and_keeps_no_words():
    """a zero-length segment with text: its tokens go into the alignment with the window's others, as upstream aligns before it
    clears such a segment; it then keeps no words, and its neighbours keep theirs"""
    from whisper_ipa_amd.transcribe import transcribe

    audio = np.zeros(10 * 16000, dtype=np.float32)
    seen = []

    def align_fn(results, text_tokens, num_frames, languages):
        seen.append([list(t) for t in text_tokens])
        return [[_wt(f" {chr(ord('a') + t - 1000)}", [t], 0.5 * k, 0.5 * k + 0.5) for k, t in enumerate(toks)] for toks in text_tokens]

    tokens = [T + 0, a, T + 100, T + 100, b, T + 100, T + 100, c, T + 200]  # the middle segment starts and ends at 2.00 s
    out = transcribe(None, audio, decode_fn=lambda w, l: [_res(tokens)], align_fn=align_fn, tokenizer=_Tok(), word_timestamps=True,
                     language="en")
    assert seen == [[[a, b, c]]]
    segs = out["segments"]
    assert [s["tokens"] for s in segs] == [[T + 0, a, T + 100], [], [T + 100, c, T + 200]] and [s["text"] for s in segs] == ["a", "", "c"]
    assert [[w["word"] for w in s["words"]] for s in segs] == [[" a"], [], [" c"]]
    assert [(w["start"], w["end"]) for w in segs[2]["words"]] == [(1.0, 1.5)]  # c is the third word of the window, not the second


def test_word_timestamps_refuses_an_fp8_model_before_decoding():
    from whisper_ipa_amd.transcribe import transcribe

    fp8_model = SimpleNamespace(_fp8={"decoder.token_embedding.weight": None}, is_multilingual=True, num_languages=99)
    with pytest.raises(NotImplementedError, match="fp8"):
        transcribe(fp8_model, np.zeros(16000, dtype=np.float32), tokenizer=_Tok(), word_timestamps=True, language="en")
