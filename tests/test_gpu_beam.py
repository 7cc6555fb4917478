"""GPU: beam search -- the BEAM instantiation of the decode self-attention (an ancestor table instead of a permuted cache), the beam tail
(csrc/beam.hip: wipa_beam_step / wipa_beam_finalize) on crafted rows, and decode through the beam entry points against the numpy
restatement of tests/beam_ref.py.  Reference: upstream's BeamSearchDecoder + MaximumLikelihoodRanker.  ``pytest -m gpu`` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_cases as BC
import beam_ref as BM
import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

SP = PR.SP
STEP_LOGPROB_TOL = 1e-3    # what tests/test_gpu_timestamps.py allows a step tail's added log-probability
DECODE_LOGPROB_TOL = 1e-2  # ... and a whole decode's sum_logprobs against the oracle


# ---------------------------------------------------------------- 1. BEAM self-attention
def _attn_beam(q, k, v, Tk, anc, G):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.ops import dt_code
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    B, _, H, _ = q.shape
    with on_stream() as s:
        out = torch.empty(B, H, 64, dtype=q.dtype, device=q.device)
        d = _lib.AttnDesc()
        d.q, d.k, d.v, d.out = ptr(q), ptr(k), ptr(v), ptr(out)
        d.q_bs, d.q_rs, d.q_hs = q.stride(0), q.stride(1), q.stride(2)
        d.k_bs, d.k_rs, d.k_hs = k.stride(0), k.stride(1), k.stride(2)
        d.v_bs, d.v_rs, d.v_hs = v.stride(0), v.stride(1), v.stride(2)
        d.o_bs, d.o_rs, d.o_hs = out.stride(0), out.stride(0), out.stride(1)
        d.B, d.H, d.Tq, d.Tk, d.causal, d.dtype = B, H, 1, Tk, 0, dt_code(q.dtype)
        _lib.check(L.wipa_decode_attn_beam(C.byref(d), ptr(anc), anc.stride(0), G, sptr(s)), "wipa_decode_attn_beam")
        s.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G", [2, 5])
def test_beam_attention_equals_plain_attention_on_a_gathered_cache(G, dtype):
    from whisper_ipa_amd import ops

    clips, H, T_buf = 2, 2, 208
    B = clips * G
    gen = torch.Generator().manual_seed(10 * G + (dtype == torch.bfloat16))
    q = torch.randn(B, 1, H, 64, generator=gen).to(dtype).cuda()
    k = torch.randn(B, T_buf, H, 64, generator=gen).to(dtype).cuda()
    v = torch.randn(B, T_buf, H, 64, generator=gen).to(dtype).cuda()
    rows = torch.arange(B) % G
    identity = rows[:, None].expand(B, T_buf).contiguous().to(torch.uint8).cuda()
    table = torch.randint(0, G, (B, T_buf), generator=gen).to(torch.uint8)
    phys = (torch.arange(B) - rows)[:, None] + table.long()            # [B, T]: the physical row of every key
    tt = torch.arange(T_buf)[None].expand(B, T_buf)
    kg, vg = k[phys.cuda(), tt.cuda()].contiguous(), v[phys.cuda(), tt.cuda()].contiguous()
    assert not torch.equal(kg, k)
    for Tk in (1, 31, 33, 129, 200):  # both sides of the 32-key and the 128-key partition edges
        plain = ops.decode_attn(q, k, v, Tk=Tk)
        assert torch.equal(_attn_beam(q, k, v, Tk, identity, G), plain), (G, dtype, Tk, "identity table")
        gathered = ops.decode_attn(q, kg, vg, Tk=Tk)
        assert torch.equal(_attn_beam(q, k, v, Tk, table.cuda(), G), gathered), (G, dtype, Tk, "random table")


# ---------------------------------------------------------------- 2. wipa_beam_step on crafted rows
def _up256(n):
    return (n + 255) // 256 * 256


def _beam_parts(buf, B, G, maxc, ld_tok):
    """the documented layout of the beam buffer (include/wipa.h) -> dict of host arrays"""
    clips, cap = B // G, max(G, maxc)
    raw = buf.cpu().numpy()
    o = 0
    out = {}

    def take(name, nbytes, dtype, shape):
        nonlocal o
        out[name] = raw[o:o + nbytes].view(dtype).reshape(shape).copy()
        o += _up256(nbytes)

    take("anc", B * ld_tok, np.uint8, (B, ld_tok))
    take("cand", B * (G + 1) * 8, np.int32, (B, G + 1, 2))
    take("src", B * 4, np.int32, (B,))
    take("fin_tok", clips * cap * ld_tok * 4, np.int32, (clips, cap, ld_tok))
    take("fin_score", clips * cap * 4, np.float32, (clips, cap))
    take("fin_len", clips * cap * 4, np.int32, (clips, cap))
    take("fin_count", clips * 4, np.int32, (clips,))
    o += 256
    assert o == raw.size, (o, raw.size)  # the buffer has the documented size
    return out


@pytest.mark.parametrize("scene", sorted(BC.SCENES))
def test_beam_step_on_crafted_rows_matches_the_restatement(scene):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    G, patience, steps, with_rules = BC.SCENES[scene]
    maxc = round(G * (patience or 1.0))
    clips, V, ld_tok, ldl = 2, BC.V, 40, BC.V + 1
    B = clips * G
    rng = np.random.default_rng(len(scene))
    first_scene = steps[0][1]
    n_gen = 0 if first_scene else 2
    hist = np.zeros((B, ld_tok), dtype=np.int32)
    hist[:, :BC.N_INIT] = BC.INITIAL
    if n_gen:
        hist[:, BC.N_INIT:BC.N_INIT + n_gen] = rng.integers(10, 800, size=(B, n_gen))
        if with_rules:
            hist[:, BC.N_INIT:BC.N_INIT + 2] = BC.TB + 3  # a closed pair: the step after it offers text only
    sums0 = np.zeros(B, dtype=np.float32) if first_scene else (-(rng.random(B) * 3 + 0.5)).astype(np.float32)
    ref = [BM.Clip(hist[c * G:(c + 1) * G, :BC.N_INIT + n_gen].astype(np.int64), sums0[c * G:(c + 1) * G].copy(),
                   anc=np.tile((np.arange(G) % G)[:, None], (1, ld_tok)).astype(np.uint8)) for c in range(clips)]
    mask = np.zeros(V, dtype=np.float32)
    rules = _lib.DecodeRules(BC.TB, BC.NT, 50) if with_rules else None
    with on_stream() as s:
        d_tok, d_sum = torch.from_numpy(hist).cuda(), torch.from_numpy(sums0).cuda()
        d_mask = torch.from_numpy(mask).cuda()
        pos = torch.tensor([BC.N_INIT + n_gen - 1], dtype=torch.int32, device="cuda")
        nd = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        nbytes = int(L.wipa_beam_bytes(B, G, maxc, ld_tok))
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        _lib.check(L.wipa_beam_begin(ptr(buf), nbytes, B, G, maxc, ld_tok, sptr(s)), "wipa_beam_begin")
        for i, (eot_rank, first) in enumerate(steps):
            logits = BC.crafted_rows(1000 * len(scene) + i, G, clips, eot_rank)
            if with_rules:
                logits[:, BC.TB + 5 + i] = np.float32(5.5)  # a timestamp among the rows' best three, had the rules not closed the pair
            padded = np.zeros((B, ldl), dtype=np.float32)
            padded[:, :V] = logits
            d_logits = torch.from_numpy(padded).cuda()
            _lib.check(L.wipa_beam_step(ptr(d_logits), ldl, B, V, ptr(d_mask), ptr(d_mask), ptr(d_tok), ld_tok, ptr(pos), BC.N_INIT, BC.EOT,
                                        C.byref(rules) if rules is not None else None, ptr(buf), G, maxc, ptr(d_sum), ptr(nd), sptr(s)),
                       "wipa_beam_step")
            s.synchronize()
            p = int(pos.cpu()[0])
            got_tok, got_sum, parts = d_tok.cpu().numpy(), d_sum.cpu().numpy(), _beam_parts(buf, B, G, maxc, ld_tok)
            incomplete = 0
            for c in range(clips):
                clip = ref[c]
                rows = [BM.filtered_row(logits[c * G + j], mask, BC.RULES if with_rules else None, clip.tokens[j, BC.N_INIT:].tolist(), BC.EOT,
                                        first) for j in range(G)]
                before = clip.margin
                clip.margin = np.inf
                BM.update(clip, rows, BC.EOT, maxc, first)
                if BM.complete(clip, maxc) and len(clip.finished) < G:  # patience below 1: the completing step is where upstream finalizes
                    BM.finalize(clip, BC.EOT)
                assert clip.margin >= BC.CRAFT_GAP, (scene, i, c, clip.margin)  # the crafted gaps are what they claim to be
                clip.margin = min(before, clip.margin)
                sl = slice(c * G, (c + 1) * G)
                case = (scene, i, c)
                assert (parts["src"][sl] == clip.src).all(), (case, parts["src"][sl], clip.src)
                assert (got_tok[sl, :p + 2] == clip.tokens).all(), (case, got_tok[sl, :p + 2], clip.tokens)
                assert (parts["anc"][sl, :p + 1] == clip.anc[:, :p + 1]).all(), case
                assert (parts["anc"][sl, p + 1:] == (np.arange(G) % G)[:, None]).all(), case  # untouched columns keep the identity
                assert np.abs(got_sum[sl] - clip.sums).max() < STEP_LOGPROB_TOL, (case, got_sum[sl], clip.sums)
                clip.sums = got_sum[sl].copy()  # the next step adds to the device's sums: every comparison is of ONE step's arithmetic
                assert parts["fin_count"][c] == len(clip.finished) <= max(G, maxc), (case, parts["fin_count"][c], len(clip.finished))
                for kk, (seq, score) in enumerate(clip.finished):
                    assert parts["fin_tok"][c, kk, :len(seq)].tolist() == seq, (case, kk)
                    assert parts["fin_len"][c, kk] == len(seq) - 1 - BC.N_INIT, (case, kk)
                    assert abs(parts["fin_score"][c, kk] - score) < STEP_LOGPROB_TOL, (case, kk)
                    clip.finished[kk] = (seq, np.float32(parts["fin_score"][c, kk]))
                incomplete += int(not BM.complete(clip, maxc))
            assert int(nd.cpu()[0]) == incomplete, (scene, i)
            pos += 1
        # wipa_beam_finalize on the store the scene leaves: fill-up with the live beams, then the ranking, at both length penalties
        from whisper_ipa_amd.decoding import length_penalty_table

        n = int(pos.cpu()[0]) + 1 - BC.N_INIT
        for lp in (None, 0.6):
            pen = torch.from_numpy(length_penalty_table(n, lp)).cuda()
            width = BC.N_INIT + n + 1
            best = torch.full((clips, width), -7, dtype=torch.int32, device="cuda")
            best_sum = torch.zeros(clips, dtype=torch.float32, device="cuda")
            best_len = torch.zeros(clips, dtype=torch.int32, device="cuda")
            _lib.check(L.wipa_beam_finalize(ptr(buf), ptr(d_tok), ld_tok, B, G, maxc, BC.N_INIT, n, BC.EOT, ptr(d_sum), ptr(pen), ptr(best), width,
                                            ptr(best_sum), ptr(best_len), sptr(s)), "wipa_beam_finalize")
            s.synchronize()
            parts = _beam_parts(buf, B, G, maxc, ld_tok)
            for c in range(clips):
                done = BM.Clip(ref[c].tokens.copy(), ref[c].sums.copy(), finished=list(ref[c].finished))
                BM.finalize(done, BC.EOT)
                k, toks, score = BM.rank(done, BC.N_INIT, BC.EOT, lp)
                case = (scene, "finalize", lp, c)
                assert parts["fin_count"][c] == len(done.finished) >= G, case
                assert [parts["fin_len"][c, kk] for kk in range(len(done.finished))] == [len(seq) - 1 - BC.N_INIT for seq, _ in done.finished], case
                assert int(best_len.cpu()[c]) == len(toks), (case, int(best_len.cpu()[c]), len(toks), k)
                row = best.cpu().numpy()[c]
                assert row[BC.N_INIT:BC.N_INIT + len(toks)].tolist() == [int(t) for t in toks], case
                assert (row[BC.N_INIT + len(toks):] == BC.EOT).all(), case
                assert np.float32(best_sum.cpu()[c]) == np.float32(score), case  # the ref's scores were taken from the device's store
    lengths = {len(seq) for c in ref for seq, _ in c.finished}
    if scene in ("store_overflow_patience_2", "completes_then_steps_on"):
        assert len(lengths) >= 2  # the ranking saw sequences of different lengths
    if "overflow" in scene:
        assert all(len(c.finished) == maxc for c in ref)  # the store did fill, and the later EOTs were turned away
    if "rules" in scene:
        assert all((c.tokens[:, -1] < BC.TB).all() for c in ref)  # behind the pair: text


# ---------------------------------------------------------------- 3.-6. the decode
@pytest.fixture(scope="module")
def models():
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("micro"):
                W, xa = BC.micro_fixture()
                dims, dtype = PR.MICRO, torch.float32
            else:
                dims, dtype = PR.W384, torch.bfloat16
                if "W384" not in cache:
                    W = R.synthetic_weights(dims, seed=1)
                    with torch.no_grad():
                        cache["W384"] = (W, R.encoder_forward(W, dims, PR.clip_mels()))
                W, xa = cache["W384"]
            m = Whisper(ModelDimensions(**dims.__dict__), dtype=dtype, cross_attention=name.split("_")[1])
            m.load_weights(W)
            cache[name] = (m, xa.cuda())
        return cache[name]

    return get


def _gpu_rules(timed):
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(SP.timestamp_begin, SP.no_timestamps, 50) if timed else None


@pytest.mark.parametrize("G,patience,timed", BC.MODEL_CASES)
def test_beam_decode_matches_the_restatement(models, G, patience, timed):
    """exact ids against the f32 restatement.  The f32 model decodes with cached cross K / V: the absorbed form exists for bf16 models
    only, where it is held to the bit-exact properties below (a beam of one is the greedy decode, a clip alone is the clip in a batch)"""
    from whisper_ipa_amd.decoding import Beams, greedy_decode_tokens

    cross = "cached"
    model, xa = models("micro_" + cross)
    initial, always, first, _ = BC.decode_inputs(timed)
    maxc = round(G * (patience or 1.0))
    for lp in BC.LENGTH_PENALTIES:
        want = BC.restated(G, patience, timed, lp)
        for use_graph in (True, False):
            g = greedy_decode_tokens(model, xa, initial, always, first, SP.eot, max_new_tokens=BC.SAMPLE_LEN, rules=_gpu_rules(timed), n_group=G,
                                     length_penalty=lp, beams=Beams(maxc), use_graph=use_graph, check_every=4)
            for c, w in enumerate(want):
                n = int(g.lengths[c, 0])
                got = g.tokens[c, len(initial):len(initial) + n].tolist()
                case = (G, patience, timed, cross, lp, use_graph, c)
                assert got == w.tokens, (case, got, w.tokens, float(g.sum_logprobs[c]), float(w.sum_logprob))
                assert abs(float(g.sum_logprobs[c]) - float(w.sum_logprob)) < DECODE_LOGPROB_TOL, case


def test_decode_with_beam_size_returns_the_restatements_winner(models):
    from whisper_ipa_amd.decoding import DecodingOptions, decode

    model, xa = models("micro_cached")
    res = decode(model, xa, DecodingOptions(language="en", without_timestamps=True, beam_size=5, patience=2.0, length_penalty=0.6,
                                            sample_len=BC.SAMPLE_LEN, fp16=False))
    want = BC.restated(5, 2.0, False, 0.6)
    for r, w in zip(res, want):
        assert r.tokens == w.tokens
        assert abs(r.avg_logprob - float(w.sum_logprob) / (len(w.tokens) + 1)) < 1e-3


@pytest.mark.parametrize("name,timed", [("micro_cached", False), ("micro_cached", True), ("w384_cached", False), ("w384_absorbed", True)])
def test_beam_of_one_is_the_greedy_decode_bit_for_bit(models, monkeypatch, name, timed):
    from whisper_ipa_amd.decoding import Beams, greedy_decode_tokens

    # the greedy reference reduces the written logits row, as the beam tail does: the bf16 path that merges the logits GEMM's partial
    # sums adds them up in another order
    monkeypatch.setenv("WIPA_LOGITS_FUSED", "0")
    model, xa = models(name)
    initial, always, first, _ = BC.decode_inputs(timed)
    n_init, new = len(initial), 16
    greedy = greedy_decode_tokens(model, xa, initial, always, first, SP.eot, max_new_tokens=new, rules=_gpu_rules(timed), stop_on_eot=False)
    beam = greedy_decode_tokens(model, xa, initial, always, first, SP.eot, max_new_tokens=new, rules=_gpu_rules(timed), n_group=1, beams=Beams(1),
                                stop_on_eot=False)
    for c in range(xa.shape[0]):
        body = greedy.tokens[c, n_init:].tolist()
        n = body.index(SP.eot) if SP.eot in body else len(body)
        assert int(beam.lengths[c, 0]) == n
        assert beam.tokens[c, n_init:n_init + n].tolist() == body[:n]
        assert np.float32(beam.sum_logprobs[c]) == np.float32(greedy.sum_logprobs[c]), (c, beam.sum_logprobs[c], greedy.sum_logprobs[c])


def test_a_clip_decodes_the_same_alone_and_in_a_batch(models):
    from whisper_ipa_amd.decoding import Beams, greedy_decode_tokens

    model, xa = models("w384_absorbed")
    initial, always, first, _ = BC.decode_inputs(True)
    kw = dict(max_new_tokens=16, rules=_gpu_rules(True), n_group=5, length_penalty=0.6, beams=Beams(10))
    both = greedy_decode_tokens(model, xa, initial, always, first, SP.eot, **kw)
    for c in range(xa.shape[0]):
        alone = greedy_decode_tokens(model, xa[c:c + 1], initial, always, first, SP.eot, **kw)
        n = int(alone.lengths[0, 0])
        assert n == int(both.lengths[c, 0])
        assert (alone.tokens[0, :len(initial) + n] == both.tokens[c, :len(initial) + n]).all()
        assert np.float32(alone.sum_logprobs[0]) == np.float32(both.sum_logprobs[c])


def test_the_layout_holds_the_audio_once_per_clip_and_the_beam_buffer_has_the_documented_size(models):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import _grouped

    model, _ = models("micro_cached")
    L = _lib.lib()
    pk = model.packed()
    one, five = _lib.DecLayout(), _lib.DecLayout()
    _lib.check(L.wipa_decoder_layout(C.byref(pk["cfg"]), 2, C.byref(one)))
    _lib.check(L.wipa_decoder_layout(C.byref(_grouped(pk, 5)["cfg"]), 10, C.byref(five)))
    assert five.self_kv - five.cross_kv == one.self_kv - one.cross_kv  # 10 rows, the audio of 2 clips
    B, G, maxc, ld = 10, 5, 10, five.ld_tok
    clips, cap = B // G, max(G, maxc)
    want = sum(_up256(n) for n in (B * ld, B * (G + 1) * 8, B * 4, clips * cap * ld * 4, clips * cap * 4, clips * cap * 4, clips * 4)) + 256
    assert int(L.wipa_beam_bytes(B, G, maxc, ld)) == want
    assert int(L.wipa_beam_bytes(B, 3, maxc, ld)) == 0  # rows that do not divide into groups


def test_beam_entry_points_refuse_before_anything_is_enqueued(models, monkeypatch):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import _grouped, _mask, _state_for
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    L = _lib.lib()
    model, _ = models("micro_cached")
    G, B = 2, 4
    pk = _grouped(model.packed(), G)
    m = _mask(model, [])
    with on_stream() as s:
        st = _state_for(model, B, pk)
        buf = st.beam_buffer(G, 2)

        def run(nbytes=None, maxc=2, rows=B):
            call = _lib.DecodeCall(n_init=3, eot=SP.eot, mask_first=ptr(m), mask_always=ptr(m), beam=ptr(buf),
                                   beam_bytes=buf.numel() if nbytes is None else nbytes, beam_max_candidates=maxc)
            rc = L.wipa_decoder_run_ex(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), rows, C.byref(call), 1, 0, sptr(s))
            msg = L.wipa_last_error().decode()
            assert rc == 0 or msg.startswith("wipa_decoder_run_ex: "), msg
            return rc, msg

        for kw, word in ((dict(nbytes=int(L.wipa_beam_bytes(B, G, 2, st.layout.ld_tok)) - 1), "call.beam_bytes"), (dict(maxc=0), "call.beam_max_candidates"),
                         (dict(maxc=65), "call.beam_max_candidates"),
                         (dict(rows=3), "multiple")):
            rc, msg = run(**kw)
            assert rc != 0 and word in msg, (kw, rc, msg)
        for env, val in (("WIPA_DECODE_TAIL", "0"), ("WIPA_DECODE_FUSED", "1")):
            monkeypatch.setenv(env, val)
            rc, msg = run()
            monkeypatch.delenv(env)
            assert rc != 0 and env in msg, (env, rc, msg)
        s.synchronize()


# ---------------------------------------------------------------- 7. transcribe(beam_size=)
def test_transcribe_with_beam_size_equals_the_restatements_window_loop(models):
    """the same ``transcribe`` loop over the model's beam decode and over the restatement's (tests/beam_cases.py), window by window"""
    import warnings

    import whisper_ipa_amd as wipa

    model, _ = models("micro_cached")
    want, margins = BC.restated_transcribe()
    assert len(margins) >= 3 and min(margins) > BC.required_margin()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = wipa.transcribe(model, BC.transcribe_audio(), language="en", sample_len=BC.SAMPLE_LEN, fp16=False, beam_size=BC.TRANSCRIBE_BEAMS)
    for g, w in zip(got, want):
        assert g["text"] == w["text"] and g["language"] == w["language"]
        assert [(s["seek"], s["start"], s["end"], s["tokens"]) for s in g["segments"]] == [(s["seek"], s["start"], s["end"], s["tokens"])
                                                                                            for s in w["segments"]]
        for a, b in zip(g["segments"], w["segments"]):
            assert abs(a["avg_logprob"] - b["avg_logprob"]) < DECODE_LOGPROB_TOL and a["temperature"] == 0.0
    assert len({s["seek"] for s in got[0]["segments"]}) >= 2  # the long file walked on to a second window
