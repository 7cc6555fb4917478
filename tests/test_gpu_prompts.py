"""GPU: prompt conditioning -- per-row prompts right-aligned to one prompt width (include/wipa.h: wipa_decoder_begin_ragged /
wipa_decoder_run_ex with wipa_decode_call.starts_dev; the RAGGED instantiations of decode_attn_kernel and of the step tails) against tests/prompt_ref.py, where every
row is decoded alone with its unpadded initial tokens.  Reference: mlx_whisper.transcribe's condition_on_previous_text
(scripts/evaluate_model.py:112-119 of the reference calls it with upstream's defaults).  ``pytest -m gpu`` on an MI355X.

Five rows with histories of 0, 1, 17, 70 and 223 tokens: a row without padding, a row that is all padding but three columns, window
starts inside the first key group of decode_attn_kernel and in later ones, on both sides of its 32- and 128-key strides.  On the CPU
oracle the per-row reference has a smallest top-2 margin of 0.0116 (lively, 223) and a smallest timestamp-mass gap of 0.0417 (scripted,
0) against an f32 logit error of 3e-5 .. 2.1e-4 (README), and every rule branch fires in every row: the ids can be compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import prompt_ref as PR
import timestamp_ref as TR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP = PR.MICRO, PR.W384, PR.SP
V, TB, NT, EOT, STEPS = PR.V, PR.TB, PR.NT, PR.EOT, PR.STEPS
ROWS = PR.initial_rows()
LONGEST = max(len(r) for r in ROWS)  # 227: [sot_prev] + 223 + sot_sequence


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def _rules(max_init=50):
    from whisper_ipa_amd import _lib

    return _lib.DecodeRules(TB, NT, max_init)


@pytest.fixture(scope="module")
def mels():
    return PR.clip_mels()


@pytest.fixture(scope="module")
def refs(mels):
    """the per-row CPU loop, once per weight set: (W, xa, [RowRef])"""
    out = {}
    for name, scripted in (("lively", False), ("scripted", True)):
        W = PR.weights(MICRO, 7, scripted)
        with torch.no_grad():
            xa = R.encoder_forward(W, MICRO, mels)
        rows = PR.per_row_reference(W, MICRO, xa, ROWS)
        for b, r in enumerate(rows):
            print(f"{name} row {b} ({len(r.initial)} initial tokens): min top-2 margin {r.loop.margins.min():.4f}, min mass gap "
                  f"{r.loop.mass_gaps.min():.4f}, branches {r.loop.counts}")
            # before any GPU result is compared: the reference decides every token by more than the f32 logit error can move
            assert r.loop.margins.min() > 5e-3 and r.loop.mass_gaps.min() > 5e-3, (name, b)
            assert all(n >= 1 for n in r.loop.counts.values()), (name, b, r.loop.counts)
        out[name] = (W, xa, rows)
    return out


def _feats(xa, n=len(ROWS)):
    return xa[[b % xa.shape[0] for b in range(n)]].contiguous()


def _check_against_rows(g, rows, P):
    assert g.n_init == P and g.tokens.shape == (len(rows), P + STEPS)
    for b, r in enumerate(rows):
        n = len(r.initial)
        assert g.starts[b] == P - n
        assert g.tokens[b, P - n: P].tolist() == r.initial and (g.tokens[b, : P - n] == 0).all()
        want = r.loop.tokens[0, n:]
        print(f"row {b}: sum_logprobs {g.sum_logprobs[b]:.5f} vs {r.loop.sum_logprobs[0]:.5f}")
        assert g.tokens[b, P:].tolist() == want.tolist(), (b, g.tokens[b, P:].tolist(), want.tolist())
        assert abs(g.sum_logprobs[b] - r.loop.sum_logprobs[0]) < 1e-2


# ---------------------------------------------------------------- 1. f32: the ragged batch of five against the per-row CPU loop
@pytest.mark.parametrize("weights", ["lively", "scripted"])
@pytest.mark.parametrize("use_graph,prefill", [(True, True), (False, True), (True, False), (False, False)])
def test_ragged_batch_f32_vs_per_row_cpu_loop(refs, monkeypatch, weights, use_graph, prefill):
    """The batched prompt pass (wipa_decoder_prefill_ragged) and the stepped prompt (WIPA_NO_PREFILL=1), replayed and eager.
    P = 227, unrounded (pad_to): the row with the 223-token history has no padding, the bare sot_sequence is all padding but three
    columns.  Tokens from column P on, log-prob sums (1e-2: the bound of test_decode_with_rules_f32_bit_exact_vs_cpu_loop), the first
    generated column's logits (1e-3: the project's f32 tolerance) and no_speech_prob (|dp| <= 2 p max|dlogit|: 2e-3)."""
    from whisper_ipa_amd.decoding import _no_speech_from, ragged_decode_tokens
    from whisper_ipa_amd.tokenizer import get_tokenizer

    W, xa, rows = refs[weights]
    if not prefill:
        monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    feats = _feats(xa).cuda()
    g = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, use_graph=use_graph, rules=_rules(),
                             pad_to=LONGEST, sot_back=len(PR.SOT_SEQUENCE))
    _check_against_rows(g, rows, LONGEST)
    tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    assert tok.no_speech == SP.no_speech
    nsp = _no_speech_from(g.sot_logits, tok)
    sot_err = max(float(np.abs(g.sot_logits[b].cpu().numpy() - r.sot_logits).max()) for b, r in enumerate(rows))
    print(f"no_speech_prob {nsp.tolist()} vs {[r.no_speech for r in rows]}; max |dlogit| at the sot column {sot_err:.2e}")
    assert sot_err < 1e-3
    for b, r in enumerate(rows):
        assert abs(nsp[b] - r.no_speech) < 2e-3
    one = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=1, stop_on_eot=False, use_graph=use_graph, rules=_rules(),
                               pad_to=LONGEST)
    got = one.last_logits.cpu().numpy()
    err = max(float(np.abs(got[b] - r.loop.step_logits[0][0]).max()) for b, r in enumerate(rows))
    print(f"{weights}: max |dlogit| of the first generated column {err:.2e}")
    assert err < 1e-3


# ---------------------------------------------------------------- 2. the batched prompt pass equals stepping the prompt
@pytest.mark.parametrize("dims,dtype,cross", [(MICRO, torch.float32, "cached"), (W384, torch.bfloat16, "cached"), (W384, torch.bfloat16, "absorbed")])
def test_prompt_pass_equals_stepping_the_prompt(mels, monkeypatch, dims, dtype, cross):
    """wipa_decoder_prefill_ragged + wipa_decoder_run_ex (starts_dev) against the prompt walked column by column, for the same ragged batch:
    f32: the same tokens, log-prob sums and first-column logits within 1e-3 (the bound of test_prompt_prefill_equals_stepwise_prompt:
    the pass batches B * P rows into other GEMM and attention kernels than the step's).  bf16, both cross-attention forms (the pass
    projects the absorbed form's K / V itself): the figures are printed; the logits must agree to 2^-5 of the largest logit -- bf16
    rounds to 2^-8 relative at every GEMM input and the two paths round a few dozen times apart, the residual stream is f32 in both."""
    from whisper_ipa_amd.decoding import ragged_decode_tokens

    W = PR.weights(dims, 7 if dims is MICRO else 1, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, dims, mels)
    always, first = R.suppress_lists(SP)
    m = _model(dims, W, dtype) if dtype == torch.float32 else _model_cross(dims, W, dtype, cross)
    feats = _feats(xa).cuda().to(dtype)
    kw = dict(max_new_tokens=STEPS, stop_on_eot=False, rules=_rules(), sot_back=len(PR.SOT_SEQUENCE))
    a = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, **kw)
    a1 = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=1, stop_on_eot=False, rules=_rules())
    la, sa = a1.last_logits.float().cpu().numpy().copy(), a.sot_logits.float().cpu().numpy().copy()
    monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    b = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, **kw)
    b1 = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=1, stop_on_eot=False, rules=_rules())
    lb, sb = b1.last_logits.float().cpu().numpy(), b.sot_logits.float().cpu().numpy()
    err, err_sot = float(np.abs(la - lb).max()), float(np.abs(sa - sb).max())
    same = float((a.tokens == b.tokens).mean())
    print(f"{dtype} {cross}: max |dlogit| first column {err:.2e}, sot column {err_sot:.2e}; token match {same:.3f}; "
          f"sum_logprobs {a.sum_logprobs.tolist()} vs {b.sum_logprobs.tolist()}")
    assert a.n_init == b.n_init == 240 and a.tokens.shape == b.tokens.shape
    if dtype == torch.float32:
        assert (a.tokens == b.tokens).all()
        assert np.abs(a.sum_logprobs - b.sum_logprobs).max() < 1e-3
        assert err < 1e-3 and err_sot < 1e-3
    else:
        assert np.isfinite(la).all() and np.isfinite(sa).all()
        assert err < 2.0 ** -5 * float(np.abs(lb).max()) and err_sot < 2.0 ** -5 * float(np.abs(sb).max())
        assert (a.tokens[:, :240] == b.tokens[:, :240]).all()  # the prompt columns are the caller's


def _model_cross(dims_o, W, dtype, cross):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype, cross_attention=cross)
    m.load_weights(W)
    return m


# ---------------------------------------------------------------- 3. row independence, bf16 at d = 384
def test_ragged_rows_are_independent_of_their_neighbours_bf16_d384(mels):
    """every row of the ragged batch against the same row in a batch of five copies of itself packed to the same P: tokens and log-prob
    sums bit for bit -- nothing a row computes may depend on its neighbours or on their padding.  P is the rounded width here (240)."""
    from whisper_ipa_amd.decoding import pack_prompts, ragged_decode_tokens

    W = PR.weights(W384, 1, True)
    with torch.no_grad():
        xa = R.encoder_forward(W, W384, mels)
    always, first = R.suppress_lists(SP)
    m = _model(W384, W, torch.bfloat16)
    feats = _feats(xa).cuda().to(torch.bfloat16)
    P = pack_prompts(ROWS, 448, STEPS)[2]
    assert P == 240
    g = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, rules=_rules())
    assert g.n_init == P
    for b in range(len(ROWS)):
        alone = ragged_decode_tokens(m, feats[b: b + 1].expand(5, -1, -1).contiguous(), [ROWS[b]] * 5, always, first, EOT, max_new_tokens=STEPS,
                                     stop_on_eot=False, rules=_rules(), pad_to=P)
        for c in range(5):
            assert (alone.tokens[c] == g.tokens[b]).all(), (b, c, alone.tokens[c, P:].tolist(), g.tokens[b, P:].tolist())
            assert alone.sum_logprobs[c] == g.sum_logprobs[b], (b, c)
    # the bf16 path differs from the f32 loop by its logit error only: report how far the free run followed it
    cpu = PR.per_row_reference(W, W384, xa, ROWS)
    same = np.mean([(g.tokens[b, P:] == r.loop.tokens[0, len(r.initial):]).mean() for b, r in enumerate(cpu)])
    print(f"token match with the f32 per-row loop: {same:.3f}")


# ---------------------------------------------------------------- 4. sampling: the counter uses the row's own position
def test_ragged_sampling_draws_at_the_rows_own_position(refs):
    from whisper_ipa_amd.decoding import Sampling, ragged_decode_tokens

    W, xa, _ = refs["lively"]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    feats = _feats(xa).cuda()
    streams = [(b, 0) for b in range(len(ROWS))]
    g = ragged_decode_tokens(m, feats, ROWS, always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, rules=_rules(),
                             sample=Sampling(1, 0.6, streams))
    P = g.n_init
    for b in (1, 3):
        alone = ragged_decode_tokens(m, feats[b: b + 1], [ROWS[b]], always, first, EOT, max_new_tokens=STEPS, stop_on_eot=False, rules=_rules(),
                                     sample=Sampling(1, 0.6, [streams[b]]))
        assert alone.n_init != P  # another prompt width: the draw must not follow the column
        assert alone.tokens[0, alone.n_init:].tolist() == g.tokens[b, P:].tolist()
        # the ids are the claim; the batched prompt pass picks its GEMM kernels by B * P, so the sums agree to f32 rounding, not in bits
        assert abs(alone.sum_logprobs[0] - g.sum_logprobs[b]) < 1e-3
        ref = PR.sample_row_loop(W, MICRO, xa[b % 2: b % 2 + 1], ROWS[b], STEPS, 1, 0.6, streams[b])
        print(f"row {b}: min key margin of the restatement {ref.key_margins.min():.4f}; ids {g.tokens[b, P:].tolist()}")
        assert ref.key_margins.min() > 5e-3  # 1 / T times the f32 logit error is far below
        assert g.tokens[b, P:].tolist() == ref.tokens[len(ROWS[b]):].tolist()
        assert abs(g.sum_logprobs[b] - ref.sum_logprob) < 1e-2
    assert g.tokens[1, P:].tolist() != g.tokens[3, P:].tolist()


# ---------------------------------------------------------------- 5. starts of zero and rows without prompts
@pytest.mark.parametrize("with_rules", [True, False])
def test_zero_starts_reproduce_the_plain_entry_points(refs, monkeypatch, with_rules):
    """wipa_decoder_begin_ragged with every start 0 and P = 3, then the ragged entry points.  Stepping (wipa_decoder_run_ex with starts_dev against
    wipa_decoder_begin and the call without it, both with WIPA_NO_PREFILL=1) runs the RAGGED instantiations of the same kernels on the same
    numbers: tokens and log-prob sums bit for bit.  The batched passes are different kernels by design (wipa_decoder_prefill_ragged is
    the teacher-forced body, wipa_decoder_prefill the four-row one), so there the comparison is the one the project makes between
    wipa_decoder_prefill and stepping: the same tokens, sums within 1e-3."""
    from whisper_ipa_amd.decoding import greedy_decode_tokens, ragged_decode_tokens

    W, xa, _ = refs["lively"]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    feats = xa.cuda()
    kw = dict(max_new_tokens=STEPS, stop_on_eot=False, rules=_rules() if with_rules else None)
    want = greedy_decode_tokens(m, feats, PR.SOT_SEQUENCE, always, first, EOT, **kw)
    got = ragged_decode_tokens(m, feats, [PR.SOT_SEQUENCE] * 2, always, first, EOT, pad_to=3, **kw)
    assert (got.starts == 0).all() and got.n_init == 3
    print(f"batched passes: sum_logprobs {got.sum_logprobs.tolist()} vs {want.sum_logprobs.tolist()}")
    assert (got.tokens == want.tokens).all()
    assert np.abs(got.sum_logprobs - want.sum_logprobs).max() < 1e-3
    monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    want = greedy_decode_tokens(m, feats, PR.SOT_SEQUENCE, always, first, EOT, **kw)
    got = ragged_decode_tokens(m, feats, [PR.SOT_SEQUENCE] * 2, always, first, EOT, pad_to=3, **kw)
    assert (got.tokens == want.tokens).all()
    assert (got.sum_logprobs == want.sum_logprobs).all(), (got.sum_logprobs.tolist(), want.sum_logprobs.tolist())


def _call_fields(k):
    """a DecodeCall as plain values: integers as they are, pointers as addresses (None: NULL), the rules as their three numbers"""
    out = {}
    for name, _ in k._fields_:
        v = getattr(k, name)
        out[name] = v if v is None or type(v) is int else ((v.contents.timestamp_begin, v.contents.no_timestamps, v.contents.max_initial_timestamp_index) if v else None)
    return out


class _Spy:
    """libwipa behind a recorder: every call of an entry point is recorded by name (``calls``) and with every plain-int argument
    (``records``: (name, ints) -- sizes, batch, prompt width, eot, step count, use_graph, and the addresses ``ptr()`` hands over); a
    wipa_decoder_run_ex / wipa_decoder_prefill_ex call also with the fields of its wipa_decode_call (``fields``, and in ``records``)"""

    def __init__(self, real):
        self._real, self.calls, self.records, self.run_steps, self.fields = real, [], [], [], []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*a):
            self.calls.append(name)
            ints = tuple(v for v in a if type(v) is int)
            if name in ("wipa_decoder_run_ex", "wipa_decoder_prefill_ex"):
                k = _call_fields(a[5]._obj)  # the DecodeCall behind C.byref
                self.fields.append((name, k))
                ints += tuple(sorted(k.items()))
            self.records.append((name, ints))
            if name.startswith("wipa_decoder_run"):
                self.run_steps.append(a[6] if name == "wipa_decoder_run_ex" else a[9])  # n_steps
            return fn(*a)

        return counted


def test_decode_without_prompts_makes_the_calls_it_made(refs, monkeypatch):
    """decode() with prompts=[None] * B: exactly the library calls of decode() without the option, in the same order, and the same result"""
    import whisper_ipa_amd as wipa
    from whisper_ipa_amd import _lib

    W, xa, _ = refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    feats = xa.cuda()
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, fp16=False, sample_len=STEPS)
    wipa.decode(m, feats, opts)  # warm: the masks, the state blob and the graphs exist
    real = _lib.lib()
    spy_a, spy_b = _Spy(real), _Spy(real)
    monkeypatch.setattr(_lib, "_lib", spy_a)
    a = wipa.decode(m, feats, opts)
    monkeypatch.setattr(_lib, "_lib", spy_b)
    b = wipa.decode(m, feats, opts, prompts=[None, None])
    monkeypatch.setattr(_lib, "_lib", real)
    assert spy_a.calls == spy_b.calls and not any("ragged" in c for c in spy_b.calls), (spy_a.calls, spy_b.calls)
    assert spy_b.fields and all(k["starts_dev"] is None for _, k in spy_b.fields), spy_b.fields  # no row has a start of its own
    assert any(k["rules"] is not None for _, k in spy_b.fields)  # the decode itself runs under the timestamp rules
    assert spy_a.records == spy_b.records, (spy_a.records, spy_b.records)  # ... with the same integer arguments, step counts included
    assert [r.tokens for r in a] == [r.tokens for r in b]
    # and a prompt takes the ragged entry points
    spy_c = _Spy(real)
    monkeypatch.setattr(_lib, "_lib", spy_c)
    c = wipa.decode(m, feats, opts, prompts=[None, PR.histories()[2]])
    monkeypatch.setattr(_lib, "_lib", real)
    runs = [k for name, k in spy_c.fields if name == "wipa_decoder_run_ex"]
    assert "wipa_decoder_begin_ragged" in spy_c.calls and runs and all(k["starts_dev"] is not None for k in runs) and "wipa_decoder_begin" not in spy_c.calls
    assert "wipa_decoder_prefill_ex" not in spy_c.calls and "wipa_decoder_prefill_ragged" in spy_c.calls
    assert all(np.isfinite(r.no_speech_prob) for r in c)


@pytest.mark.parametrize("prefill", [True, False])
def test_decode_loop_step_schedule(refs, monkeypatch, prefill):
    """The n_steps of every wipa_decoder_run* call of one decode, for both public loops: eot = -1 (no row ever ends), 12 new tokens,
    the default check_every of 8, no rules.  With the batched prompt pass exactly one prefill call precedes the run calls; with
    WIPA_NO_PREFILL=1 there is none and the prompt walk (P - 1 steps) rides with the first generated columns -- after the steps up to
    the <|startoftranscript|> column when ``sot_back`` asks for that column's logits."""
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import greedy_decode_tokens, ragged_decode_tokens

    W, xa, _ = refs["lively"]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    feats = xa.cuda()
    if not prefill:
        monkeypatch.setenv("WIPA_NO_PREFILL", "1")
    rows = [list(ROWS[1][-5:]), list(PR.SOT_SEQUENCE)]
    assert [len(r) for r in rows] == [5, 3] and len(PR.SOT_SEQUENCE) == 3
    kw = dict(max_new_tokens=12)
    cases = [("wipa_decoder_prefill_ex", lambda: greedy_decode_tokens(m, feats, PR.SOT_SEQUENCE, always, first, -1, **kw), [8, 3], [10, 4]),
             ("wipa_decoder_prefill_ragged", lambda: ragged_decode_tokens(m, feats, rows, always, first, -1, pad_to=6, **kw), [8, 3], [13, 4]),
             ("wipa_decoder_prefill_ragged", lambda: ragged_decode_tokens(m, feats, rows, always, first, -1, pad_to=6, sot_back=3, **kw),
              [8, 3], [4, 9, 4])]
    real = _lib.lib()
    for prefill_name, run, with_pass, stepped in cases:
        spy = _Spy(real)
        monkeypatch.setattr(_lib, "_lib", spy)
        g = run()
        monkeypatch.setattr(_lib, "_lib", real)
        assert g.n_steps == 12
        print(prefill_name, spy.run_steps)
        assert spy.run_steps == (with_pass if prefill else stepped), (prefill_name, spy.run_steps)
        passes = [c for c in spy.calls if c.startswith("wipa_decoder_prefill")]
        assert passes == ([prefill_name] if prefill else []), passes
        if prefill:
            assert spy.calls.index(prefill_name) < min(i for i, c in enumerate(spy.calls) if c.startswith("wipa_decoder_run"))
        ragged = prefill_name == "wipa_decoder_prefill_ragged"  # the run calls of the ragged loop carry the rows' starts, the others none
        assert all((k["starts_dev"] is not None) == ragged and k["n_init"] == (6 if ragged else 3) for name, k in spy.fields if name == "wipa_decoder_run_ex")


# ---------------------------------------------------------------- 6. refusals that need a live state
def test_prompt_pass_refuses_a_small_workspace_and_bad_columns(refs):
    from whisper_ipa_amd import _lib
    from whisper_ipa_amd.decoding import _mask, _packed_for, _state_for
    from whisper_ipa_amd.runtime import on_stream, ptr, sptr

    W, xa, _ = refs["lively"]
    always, first = R.suppress_lists(SP)
    m = _model(MICRO, W, torch.float32)
    L = _lib.lib()
    B, P = 2, 16
    pk = _packed_for(m, B, STEPS)
    st = _state_for(m, B, pk)
    m_always, m_first = _mask(m, always), _mask(m, list(always) + list(first))
    need = int(L.wipa_decoder_prompt_workspace_bytes(C.byref(pk["cfg"]), B, P))
    assert need > 0 and int(L.wipa_decoder_prompt_workspace_bytes(C.byref(pk["cfg"]), B, 2 * P)) > need
    with on_stream() as s:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")

        def call(P=P, sot_col=-1, starts=st.starts, nbytes=need):
            return L.wipa_decoder_prefill_ragged(C.byref(pk["cfg"]), pk["dec_tab"], ptr(st.blob), st.blob.numel(), B, P, sot_col, EOT, ptr(m_first),
                                                 ptr(m_always), 0, None, None, ptr(starts) if starts is not None else None, ptr(ws), nbytes, sptr(s))

        assert call(nbytes=need - 1) != 0 and b"workspace too small" in L.wipa_last_error()
        assert call(sot_col=P) != 0 and b"sot_col" in L.wipa_last_error()
        assert call(P=448) != 0 and b"P=448" in L.wipa_last_error()
        assert call(starts=None) != 0 and b"starts_dev" in L.wipa_last_error()


# ---------------------------------------------------------------- 7. transcribe() with conditioning, through the model
def test_transcribe_conditions_on_previous_text_like_the_host_loop(refs):
    """whisper_ipa_amd.transcribe on a 70 s and a 40 s clip with condition_on_previous_text=True and an initial prompt: the segments
    are those of a host loop that calls decode(prompts=...) window by window with upstream's bookkeeping, and they differ from the
    unconditioned result in at least one window (otherwise this shows nothing)."""
    import warnings

    import whisper_ipa_amd as wipa
    from whisper_ipa_amd.tokenizer import get_tokenizer
    from whisper_ipa_amd.transcribe import split_segments

    W, _, _ = refs["scripted"]
    m = _model(MICRO, W, torch.float32)
    clips = [np.concatenate([R.synthetic_clip(0, 30.0), R.synthetic_clip(2, 30.0), R.synthetic_clip(1, 10.0)[: 10 * 16000]]),
             np.concatenate([R.synthetic_clip(1, 30.0), R.synthetic_clip(0, 10.0)[: 10 * 16000]])]
    assert [len(c) for c in clips] == [70 * 16000, 40 * 16000]
    prompt = "previously on this channel"
    kw = dict(language="en", sample_len=STEPS, fp16=False, no_speech_threshold=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the random-init model's average log-probability is below upstream's fallback threshold
        got = wipa.transcribe(m, clips, condition_on_previous_text=True, initial_prompt=prompt, **kw)
        plain = wipa.transcribe(m, clips, **kw)
    tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
    opts = wipa.DecodingOptions(language="en", without_timestamps=False, sample_len=STEPS, fp16=False)
    for i, clip in enumerate(clips):  # upstream's loop, one file at a time
        all_tokens, since, seek, frames, want = list(tok.encode(" " + prompt)), 0, 0, len(clip) // 160, []
        while seek < frames:
            size = min(3000, frames - seek)
            win = np.zeros((1, 480000), dtype=np.float32)
            win[0, : size * 160] = clip[seek * 160: (seek + size) * 160]
            mel = wipa.log_mel_spectrogram(torch.from_numpy(win).cuda(), n_mels=80)
            res = wipa.decode(m, mel, opts, prompts=[all_tokens[since:]])[0]
            segs, adv = split_segments(res.tokens, TB, seek * 160 / 16000, size)
            for sg in segs:
                text = tok.decode([t for t in sg["tokens"] if t < tok.eot])
                toks = [] if (sg["start"] == sg["end"] or text.strip() == "") else sg["tokens"]
                want.append((seek, sg["start"], sg["end"], toks))
                all_tokens.extend(toks)
            if res.temperature > 0.5:
                since = len(all_tokens)
            seek += adv if adv > 0 else adv + size
        have = [(s["seek"], s["start"], s["end"], s["tokens"]) for s in got[i]["segments"]]
        assert have == want, (i, have, want)
        assert len({s["seek"] for s in got[i]["segments"]}) >= 2
    differ = sum(a["tokens"] != b["tokens"] for i in range(2) for a, b in zip(got[i]["segments"], plain[i]["segments"]))
    differ += sum(len(got[i]["segments"]) != len(plain[i]["segments"]) for i in range(2))
    print(f"segments that differ from the unconditioned transcript: {differ}")
    assert differ >= 1
