"""GPU: continuous-batching decode (whisper_ipa_amd.continuous.decode_continuous; include/wipa.h: wipa_decoder_admit_rows /
wipa_decoder_shift_columns / wipa_decode_call.continuous and the CONTINUOUS step tails) against the CPU oracle's loop with every clip
decoded ALONE, batch of one, to its own length -- slots, refill, admission columns and shifts do not exist there.  ``pytest -m gpu`` on
an MI355X.

MICRO dims, f32 (the cached cross-attention form: an admission projects the clip's K / V into its slot), eight clips whose features are
eight different mixes of the two fixture clips of tests/prompt_ref.py, so a clip decoded with another slot's audio gets other ids.
Lengths 5, 27, 12, 19, 1, 22, 23, 26 through 3 slots with a check every 4 steps: 64 steps, clips finish out of order, and with
column_limit = 40 the columns move down twice, by 20 and by 12 (tests/test_continuous_host.py derives both on the fake stepper; the
shorter list 5, 17, 2, 9, 1, 12, 3, 6 ends after 32 steps and never reaches column 40).  On the CPU oracle the smallest top-2 margin over
all compared steps is 0.0075 (clip 1) against an f32 logit error of 3e-5 .. 2.1e-4 (README): the ids can be compared exactly.

bf16 at d = 384 (the absorbed form: an admission copies the clip's encoder output): the "peaky" preset.  Its smallest top-2 margin on the
CPU oracle over the compared steps (6 clips, up to 14 steps) is 45.7, against the bf16 logit error of 0.1 - 0.2 the README quotes."""
import pytest
import torch

import prompt_ref as PR
from oracle import whisper_ref as R

pytestmark = pytest.mark.gpu

MICRO, W384, SP, EOT = PR.MICRO, PR.W384, PR.SP, PR.EOT
LENS = [5, 27, 12, 19, 1, 22, 23, 26]
INIT = list(SP.sot_sequence_including_notimestamps(0))
LENS_BF16 = [3, 14, 1, 9, 6, 11]


def _model(dims_o, W, dtype):
    from whisper_ipa_amd.whisper import ModelDimensions, Whisper

    m = Whisper(ModelDimensions(**dims_o.__dict__), dtype=dtype)
    m.load_weights(W)
    return m


def mixed_features(xa: torch.Tensor, n: int) -> torch.Tensor:
    """n different feature tensors from the two fixture clips: clip i is (1 - i / (n - 1)) xa[0] + i / (n - 1) xa[1]"""
    w = torch.linspace(0.0, 1.0, n)[:, None, None]
    return ((1 - w) * xa[0:1] + w * xa[1:2]).contiguous()


def _cut(row):
    row = [int(t) for t in row]
    return row[: row.index(EOT)] if EOT in row else row


def cpu_rows(W, dims, feats, lens):
    """every clip alone through the oracle's greedy loop, to its own length: (generated ids before EOT, sum_logprobs, min margin)"""
    always, first = R.suppress_lists(SP)
    out = []
    with torch.no_grad():
        for i, n in enumerate(lens):
            g = R.greedy_decode(W, dims, feats[i: i + 1], INIT, always, first, EOT, sample_len=n, stop_on_eot=True)
            out.append((_cut(g.tokens[0, len(INIT):]), float(g.sum_logprobs[0]), float(g.margins.min())))
    return out


@pytest.fixture(scope="module")
def ref():
    """(W, features [8, 1500, 128], the per-clip CPU loop), computed once"""
    W = PR.weights(MICRO, 7, False)
    with torch.no_grad():
        xa = R.encoder_forward(W, MICRO, PR.clip_mels())
    feats = mixed_features(xa, len(LENS))
    rows = cpu_rows(W, MICRO, feats, LENS)
    for i, (ids, slp, margin) in enumerate(rows):
        print(f"clip {i}: {len(ids)} ids, sum_logprobs {slp:.5f}, min top-2 margin {margin:.4f}")
        # before any GPU result is compared: the reference decides every token by more than the f32 logit error can move
        assert margin > 5e-3, (i, margin)
    assert len({tuple(r[0][:1]) for r in rows}) > 1  # the mixes do decode differently
    return W, feats, rows


def _options(**kw):
    from whisper_ipa_amd.decoding import DecodingOptions

    return DecodingOptions(language="en", without_timestamps=True, fp16=False, **kw)


def _sum(r):
    return r.avg_logprob * (len(r.tokens) + 1)


@pytest.fixture(scope="module")
def runs(ref):
    """the continuous decodes the f32 tests share: 3 slots, 3 slots with column_limit = 40, 8 slots (no refill)"""
    from whisper_ipa_amd.continuous import decode_continuous

    W, feats, _ = ref
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    out = {}
    for name, kw in (("slots3", dict(slots=3)), ("shifted", dict(slots=3, column_limit=40)), ("slots8", dict(slots=8))):
        stats = []
        res = decode_continuous(m, dev, _options(), sample_lens=LENS, check_every=4, stats_out=stats, **kw)
        out[name] = (res, stats[0])
    return m, dev, out


def test_f32_refill_equals_the_per_clip_cpu_loop(ref, runs):
    """8 clips, slots = 3, check_every = 4: every clip's ids equal the CPU loop's exactly; sum_logprobs within the 1e-2 of
    tests/test_gpu_prompts.py against that loop"""
    _, _, rows = ref
    res, stats = runs[2]["slots3"]
    assert len(res) == len(LENS) and stats.shifts == []
    assert [clip for _, clip, _ in stats.admissions] == list(range(8)) and stats.retired != sorted(stats.retired)
    for i, (r, (ids, slp, _)) in enumerate(zip(res, rows)):
        print(f"clip {i}: sum_logprobs {_sum(r):.5f} vs {slp:.5f}; ids {r.tokens}")
        assert r.tokens == ids, (i, r.tokens, ids)
        assert abs(_sum(r) - slp) < 1e-2


def test_forced_shifts_change_nothing(runs):
    """column_limit = 40 forces two shifts; ids are those of the run without shifts, and so are the log-probability sums, bit for bit:
    decode_attn_kernel<.., RAGGED> walks a row's keys from its own start in the lane / wave partition it would use at column 0, the
    position row and the draw's counter are relative to the start, so no reduction order depends on the absolute column"""
    plain, _ = runs[2]["slots3"]
    shifted, stats = runs[2]["shifted"]
    assert stats.shifts == [20, 12]
    for i, (a, b) in enumerate(zip(plain, shifted)):
        assert a.tokens == b.tokens, (i, a.tokens, b.tokens)
        assert a.avg_logprob == b.avg_logprob, (i, a.avg_logprob, b.avg_logprob)


def test_ids_do_not_depend_on_the_slot_count(runs):
    """slots = 3 against slots = 8, where nothing is refilled: identical ids for every clip"""
    few, _ = runs[2]["slots3"]
    many, stats = runs[2]["slots8"]
    assert all(col == 0 for _, _, col in stats.admissions)
    for i, (a, b) in enumerate(zip(few, many)):
        assert a.tokens == b.tokens, (i, a.tokens, b.tokens)


def test_sampling_draws_from_the_clips_own_stream_at_its_own_position(ref, runs):
    """temperature 0.6, seed 1, slots = 3: every clip gets the ids of ragged_decode_tokens run on that clip alone with stream
    (clip, 0) -- the claim of test_ragged_sampling_draws_at_the_rows_own_position, for slots and admission columns"""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import Sampling, ragged_decode_tokens

    W, feats, _ = ref
    m, dev, _ = runs
    always, first = R.suppress_lists(SP)
    res = decode_continuous(m, dev, _options(temperature=0.6, seed=1), slots=3, sample_lens=LENS, check_every=4)
    for i, n in enumerate(LENS):
        alone = ragged_decode_tokens(m, dev[i: i + 1], [INIT], always, first, EOT, max_new_tokens=n, stop_on_eot=False,
                                     sample=Sampling(1, 0.6, [(i, 0)]))
        want = _cut(alone.tokens[0, alone.n_init:])
        assert res[i].tokens == want, (i, res[i].tokens, want)
    for i in range(len(LENS)):  # the restatement on the CPU: the draws are decided by more than the f32 logit error can move
        loop = PR.sample_row_loop(W, MICRO, feats[i: i + 1], INIT, LENS[i], 1, 0.6, (i, 0), with_rules=False)
        print(f"clip {i}: min key margin of the restatement {loop.key_margins.min():.4f}")
        assert loop.key_margins.min() > 5e-3
        assert res[i].tokens == _cut(loop.tokens[len(INIT):])
        assert abs(_sum(res[i]) - loop.sum_logprob) < 1e-2
    greedy, _ = runs[2]["slots3"]
    assert any(a.tokens != b.tokens for a, b in zip(res, greedy))


def test_bf16_d384_peaky_ids_equal_lockstep_decode():
    """W384, bf16, the absorbed cross-attention form, 6 clips through 2 slots: the ids equal lockstep ``decode`` of the same clips.
    The "peaky" preset's smallest top-2 margin on the CPU oracle over the compared steps is 45.7 (asserted > 5 below, before anything
    is compared) against a bf16 logit error of 0.1 - 0.2 (README)."""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import decode

    W = R.synthetic_weights(W384, seed=1, preset="peaky")
    with torch.no_grad():
        xa = R.encoder_forward(W, W384, PR.clip_mels())
    feats = mixed_features(xa, len(LENS_BF16))
    rows = cpu_rows(W, W384, feats, LENS_BF16)
    margin = min(r[2] for r in rows)
    print(f"peaky preset, d = 384: min top-2 margin of the CPU loop {margin:.2f}")
    assert margin > 5.0
    m = _model(W384, W, torch.bfloat16)
    assert m.use_absorbed()
    dev = feats.cuda().to(torch.bfloat16)
    stats = []
    res = decode_continuous(m, dev, _options(), slots=2, sample_lens=LENS_BF16, check_every=4, stats_out=stats)
    lock = decode(m, dev, _options(sample_len=max(LENS_BF16)))
    assert len(stats[0].admissions) == 6 and stats[0].admissions[2][2] > 0
    for i, n in enumerate(LENS_BF16):
        want = _cut(lock[i].tokens[:n])
        assert res[i].tokens == want, (i, res[i].tokens, want)
        assert res[i].tokens == rows[i][0]  # and both equal the f32 loop, as the margin promises


def test_language_none_is_detected_per_encoded_chunk(ref):
    """language=None: five clips through 2 slots, so three encoded chunks each run detect_language(with_no_speech=True) while the state
    is live.  Languages equal lockstep decode's and the oracle's, ids equal the CPU loop's with the detected language token in the
    prompt (its margins are checked first), no_speech_prob is filled."""
    from whisper_ipa_amd.continuous import decode_continuous
    from whisper_ipa_amd.decoding import DecodingOptions, decode
    from whisper_ipa_amd.tokenizer import LANGUAGES

    W, feats, _ = ref
    lens = [6, 3, 6, 2, 5]
    feats = feats[: len(lens)]
    always, first = R.suppress_lists(SP)
    with torch.no_grad():
        lang = R.detect_language(W, MICRO, feats, SP)
        want = []
        for i, n in enumerate(lens):
            init = list(INIT)
            init[1] = int(lang[i])
            g = R.greedy_decode(W, MICRO, feats[i: i + 1], init, always, first, EOT, sample_len=n, stop_on_eot=True)
            assert g.margins.min() > 5e-3, (i, g.margins.min())
            want.append(_cut(g.tokens[0, len(INIT):]))
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    opts = DecodingOptions(language=None, without_timestamps=True, fp16=False)
    res = decode_continuous(m, dev, opts, slots=2, sample_lens=lens, check_every=4)
    lock = decode(m, dev, opts, sample_len=max(lens))
    for i, r in enumerate(res):
        assert r.language == lock[i].language == LANGUAGES[int(lang[i]) - SP.sot - 1]
        assert r.tokens == want[i], (i, r.tokens, want[i])
        assert 0.0 <= r.no_speech_prob <= 1.0 and abs(sum(r.language_probs.values()) - 1.0) < 1e-3


def _kv(st, dims, B):
    """the bits of the state's self-attention K and V (f32) as int32 [layer, 2, B, n_ctx, d]: a view of the blob.  Bits, because the
    row at the position itself is not written yet and may hold anything"""
    n = dims.n_text_layer * 3 * B * dims.n_text_ctx * dims.n_text_state
    return st.blob[st.layout.self_kv: st.layout.self_kv + 4 * n].view(torch.int32).view(dims.n_text_layer, 3, B, dims.n_text_ctx,
                                                                                     dims.n_text_state)[:, 1:]


def test_admit_shift_and_idle_rows_through_the_c_abi(ref):
    """DeviceStepper drives the three entry points directly, 3 slots: clip 1 in slot 0 at column 0, five steps, clip 3 in slot 1 at column
    5, six steps.  Slot 2 is given a start in the future (column 30) and a sentinel sum: steps below its start leave its tokens and
    its sum_logprobs alone.  Then wipa_decoder_shift_columns(5): tokens, K and V of the live row (slot 1) are the pre-shift columns
    moved down by 5, bit for bit, in every layer; the position and the starts drop by 5, the row that started below the shift ends
    with start 0 and limit 0; and the live row decodes on to the CPU loop's ids."""
    from whisper_ipa_amd.continuous import DeviceStepper
    from whisper_ipa_amd.runtime import on_stream

    W, feats, rows = ref
    m = _model(MICRO, W, torch.float32)
    dev = feats.cuda()
    always, first = R.suppress_lists(SP)
    B, n_init = 3, len(INIT)
    with on_stream() as s:
        st = DeviceStepper(m, B, lambda clip: dev[clip], lambda clip: INIT, n_init, LENS, EOT, always, first, None, s)
        st.admit([(0, 1)])
        st.starts[2], st.starts[B + 2] = 30, 5
        st.st.sum_logprobs[2] = 1.25
        st.st.tokens[2, :40] = 77
        st.run(5)
        st.admit([(1, 3)])
        st.run(6)
        assert st.pos == 11
        assert st.st.pos.cpu().item() == 11
        assert st.starts.cpu().tolist() == [0, 5, 30, LENS[1], LENS[3], 5]
        assert st.st.sum_logprobs[2].item() == 1.25 and (st.st.tokens[2, :40] == 77).all()
        tok_before = st.st.tokens[:, :12].clone()
        kv_before = _kv(st.st, MICRO, B)[:, :, :, :12].clone()
        slp_before = st.st.sum_logprobs.clone()
        assert tok_before[1, 5:9].tolist() == INIT and tok_before[1, 9:12].tolist() == rows[3][0][:3]
        st.shift(5)
        assert st.pos == 6 and st.st.pos.cpu().item() == 6
        assert st.starts.cpu().tolist() == [0, 0, 25, 0, LENS[3], 5]
        assert torch.equal(st.st.tokens[:, :7], tok_before[:, 5:12])
        assert torch.equal(_kv(st.st, MICRO, B)[:, :, :, :7], kv_before[:, :, :, 5:12])
        assert torch.equal(st.st.sum_logprobs, slp_before)
        st.run(20)  # clip 3 has 19 tokens to generate from column 4 on; slot 2 starts at column 25 and picks its first token at 29
        got = st.st.tokens[1, 4: 4 + LENS[3]].cpu().tolist()
        assert _cut(got) == rows[3][0], (got, rows[3][0])
        assert abs(st.st.sum_logprobs[1].item() - rows[3][1]) < 1e-2
        assert st.st.sum_logprobs[2].item() == 1.25  # position 26: still below start + n_init
        assert st.st.tokens[0, 7: 27].cpu().tolist() == [EOT] * 20  # the row that left the window takes eot at every new column
