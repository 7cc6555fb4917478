"""What the host refusal tests of wipa_decoder_run_ex / wipa_decoder_prefill_ex share: a small configuration, pointers that are never
dereferenced, and one function that makes the call and hands back the refusal.  No GPU: every refusal comes before anything is enqueued."""
import ctypes as C

FAKE = 0x1000  # 16-byte aligned, never dereferenced
SMALL = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=2, n_vocab=51865, n_text_ctx=448, n_text_state=384,
             n_text_head=6, n_text_layer=2, dec_cross_absorbed=1)
RULES = (50364, 50363, 50)  # timestamp_begin, no_timestamps, max_initial_timestamp_index
WIPA_ERR_ARG = -1


def small_cfg(_lib, **over):
    return _lib.ModelCfg(**{**SMALL, "dtype": _lib.WIPA_BF16, **over})


def fp8_cfg(_lib):
    return small_cfg(_lib, dec_cross_absorbed=0, dec_w_dtype=_lib.WIPA_FP8_E4M3)


def refusal(_lib, entry: str, cfg, n_steps: int = 1, B: int = 4, state_bytes: int = 1 << 40, rules: bool = False, **fields) -> str:
    """``entry`` is "run" or "prefill"; ``fields`` are wipa_decode_call's beyond n_init = 3, eot and the two masks (``rules=True``: a valid
    rules struct).  Asserts WIPA_ERR_ARG and a message that starts with the entry point's name; returns the message."""
    lib = _lib.lib()
    r = _lib.DecodeRules(*RULES)
    call = _lib.DecodeCall(**{"n_init": 3, "eot": 50257, "mask_first": FAKE, "mask_always": FAKE, "rules": C.pointer(r) if rules else None, **fields})
    args = (C.byref(cfg), (C.c_void_p * 64)(), C.c_void_p(FAKE), state_bytes, B, C.byref(call))
    rc = lib.wipa_decoder_run_ex(*args, n_steps, 0, None) if entry == "run" else lib.wipa_decoder_prefill_ex(*args, 0, None)
    msg = lib.wipa_last_error().decode()
    assert rc == WIPA_ERR_ARG, (rc, msg)
    assert msg.startswith(f"wipa_decoder_{entry}_ex: "), msg
    return msg
