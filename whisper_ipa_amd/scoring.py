"""Batched PER / PFER edit distances on the GPU (csrc/score.hip behind ``wipa_edit_distance_batch``): the dynamic programs of the
reference's ``phone_error_rate`` and ``PFERCalculator.phone_feature_error_rate`` (scripts/evaluate_ipa.py:80-105, :139-213) for a
whole batch of (reference, hypothesis) phone sequences in one launch.

The host keeps the string work: the caller tokenises, and this module builds a per-call phone vocabulary, looks every DISTINCT
phone's 24 articulatory features up once, and packs ids, offsets and the launch order into one buffer for one host-to-device
copy.  The device computes every DP cell, in integers: ``per_dist`` is the Levenshtein distance, ``pfer24`` the feature-weighted
distance times 24 (insertion = deletion = 24, substitution = the number of features that differ), so

    PER  = per_dist / len(reference) * 100          PFER = pfer24 / 24 / len(reference) * 100

Sequences longer than ``MAX_LEN`` phones stay off the device: their pairs come back as -1 and are the caller's to score.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .runtime import device, on_stream, sptr

NUM_FEATURES = 24
MAX_LEN = _lib.SCORE_MAX_LEN  # phones per sequence the kernel takes (WIPA_SCORE_MAX_LEN)
_BITS = {0: 0, 1: 1, -1: 2}   # two bits per feature: any two different values differ in at least one bit
_VALUES = {0: 0, 1: 1, 2: -1}


def encode_features(vec) -> int:
    """24 feature values in {-1, 0, +1} -> the 48-bit code the kernel compares (feature f in bits 2f, 2f + 1).  Anything else --
    another length, a value such as 2 or 0.5 -- is a ``ValueError``: the integer PFER would not be the reference's."""
    vals = np.asarray(vec).reshape(-1).tolist()
    if len(vals) != NUM_FEATURES:
        raise ValueError(f"a phone has {NUM_FEATURES} features, got {len(vals)}")
    code = 0
    for f, v in enumerate(vals):
        if v not in (-1, 0, 1):
            raise ValueError(f"feature {f} is {v!r}: only -1, 0 and +1 can be encoded")
        code |= _BITS[int(v)] << (2 * f)
    return code


def decode_features(code: int) -> List[int]:
    """the inverse of ``encode_features``"""
    if not 0 <= code < 1 << (2 * NUM_FEATURES) or any((code >> (2 * f)) & 3 == 3 for f in range(NUM_FEATURES)):
        raise ValueError(f"{code:#x} is not a feature code")
    return [_VALUES[(code >> (2 * f)) & 3] for f in range(NUM_FEATURES)]


class ScorePack:
    """The pairs of one call packed for ONE host-to-device copy.  ``buffer`` (uint8, pinned when a GPU is present) holds, as int32,
    ``ref_off`` [P + 1], ``hyp_off`` [P + 1], ``order`` [P], ``ref_ids``, ``hyp_ids`` and then, 8-byte aligned, ``codes`` uint64
    [n_phones] (all zero without features); those attributes are views into it and ``offsets`` their byte positions.  ``kept`` lists
    the positions (in the caller's lists) of the P pairs packed; the others have a side longer than ``MAX_LEN``.  ``vocab`` is the
    per-call phone vocabulary in order of first appearance.  Host only: no GPU work happens here."""

    def __init__(self, ref_phones: Sequence[Sequence[str]], hyp_phones: Sequence[Sequence[str]],
                 features: Optional[Callable[[str], Sequence[int]]] = None, pin: Optional[bool] = None):
        if len(ref_phones) != len(hyp_phones):
            raise ValueError(f"{len(ref_phones)} references against {len(hyp_phones)} hypotheses")
        self.n_total = len(ref_phones)
        self.kept = np.array([k for k, (r, h) in enumerate(zip(ref_phones, hyp_phones)) if len(r) <= MAX_LEN and len(h) <= MAX_LEN],
                             dtype=np.int64)
        self.P = P = len(self.kept)
        self.has_features = features is not None
        ids = {}
        self.vocab: List[str] = []
        flat = ([], [])
        lens = (np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64))
        for slot, k in enumerate(self.kept):
            for side, seq in enumerate((ref_phones[k], hyp_phones[k])):
                lens[side][slot] = len(seq)
                for phone in seq:
                    i = ids.get(phone)
                    if i is None:
                        i = ids[phone] = len(self.vocab)
                        self.vocab.append(phone)
                    flat[side].append(i)
        self.n_phones = max(1, len(self.vocab))
        codes = [encode_features(features(phone)) for phone in self.vocab] if features is not None else []  # once per distinct phone

        R, H = len(flat[0]), len(flat[1])
        words = 3 * P + 2 + R + H
        o_codes = -(-4 * words // 8) * 8
        self.nbytes = o_codes + 8 * self.n_phones
        pin = torch.cuda.is_available() if pin is None else pin
        self.buffer = torch.zeros(self.nbytes, dtype=torch.uint8, pin_memory=bool(pin))
        raw = self.buffer.numpy()
        self.offsets = {}

        def view(name, first_word, count):
            self.offsets[name] = 4 * first_word
            return raw[4 * first_word: 4 * (first_word + count)].view(np.int32)

        self.ref_off, self.hyp_off = view("ref_off", 0, P + 1), view("hyp_off", P + 1, P + 1)
        self.order = view("order", 2 * P + 2, P)
        self.ref_ids, self.hyp_ids = view("ref_ids", 3 * P + 2, R), view("hyp_ids", 3 * P + 2 + R, H)
        self.offsets["codes"] = o_codes
        self.codes = raw[o_codes:].view(np.uint64)
        self.ref_off[1:], self.hyp_off[1:] = np.cumsum(lens[0]), np.cumsum(lens[1])
        self.order[:] = np.argsort(-(lens[0] * lens[1]), kind="stable")  # m n descending: the long pairs start first
        self.ref_ids[:], self.hyp_ids[:] = flat[0], flat[1]
        self.codes[: len(codes)] = codes
        for a in (self.ref_ids, self.hyp_ids):  # the C entry point checks the offsets, not the ids
            assert a.size == 0 or (0 <= int(a.min()) and int(a.max()) < self.n_phones)


@dataclass
class ScoreHandle:
    """a launch in flight: what ``score_collect`` needs, and what must stay alive until the kernel has run"""
    pack: ScorePack
    device_buffer: Optional[torch.Tensor]
    out: Optional[torch.Tensor]  # int32 [2, P] on the device: per_dist | pfer24
    stream: Optional[torch.cuda.Stream]


def launch_packed(pack: ScorePack, buf: torch.Tensor, out: torch.Tensor, s: torch.cuda.Stream) -> None:
    """the kernel alone on stream ``s``: ``buf`` is the device copy of ``pack.buffer``, ``out`` int32 [2, P]"""
    base, o = buf.data_ptr(), pack.offsets
    i32p = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().wipa_edit_distance_batch(
        base + o["ref_ids"], base + o["ref_off"], base + o["hyp_ids"], base + o["hyp_off"], base + o["order"], pack.P,
        base + o["codes"] if pack.has_features else None, pack.n_phones, pack.ref_off.ctypes.data_as(i32p),
        pack.hyp_off.ctypes.data_as(i32p), out.data_ptr(), out.data_ptr() + 4 * pack.P, sptr(s)), "wipa_edit_distance_batch")


def score_launch(ref_phones: Sequence[Sequence[str]], hyp_phones: Sequence[Sequence[str]],
                 features: Optional[Callable[[str], Sequence[int]]] = None) -> ScoreHandle:
    """Pack the pairs (``ScorePack``; ``features(phone)`` -> 24 values in {-1, 0, +1} is called once per distinct phone, ``None`` =
    PER only), copy the pack in one transfer and launch on the current library stream.  Returns at once."""
    pack = ScorePack(ref_phones, hyp_phones, features)
    dev = device()
    _lib.lib()
    if pack.P == 0:
        return ScoreHandle(pack, None, None, None)
    with on_stream() as s:
        buf = torch.empty(pack.nbytes, dtype=torch.uint8, device=dev)
        buf.copy_(pack.buffer, non_blocking=True)  # offsets, order, ids and codes: one copy
        out = torch.empty(2, pack.P, dtype=torch.int32, device=dev)
        launch_packed(pack, buf, out, s)
    return ScoreHandle(pack, buf, out, s)


def score_collect(handle: ScoreHandle) -> Tuple[np.ndarray, np.ndarray]:
    """(per_dist, pfer24) as int64 arrays, one entry per pair of the call; -1 where a side was longer than ``MAX_LEN`` and the
    pair was not launched.  Copies the results back and synchronises the launch's stream."""
    pack = handle.pack
    per, pf = np.full(pack.n_total, -1, dtype=np.int64), np.full(pack.n_total, -1, dtype=np.int64)
    if handle.out is not None:
        host = torch.empty(2, pack.P, dtype=torch.int32, pin_memory=True)
        with torch.cuda.stream(handle.stream):
            host.copy_(handle.out, non_blocking=True)
        handle.stream.synchronize()
        got = host.numpy()
        per[pack.kept], pf[pack.kept] = got[0], got[1]
    return per, pf


def score_pairs(ref_phones: Sequence[Sequence[str]], hyp_phones: Sequence[Sequence[str]],
                features: Optional[Callable[[str], Sequence[int]]] = None) -> Tuple[np.ndarray, np.ndarray]:
    return score_collect(score_launch(ref_phones, hyp_phones, features))
