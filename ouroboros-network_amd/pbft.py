"""Byron ledger-view checks -- what the reference's PBFT instance checks per
regular header beside the block signature (ouroboros-consensus/src/Ouroboros/
Consensus/Protocol/PBFT.hs:322-357): the issuer is a delegate of a genesis key
in the ledger's delegation map, the slot does not go back behind the last
signed slot, and that genesis key has not signed more than ``threshold`` of the
last ``window`` blocks.

``byron_key_hash`` / ``pbft_checks`` / ``pbft_window_fold`` call the library
(``csrc/sha3.h``, ``csrc/pbft_view.h``, ``k_pbft_checks``,
``ouro_pbft_window_fold``); there is no CPU fallback other than the library's
own host path.  ``key_hash`` / ``pbft_rule`` restate the same rules in plain
Python -- hashlib for the two hashes, bisect for the lookup, a deque and a dict
for the window, following PBFT/State.hs line by line -- for the tests' expected
side; nothing in them comes from the library.

Pinned by the reference's fixtures (tests/test_pbft_rule.py): hashVerKey =
Blake2b-224 of SHA3-256 of the key's CBOR encoding, the direction of the lookup
(delegate -> genesis), and the serialised window.
"""
from __future__ import annotations

import bisect
import ctypes
import hashlib
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from ._native import (LV_NO_POOL, PBFT_ALL_OK, PBFT_BOUNDARY, PBFT_DELEGATE_KNOWN, PBFT_SLOT_OK,
                      PBFT_WINDOW_OK)
from ._pack import ptr

__all__ = ["PBftViews", "PBftState", "byron_key_hash", "pbft_checks", "pbft_window_fold",
           "validate_chain_pbft_cbor",
           "key_hash", "pbft_rule", "PBFT_ALL_OK", "PBFT_BOUNDARY", "PBFT_DELEGATE_KNOWN",
           "PBFT_SLOT_OK", "PBFT_WINDOW_OK"]

PACK_OK, PACK_EBB = 0, 6   # the Byron slicer's statuses of a regular / boundary header


class PBftViews:
    """A delegation schedule (``ouro_pbft_views``): ``entries`` is a sequence
    of (first_slot, [(delegate id, genesis id), ...]) by ascending first_slot,
    the first at slot 0.  Pairs are sorted by delegate id here unless
    sort=False; everything else is passed as given, so that the library's own
    checks can be tested."""

    def __init__(self, entries: Sequence[Tuple[int, Sequence[Tuple[bytes, bytes]]]], window: int,
                 threshold: int, sort: bool = True):
        self.entries = [(int(fs), tuple(sorted(ps) if sort else ps)) for fs, ps in entries]
        self.window, self.threshold = int(window), int(threshold)
        k = len(self.entries)
        rows = [p for _, ps in self.entries for p in ps]
        self.first_slot = np.array([fs for fs, _ in self.entries], np.uint64)
        self.dlg_begin = np.zeros(k + 1, np.uint32)
        for j, (_, ps) in enumerate(self.entries):
            self.dlg_begin[j + 1] = self.dlg_begin[j] + len(ps)
        m = max(len(rows), 1)
        self.delegate_id = np.zeros((m, 28), np.uint8)
        self.genesis_id = np.zeros((m, 28), np.uint8)
        for r, (d, g) in enumerate(rows):
            self.delegate_id[r] = np.frombuffer(d, np.uint8)
            self.genesis_id[r] = np.frombuffer(g, np.uint8)
        self.rows = len(rows)

    def c_struct(self) -> _native.PBftViewsC:
        return _native.PBftViewsC(len(self.entries), self.first_slot.ctypes.data,
                                  self.dlg_begin.ctypes.data, self.delegate_id.ctypes.data,
                                  self.genesis_id.ctypes.data, self.window, self.threshold)

    def genesis_of_row(self, row: int) -> bytes:
        return self.genesis_id[row].tobytes()


class PBftState:
    """The signing window of a chain state (``ouro_pbft_state``; PBftState's
    inWindow): (slot, genesis id) pairs, oldest first."""

    def __init__(self, signers: Sequence[Tuple[int, bytes]] = ()):
        self.signers: List[Tuple[int, bytes]] = [(int(s), bytes(g)) for s, g in signers]

    def __eq__(self, other) -> bool:
        return isinstance(other, PBftState) and self.signers == other.signers

    def __repr__(self) -> str:
        return f"PBftState({[(s, g.hex()) for s, g in self.signers]})"

    def arrays(self):
        n = len(self.signers)
        ids = np.zeros((max(n, 1), 28), np.uint8)
        slots = np.zeros(max(n, 1), np.uint64)
        for i, (s, g) in enumerate(self.signers):
            ids[i] = np.frombuffer(g, np.uint8)
            slots[i] = s
        return n, ids, slots

    # the reference's serialisation format version 1 (PBFT/State.hs:278-306):
    # [1, {genesis id: [slots]}], the map as `invert` builds it

    @classmethod
    def from_cbor(cls, buf: bytes) -> "PBftState":
        """decodePBftState: uninvert sorts the (slot, key) pairs by slot (a
        stable sort over Map.toList's order)."""
        from . import header as H

        buf = bytes(buf)
        ver, body = H.array_items(buf, 0)
        if H.uint_at(buf, ver[0]) != 1:
            raise ValueError("PBftState: serialisation format version is not 1")
        major, cnt, at = H._head(buf, body[0])
        if major != 5:
            raise ValueError("PBftState: not a map")
        pairs = []
        for _ in range(cnt):
            key = H.bytes_at(buf, at)
            at = H.skip(buf, at)
            lmajor, lcnt, at = H._head(buf, at)
            if lmajor != 4:
                raise ValueError("PBftState: not a list of slots")
            while lcnt != 0:  # (a Haskell list: indefinite length, lcnt = -1, up to the break)
                if lcnt < 0 and buf[at] == 0xFF:
                    at += 1
                    break
                pairs.append((H.uint_at(buf, at), key))
                at = H.skip(buf, at)
                lcnt -= lcnt > 0
        if at != len(buf):
            raise ValueError("PBftState: trailing bytes")
        pairs.sort(key=lambda p: p[0])
        return cls(pairs)

    def to_cbor(self) -> bytes:
        """encodePBftState: invert folds from the oldest signer and prepends,
        so each key's slots stand newest first; a Haskell list is encoded with
        indefinite length, the map with its keys ascending."""
        inv: Dict[bytes, List[int]] = {}
        for s, g in self.signers:
            inv.setdefault(g, []).insert(0, s)
        out = bytearray(b"\x82\x01" + _head(5, len(inv)))
        for g in sorted(inv):
            out += _head(2, len(g)) + g + b"\x9f"
            for s in inv[g]:
                out += _head(0, s)
            out += b"\xff"
        return bytes(out)


def _head(major: int, val: int) -> bytes:
    if val < 24:
        return bytes([major << 5 | val])
    for code, size in ((24, 1), (25, 2), (26, 4), (27, 8)):
        if val < 1 << (8 * size):
            return bytes([major << 5 | code]) + val.to_bytes(size, "big")
    raise ValueError("CBOR head out of range")


def _state_args(state: Optional[PBftState], window: int):
    """(state struct or None, id_out, slot_out, n_out, keep-alive)"""
    if state is None:
        return None, None, None, None, ()
    n, ids, slots = state.arrays()
    cap = max(int(window), 1)
    id_out = np.zeros((cap, 28), np.uint8)
    slot_out = np.zeros(cap, np.uint64)
    n_out = ctypes.c_size_t(0)
    return _native.PBftStateC(n, ids.ctypes.data, slots.ctypes.data), id_out, slot_out, n_out, (
        ids, slots)


def _state_after(id_out, slot_out, n_out) -> PBftState:
    return PBftState([(int(slot_out[i]), id_out[i].tobytes()) for i in range(n_out.value)])


def byron_key_hash(xpub, *, host: bool = False) -> np.ndarray:
    """``ouro_byron_key_hash_batch``: n x 64 XPub bytes -> n x 28 key hashes."""
    x = np.ascontiguousarray(xpub, np.uint8).reshape(-1, 64)
    n = x.shape[0]
    out = np.zeros((max(n, 1), 28), np.uint8)
    name = "ouro_byron_key_hash_batch" + ("_host" if host else "")
    _native.check(getattr(_native.load(), name)(n, ptr(x) if n else None, ptr(out)), name)
    return out[:n]


def pbft_checks(delegate_vk, slot, status, views: PBftViews, *, state: Optional[PBftState] = None,
                host: bool = False):
    """The Byron ledger-view checks of n sliced Byron header rows (the columns
    of ``ouro_byron_pack_cbor``, the slots and the slicer's status).  Returns
    (pbft, genesis_row, signed_count[, state_after]): the PBFT_* bits, each
    delegate's schedule row (LV_NO_POOL: none) and, with ``state``, the fold's
    counts and the window afterwards.  host=True: the library's host path."""
    vk = np.ascontiguousarray(delegate_vk, np.uint8).reshape(-1, 64)
    n = vk.shape[0]
    sl = np.ascontiguousarray(slot, np.uint64).reshape(n)
    st = np.ascontiguousarray(status, np.uint8).reshape(n)
    bits = np.zeros(max(n, 1), np.uint8)
    rows = np.zeros(max(n, 1), np.uint32)
    cnt = np.zeros(max(n, 1), np.uint64)
    cv = views.c_struct()
    cs, id_out, slot_out, n_out, _keep = _state_args(state, views.window)
    name = "ouro_pbft_ledger_checks" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(
        n, ptr(vk) if n else None, ptr(sl) if n else None, ptr(st) if n else None,
        ctypes.byref(cv), None if cs is None else ctypes.byref(cs),
        None if cs is None else ptr(id_out), None if cs is None else ptr(slot_out),
        None if cs is None else ctypes.addressof(n_out), ptr(bits), ptr(rows), ptr(cnt))
    _native.check(rc, name)
    out = (bits[:n], rows[:n], cnt[:n])
    return out + (_state_after(id_out, slot_out, n_out),) if state is not None else out


def pbft_window_fold(pbft, genesis_row, slot, views: PBftViews, state: PBftState):
    """``ouro_pbft_window_fold``: SLOT_OK and WINDOW_OK into a copy of ``pbft``
    in stream order.  Returns (pbft, signed_count, state_after)."""
    bits = np.array(pbft, np.uint8).reshape(-1)
    n = bits.shape[0]
    rows = np.ascontiguousarray(genesis_row, np.uint32).reshape(n)
    sl = np.ascontiguousarray(slot, np.uint64).reshape(n)
    cnt = np.zeros(max(n, 1), np.uint64)
    cv = views.c_struct()
    cs, id_out, slot_out, n_out, _keep = _state_args(state, views.window)
    buf = bits if n else np.zeros(1, np.uint8)
    rc = _native.load().ouro_pbft_window_fold(
        n, ptr(rows) if n else None, ptr(sl) if n else None, ctypes.byref(cv), ctypes.byref(cs),
        ptr(id_out), ptr(slot_out), ctypes.addressof(n_out), ptr(buf), ptr(cnt))
    _native.check(rc, "ouro_pbft_window_fold")
    return bits, cnt[:n], _state_after(id_out, slot_out, n_out)


def validate_chain_pbft_cbor(raw_headers, slots_per_kes_period: int, protocol_magic: int,
                             views, globals_, pbft_views: PBftViews, *,
                             state: Optional[PBftState] = None, **kw):
    """``ouro_chain_validate_ledger_pbft_cbor``: header.validate_chain_ledger_cbor
    (its arguments and its tuple) with the Byron ledger-view checks in the same
    call; the tuple goes on with (pbft, genesis_row, signed_count,
    state_after).  ``state`` = None: no fold."""
    from . import header as H

    return H.validate_chain_ledger_cbor(raw_headers, slots_per_kes_period, protocol_magic, views,
                                        globals_, pbft=pbft_views, pbft_state=state, **kw)


# ---- the rules restated (the tests' expected side) -----------------------------

def key_hash(xpub: bytes) -> bytes:
    """CC.Common.hashKey: Blake2b-224 of SHA3-256 of the key's CBOR encoding
    (bytes(64): 58 40, then the XPub)."""
    return hashlib.blake2b(hashlib.sha3_256(b"\x58\x40" + bytes(xpub)).digest(),
                           digest_size=28).digest()


def pbft_rule(views: PBftViews, delegate_vk: Sequence[bytes], slot: Sequence[int],
              status: Sequence[int], state: Optional[PBftState] = None):
    """(pbft, genesis_row, signed_count, state_after or None) of n rows in
    stream order: the lookup of PBFT.hs:346-350 and, with ``state``, the slot
    check (340-344), ``append`` (State.hs:207-229) and the threshold."""
    firsts = [fs for fs, _ in views.entries]
    window: deque = deque(state.signers if state is not None else ())
    counts: Dict[bytes, int] = {}
    for _, g in window:
        counts[g] = counts.get(g, 0) + 1
    bits_out, rows_out, cnt_out = [], [], []
    for vk, s, st in zip(delegate_vk, slot, status):
        bits, row, cnt = 0, LV_NO_POOL, 0
        if st == PACK_EBB:
            bits = PBFT_BOUNDARY | PBFT_ALL_OK       # PBftValidateBoundary: return state
        elif st == PACK_OK:
            j = bisect.bisect_right(firsts, s) - 1
            ps = views.entries[j][1]
            ids = [d for d, _ in ps]
            kh = key_hash(vk)
            r = bisect.bisect_left(ids, kh)
            if r < len(ids) and ids[r] == kh:        # Bimap.lookupR
                bits |= PBFT_DELEGATE_KNOWN
                row = int(views.dlg_begin[j]) + r
                if state is not None:
                    gk = ps[r][1]
                    if not window or s >= window[-1][0]:   # NotOrigin slot >= lastSignedSlot
                        bits |= PBFT_SLOT_OK
                    full = len(window) == views.window
                    window.append((s, gk))                 # inWindow |> signer
                    counts[gk] = counts.get(gk, 0) + 1
                    if full:                               # size inWindow == n: x :<| xs
                        _, old = window.popleft()
                        counts[old] -= 1
                        if counts[old] == 0:
                            del counts[old]
                    cnt = counts.get(gk, 0)                # countSignedBy
                    if cnt <= views.threshold:
                        bits |= PBFT_WINDOW_OK
        bits_out.append(bits)
        rows_out.append(row)
        cnt_out.append(cnt)
    after = PBftState(list(window)) if state is not None else None
    return (np.array(bits_out, np.uint8), np.array(rows_out, np.uint32),
            np.array(cnt_out, np.uint64), after)
