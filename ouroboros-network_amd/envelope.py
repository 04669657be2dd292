"""The header envelope of a raw chain, restated in Python from the reference:
validateEnvelope (ouroboros-consensus/src/Ouroboros/Consensus/
HeaderValidation.hs:297-344) over raw wire headers, and every header's hash.

This module is the independent statement of the rule that csrc/envelope.h
implements for the host and the device: it is written from the reference and
from this package's Python slicers (header.parse_header, byron.byron_status)
and hashlib, never from the C.  tests/test_envelope_rule.py pins it to the
reference's golden fixtures and the C to it.

Header hash
  TPraos  Blake2b-256 of the #6.24 payload, the [header_body, kes_sig] item as
          it stands (Shelley/Ledger/Block.hs:106,142, bhHash).
  Byron   Blake2b-256(0x82 || kind || header item), kind 1 for a regular header
          and 0 for an epoch-boundary one (Byron/Ledger/Block.hs:74,
          Orphans.hs:101 wrapBoundaryBytes), whatever the wire form.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import byron as B
from . import header as H

ENV_BLOCKNO_OK = 0x01
ENV_SLOT_OK = 0x02
ENV_PREVHASH_OK = 0x04
ENV_EXTRA_OK = 0x08
ENV_ALL_OK = 0x0F

GENESIS = "genesis"  # headerPrevHash = GenesisHash
W64 = 2**64


def _b2b(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


@dataclass
class Cfg:
    """byron_epoch_slots: the slots of a Byron epoch; limits: None, or
    (max_header_size, max_body_size, max_major_pv) of ledger-specs chainChecks."""
    byron_epoch_slots: int = 21600
    limits: Optional[Tuple[int, int, int]] = None


@dataclass
class Tip:
    """AnnTip: the last header of the chain so far.  usable = False: a header
    that could not be read; nothing links to it."""
    proto: int
    is_ebb: bool
    slot: int
    block_no: int
    hash: bytes
    usable: bool = True


ORIGIN = None  # WithOrigin's Origin


@dataclass
class Record:
    """One header as validateEnvelope sees it."""
    proto: int
    is_ebb: bool
    slot: int
    block_no: int
    prev: object          # GENESIS, 32 bytes, or None (a field that is neither)
    hash: bytes
    header_size: int = 0  # TPraos: bytes of the [header_body, kes_sig] item
    body_size: Optional[int] = None   # TPraos body field 7 (None: not a uint)
    prot_major: Optional[int] = None  # TPraos body field 13


def _uint_or_none(buf: bytes, i: int) -> Optional[int]:
    try:
        mt, arg, _ = H._head(buf, i)
    except (H.CBORError, IndexError):
        return None
    return arg if mt == 0 and arg >= 0 else None


def _bytes32_or_none(buf: bytes, i: int) -> Optional[bytes]:
    try:
        b = H.bytes_at(buf, i)
    except (H.CBORError, IndexError):
        return None
    return b if len(b) == 32 else None


def _tpraos_record(raw: bytes) -> Optional[Record]:
    try:
        H.parse_header(raw)  # the slicer's acceptance
    except (H.CBORError, IndexError):
        return None
    buf = bytes(raw)
    i = 0
    mt, arg, j = H._head(buf, 0)
    if mt == 4:  # [era, wrapped]
        i = H.skip(buf, j)
    _, _, j = H._head(buf, i)        # tag 24
    _, ln, k = H._head(buf, j)       # the byte string
    payload = buf[k:k + ln]
    body = H.array_items(payload, 0)[0]
    f = H.array_items(payload, body[0])
    if payload[f[2][0]:f[2][1]] == b"\xf6":
        prev = GENESIS
    else:
        prev = _bytes32_or_none(payload, f[2][0])
    return Record(proto=H.PROTO_TPRAOS, is_ebb=False, slot=H.uint_at(payload, f[1][0]),
                  block_no=H.uint_at(payload, f[0][0]), prev=prev, hash=_b2b(payload),
                  header_size=len(payload), body_size=_uint_or_none(payload, f[7][0]),
                  prot_major=_uint_or_none(payload, f[13][0]))


def _byron_item(raw: bytes) -> Tuple[int, bytes]:
    """(kind, the header item's bytes) of a Byron header the slicer accepts."""
    buf = bytes(raw)
    mt, arg, j = H._head(buf, 0)
    pos, kind, nested = 0, None, mt == 4
    if nested:
        mt1, a1, j1 = H._head(buf, j)
        if mt1 == 0:  # F3: [0, F2]
            _, _, j = H._head(buf, j1)
        ks = H.array_items(buf, j)
        kind = H.uint_at(buf, ks[0][0])
        pos = ks[1][1]
    _, _, j = H._head(buf, pos)   # tag 24
    _, ln, k = H._head(buf, j)    # the byte string
    payload = buf[k:k + ln]
    if nested:
        return kind, payload
    top = H.array_items(payload, 0)  # F1: [kind, header]
    return H.uint_at(payload, top[0][0]), payload[top[1][0]:top[1][1]]


def _byron_record(raw: bytes, epoch_slots: int) -> Optional[Record]:
    st, _ = B.byron_status(raw)
    if st not in (B.PACK_OK, B.PACK_EBB):
        return None
    kind, item = _byron_item(raw)
    ebb = st == B.PACK_EBB
    assert kind == (0 if ebb else 1)
    try:
        f = H.array_items(item, 0)
        if len(f) != 5:
            return None
        prev = _bytes32_or_none(item, f[1][0])
        cons = H.array_items(item, f[3][0])
        if ebb:   # [epoch, [difficulty]]
            if len(cons) != 2:
                return None
            epoch, in_epoch, diff_at = _uint_or_none(item, cons[0][0]), 0, cons[1][0]
        else:     # [slotId, leaderKey, difficulty, signature], slotId = [epoch, slot]
            sid = H.array_items(item, cons[0][0])
            if len(sid) != 2:
                return None
            epoch, in_epoch = _uint_or_none(item, sid[0][0]), _uint_or_none(item, sid[1][0])
            diff_at = cons[2][0]
        d = H.array_items(item, diff_at)
        if len(d) != 1:
            return None
        diff = _uint_or_none(item, d[0][0])
    except (H.CBORError, IndexError):
        return None
    if prev is None or epoch is None or in_epoch is None or diff is None:
        return None
    # the boundary-header decoder: GenesisHash iff epoch 0
    if ebb and epoch == 0:
        prev = GENESIS
    return Record(proto=H.PROTO_PBFT, is_ebb=ebb, slot=(epoch * epoch_slots + in_epoch) % W64,
                  block_no=diff, prev=prev, hash=_b2b(bytes([0x82, 0 if ebb else 1]) + item))


def header_record(raw: bytes, cfg: Cfg = Cfg()) -> Optional[Record]:
    """The envelope record of a raw header, None when it cannot be used (the
    slicer of its era rejects it, or its envelope fields have another shape)."""
    if H.era_class(raw) == H.PROTO_PBFT:
        return _byron_record(raw, cfg.byron_epoch_slots)
    return _tpraos_record(raw)


def header_hash(raw: bytes) -> bytes:
    """headerHash of a raw header; 32 zero bytes for one that cannot be used."""
    r = header_record(raw)
    return r.hash if r else bytes(32)


class Unusable:
    """The predecessor was a header that could not be used."""


def _succ(x: int) -> Optional[int]:
    return x + 1 if x + 1 < W64 else None  # succ maxBound has no value


def link(prev, cur: Optional[Record], cfg: Cfg) -> int:
    """validateEnvelope of `cur` (None: a header that cannot be used) on top of
    `prev` (ORIGIN, a Tip, a Record, or an Unusable) as ENV_* bits, all four
    evaluated."""
    if cur is None:
        return 0
    bits = 0
    extra = True
    if cur.proto == H.PROTO_PBFT:
        if cur.is_ebb:  # Byron/Ledger/HeaderValidation.hs:61-72
            extra = cur.slot % cfg.byron_epoch_slots == 0
    elif cfg.limits is not None:  # chainChecks
        mh, mb, mv = cfg.limits
        extra = (cur.body_size is not None and cur.prot_major is not None and
                 cur.header_size <= mh and cur.body_size <= mb and cur.prot_major <= mv)
    if extra:
        bits |= ENV_EXTRA_OK
    if prev is ORIGIN:
        if cur.block_no == 0:       # expectedFirstBlockNo
            bits |= ENV_BLOCKNO_OK
        bits |= ENV_SLOT_OK         # minimumPossibleSlotNo = 0
        if cur.prev == GENESIS:     # checkPrevHash' Origin GenesisHash
            bits |= ENV_PREVHASH_OK
        return bits
    if isinstance(prev, Unusable) or (isinstance(prev, Tip) and not prev.usable):
        return bits
    byron = prev.proto == H.PROTO_PBFT and cur.proto == H.PROTO_PBFT
    # Byron/Ledger/HeaderValidation.hs:46-56; everything else, a change of era
    # included (HardFork/Combinator/Block.hs:235-252), is succ
    want_no = prev.block_no if byron and not prev.is_ebb and cur.is_ebb else _succ(prev.block_no)
    min_slot = prev.slot if byron and prev.is_ebb and not cur.is_ebb else _succ(prev.slot)
    if want_no is not None and cur.block_no == want_no:
        bits |= ENV_BLOCKNO_OK
    if min_slot is not None and cur.slot >= min_slot:
        bits |= ENV_SLOT_OK
    if isinstance(cur.prev, bytes) and cur.prev == prev.hash:
        bits |= ENV_PREVHASH_OK
    return bits


def tip_of(rec) -> Tip:
    """The tip after header `rec` (None: one that could not be used)."""
    if rec is None:
        return Tip(0xFF, False, 0, 0, bytes(32), usable=False)
    return Tip(rec.proto, rec.is_ebb, rec.slot, rec.block_no, rec.hash)


def validate_envelope(raws: Sequence[bytes], tip=ORIGIN, cfg: Cfg = Cfg()):
    """(records, hashes, bits, tip_out) of a raw header stream: header i on top
    of header i - 1 as given, header 0 on top of `tip` (ORIGIN or a Tip)."""
    recs: List[Optional[Record]] = [header_record(r, cfg) for r in raws]
    bits = []
    prev = tip
    for r in recs:
        bits.append(link(prev, r, cfg))
        prev = r if r is not None else Unusable()
    hashes = [r.hash if r else bytes(32) for r in recs]
    tip_out = tip if not recs else tip_of(recs[-1])
    return recs, hashes, bits, tip_out


def first_invalid(bits, crypto_valid=None) -> int:
    """The length of the longest prefix the reference's sequential fold
    accepts: the first i with an ENV_* bit clear (or crypto_valid[i] false);
    len(bits) when there is none."""
    for i, b in enumerate(bits):
        if (int(b) & ENV_ALL_OK) != ENV_ALL_OK:
            return i
        if crypto_valid is not None and not crypto_valid[i]:
            return i
    return len(bits)
