"""Whole-block storage integrity (verifyBlockIntegrity) and the batched
Blake2b-256, from raw block CBOR.

* ``verify_block_integrity_cbor``: ouro_block_integrity_verify_cbor[_host]
  (include/ouro_verify.h): verifyHeaderIntegrity (Sum6KES) and
  blockMatchesHeader (bbHash == the header's bodyHash) per block;
* ``blake2b256_batch``: ouro_blake2b256_batch[_host];
* ``parse_block``: a pure-Python restatement of the block slicer
  (csrc/cbor_block.h), written independently of it the way
  header.parse_header stands beside csrc/cbor.h; the tests take their
  expectations from it, from hashlib and from the oracle, never from the
  library.

Block encodings (the reference's golden files):
    [header, txBodies, txWitnesses, txMetadata]      Shelley on disk
    #6.24(bytes .cbor block)                         Shelley on the wire
    [tag, block]                                     Cardano on disk
    #6.24(bytes .cbor [tag, block])                  Cardano on the wire
The HFC block tag is 0 = Byron EBB, 1 = Byron regular, 2 and up = Shelley
family.  bbHash = Blake2b-256 of the three Blake2b-256 digests of items 1..3,
each over the item's bytes as they stand in the block.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from . import _native
from .header import (PACK_EBYRON, PACK_ECBOR, PACK_ESHAPE, PACK_ESIZE, PACK_ESPAN,  # noqa: F401
                     PACK_OK, raw_triplet)

BLK_KES_OK = 0x01    # verifyHeaderIntegrity
BLK_BODY_OK = 0x02   # blockMatchesHeader
BLK_ALL_OK = 0x03    # verifyBlockIntegrity

MAX_DEPTH = 64       # csrc/cbor.h kMaxDepth: open containers below the item itself


class BlockError(ValueError):
    """A block the slicer rejects; .status is the OURO_PACK_* code."""

    def __init__(self, status: int, what: str):
        super().__init__(what)
        self.status = status


def _fail(status, what):
    raise BlockError(status, what)


def _head(buf: bytes, i: int, end: int):
    """(major type, argument or None for indefinite, index after the head)"""
    if i >= end:
        _fail(PACK_ECBOR, "truncated")
    ib = buf[i]
    mt, ai = ib >> 5, ib & 31
    i += 1
    if ai < 24:
        return mt, ai, i
    if ai <= 27:
        w = 1 << (ai - 24)
        if end - i < w:
            _fail(PACK_ECBOR, "truncated head")
        return mt, int.from_bytes(buf[i:i + w], "big"), i + w
    if ai == 31:
        return mt, None, i
    _fail(PACK_ECBOR, f"reserved additional info {ai}")


def _skip(buf: bytes, i: int, end: int) -> int:
    """Index past the data item at i, without recursion: a stack of the items
    still to read per open container (None: until a break), at most MAX_DEPTH
    open below the item."""
    stack = [1]
    while True:
        while stack and stack[-1] == 0:
            stack.pop()
        if not stack:
            return i
        if stack[-1] is None:
            if i >= end:
                _fail(PACK_ECBOR, "truncated")
            if buf[i] == 0xFF:
                i += 1
                stack.pop()
                continue
        else:
            stack[-1] -= 1
        mt, arg, j = _head(buf, i, end)
        push = False
        count = 0
        if mt in (0, 1, 7):
            i = j
        elif mt in (2, 3):
            if arg is None:
                push, count = True, None
                i = j
            else:
                if end - j < arg:
                    _fail(PACK_ECBOR, "truncated string")
                i = j + arg
        elif mt in (4, 5):
            if arg is not None and arg > end:
                _fail(PACK_ECBOR, "count beyond the input")
            push = True
            count = None if arg is None else (2 * arg if mt == 5 else arg)
            i = j
        else:  # a tag, then its content
            push, count = True, 1
            i = j
        if push:
            if len(stack) - 1 == MAX_DEPTH:
                _fail(PACK_ECBOR, "nested too deep")
            stack.append(count)


def _array_items(buf, i, end, cap):
    """Spans of the elements of the definite array at i; None when there are
    more than `cap` (every element is still read first)."""
    mt, arg, j = _head(buf, i, end)
    if mt != 4 or arg is None:
        _fail(PACK_ECBOR, "expected a definite array")
    out = []
    for _ in range(arg):
        k = _skip(buf, j, end)
        out.append((j, k))
        j = k
    return None if arg > cap else out


def _uint_at(buf, i, end):
    try:
        mt, arg, _ = _head(buf, i, end)
    except BlockError:
        _fail(PACK_ESHAPE, "expected uint")
    if mt != 0 or arg is None:
        _fail(PACK_ESHAPE, "expected uint")
    return arg


def _bytes_at(buf, i, end):
    """The definite byte string at i, or None (wrong type)"""
    try:
        mt, arg, j = _head(buf, i, end)
    except BlockError:
        return None
    if mt != 2 or arg is None or end - j < arg:
        return None
    return bytes(buf[j:j + arg])


@dataclass
class ShelleyBlock:
    tag: int                  # HFC block tag (2 Shelley, 3 Allegra, 4 Mary); 2 if bare
    slot: int
    hot_vk: bytes
    ocert_kes_period: int
    kes_sig: bytes
    header_body_span: Tuple[int, int]   # the KES message inside the block
    body_hash: bytes                    # header body field 8 (claimed)
    segments: List[Tuple[int, int]]     # (offset, length) of items 1..3

    def bb_hash(self, raw: bytes) -> bytes:
        h = lambda m: hashlib.blake2b(m, digest_size=32).digest()  # noqa: E731
        return h(b"".join(h(raw[o:o + n]) for o, n in self.segments))


def parse_block(raw: bytes) -> ShelleyBlock:
    """Slice one block; raises BlockError(status) where the C slicer rejects."""
    buf = bytes(raw)
    end = len(buf)
    tag = 2
    mt, arg, j = _head(buf, 0, end)
    if mt == 6:
        if arg != 24:
            _fail(PACK_ESHAPE, "expected tag 24")
        mt, arg, k = _head(buf, j, end)
        if mt != 2 or arg is None:
            _fail(PACK_ESHAPE, "expected definite CBOR-in-bytes")
        if end - k < arg or k + arg != end:
            _fail(PACK_ECBOR, "payload past the span or bytes after the block")
        mt, arg, j = _head(buf, k, end)
    if mt != 4 or arg is None:
        _fail(PACK_ESHAPE, "expected a definite array")
    if arg == 2:
        tag = _uint_at(buf, j, end)
        if tag <= 1:
            _fail(PACK_EBYRON, "a Byron block")
        pos = _skip(buf, j, end)
        mt, arg, j = _head(buf, pos, end)
        if mt != 4 or arg is None:
            _fail(PACK_ESHAPE, "expected a definite array")
    if arg != 4:
        _fail(PACK_ESHAPE, "a block has 4 items")
    # item 0: [header_body, kes_sig]
    mt, arg, b0 = _head(buf, j, end)
    if mt != 4 or arg is None:
        _fail(PACK_ECBOR, "header: expected a definite array")
    if arg != 2:
        _fail(PACK_ESHAPE, "header must be [body, sig]")
    f = _array_items(buf, b0, end, 15)
    if f is None or len(f) != 15:
        _fail(PACK_ESHAPE, "header body must have 15 fields")
    b1 = s0 = f[14][1]
    s1 = _skip(buf, s0, end)
    eta = _array_items(buf, f[5][0], end, 2)
    lead = _array_items(buf, f[6][0], end, 2)
    if eta is None or lead is None or len(eta) != 2 or len(lead) != 2:
        _fail(PACK_ESHAPE, "VRF certificates must be [output, proof]")
    _uint_at(buf, f[0][0], end)
    slot = _uint_at(buf, f[1][0], end)
    sized = []
    for a, b, want in ((f[3][0], f[4][0], (32, 32)), (eta[0][0], eta[1][0], (64, 80)),
                       (lead[0][0], lead[1][0], (64, 80))):
        x, y = _bytes_at(buf, a, end), _bytes_at(buf, b, end)
        if x is None or y is None:
            _fail(PACK_ESHAPE, "expected bytes")
        sized += [(x, want[0]), (y, want[1])]
    hot = _bytes_at(buf, f[9][0], end)
    if hot is None:
        _fail(PACK_ESHAPE, "hot key: expected bytes")
    _uint_at(buf, f[10][0], end)
    c0 = _uint_at(buf, f[11][0], end)
    sigma, ksig = _bytes_at(buf, f[12][0], end), _bytes_at(buf, s0, end)
    if sigma is None or ksig is None:
        _fail(PACK_ESHAPE, "signatures: expected bytes")
    sized += [(hot, 32), (sigma, 64), (ksig, 448)]
    if any(len(x) != want for x, want in sized):
        _fail(PACK_ESIZE, "a fixed-size crypto field has the wrong length")
    bh = _bytes_at(buf, f[8][0], end)
    if bh is None:
        _fail(PACK_ESHAPE, "bodyHash: expected bytes")
    if len(bh) != 32:
        _fail(PACK_ESIZE, "bodyHash: expected 32 bytes")
    segs, p = [], s1
    for _ in range(3):
        q = _skip(buf, p, end)
        segs.append((p, q - p))
        p = q
    if p != end:
        _fail(PACK_ECBOR, "bytes after the block")
    return ShelleyBlock(tag=tag, slot=slot, hot_vk=hot, ocert_kes_period=c0, kes_sig=ksig,
                        header_body_span=(b0, b1), body_hash=bh, segments=segs)


def block_status(raw: bytes) -> int:
    """OURO_PACK_* as the slicer reports it"""
    try:
        parse_block(raw)
    except BlockError as e:
        return e.status
    return PACK_OK


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def verify_block_integrity_cbor(raws, slots_per_kes_period: int, host: bool = False):
    """verifyBlockIntegrity over raw blocks: returns (verdict, status,
    body_hash) -- BLK_* bits per block (0 for one that does not slice),
    PACK_* per block, and the computed bbHash (n x 32; zeros for a block that
    does not slice).  raws: a sequence of bytes or a (buf, off, len) triple.
    host=True: ouro_block_integrity_verify_cbor_host, no device touched."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    if ln.size != n:
        raise ValueError("off / len: one entry per block")
    status = np.zeros(max(n, 1), np.uint8)
    verdict = np.zeros(max(n, 1), np.uint8)
    body_hash = np.zeros((max(n, 1), 32), np.uint8)
    lib = _native.load()
    name = "ouro_block_integrity_verify_cbor" + ("_host" if host else "")
    rc = getattr(lib, name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n, slots_per_kes_period,
                            _ptr(status), _ptr(verdict), _ptr(body_hash))
    _native.check(rc, name)
    return verdict[:n], status[:n], body_hash[:n]


def blake2b256_batch(msgs, host: bool = False) -> np.ndarray:
    """Blake2b-256 of every message: (n, 32) uint8.  msgs: a sequence of bytes
    or a (buf, off, len) triple of spans inside buf (any alignment, overlapping
    spans allowed)."""
    buf, off, ln = raw_triplet(msgs)
    n = int(off.size)
    if ln.size != n:
        raise ValueError("off / len: one entry per message")
    out = np.zeros((max(n, 1), 32), np.uint8)
    lib = _native.load()
    name = "ouro_blake2b256_batch" + ("_host" if host else "")
    rc = getattr(lib, name)(n, _ptr(buf), buf.size, _ptr(off), _ptr(ln), _ptr(out))
    _native.check(rc, name)
    return out[:n]
