"""Transaction key witnesses from raw block CBOR: the tx ids and the Ed25519
verification of every witness over its transaction's id.

* ``parse_witnesses``: a pure-Python restatement of the witness slicer
  (csrc/cbor_witness.h), written independently of it the way block.parse_block
  stands beside csrc/cbor_block.h; the tests take their expectations from it,
  from hashlib and from the oracle, never from the library;
* ``verify_block_witnesses``: ouro_block_witness_verify_cbor[_host]
  (include/ouro_verify.h);
* ``count_block_witnesses``: ouro_block_witness_count_cbor[_host].

The rule.  A block is one of block.py's four encodings, a
definite array(4) that ends exactly at its span; item 0 (the header) and item 3
(the metadata) are skipped, not examined.
    txBodies    = [* map]              definite or indefinite; tx id =
                                       Blake2b-256 of the element as it stands
    txWitnesses = [* {uint => any}]    as many elements as txBodies
      key 0: [* [vkey: bytes(32), sig: bytes(64)]]
      key 2: [* [vkey: bytes(32), sig: bytes(64), chain_code: bytes(32), attributes]]
      any other key: skipped; a repeated key is walked again
An entry's fields are walked first (PACK_ECBOR), then their types (PACK_ESHAPE),
then their sizes (PACK_ESIZE).  Witnesses are numbered in the order the walk
meets them; each one's message is its transaction's id, verified as plain
Ed25519 with libsodium 1.0.18's rules, for both kinds.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from . import _native
from .block import BlockError, _bytes_at, _fail, _head, _skip, _uint_at
from .header import (PACK_EBYRON, PACK_ECBOR, PACK_ESHAPE, PACK_ESIZE, PACK_ESPAN,  # noqa: F401
                     PACK_OK, raw_triplet)

PACK_ECAP = 8        # OURO_PACK_ECAP: the block's rows pass a capacity
WIT_ALL_OK = 0x01    # OURO_WIT_ALL_OK


@dataclass
class Witness:
    tx: int          # index of its transaction within the block
    kind: int        # 0: a key witness; 2: a bootstrap witness
    vk: bytes
    sig: bytes


@dataclass
class BlockWitnesses:
    tx_spans: List[Tuple[int, int]]     # (offset, length) of every tx body
    witnesses: List[Witness]

    def tx_ids(self, raw: bytes) -> List[bytes]:
        return [hashlib.blake2b(raw[o:o + n], digest_size=32).digest() for o, n in self.tx_spans]


def _open(buf, i, end, want):
    """The array (want 4) or map (5) at i: (count or None, index after the head)"""
    mt, arg, j = _head(buf, i, end)
    if mt != want:
        _fail(PACK_ESHAPE, "expected an array" if want == 4 else "expected a map")
    return arg, j


def _walk(buf, i, end, count, item):
    """item(start) -> the index after it, for every item (pair) of the
    container whose first item is at i (count None: until the break); returns
    the index after the container"""
    k = 0
    while True:
        if count is None:
            if i >= end:
                _fail(PACK_ECBOR, "truncated before the break")
            if buf[i] == 0xFF:
                return i + 1
        elif k == count:
            return i
        k += 1
        i = item(i)


def parse_witnesses(raw: bytes) -> BlockWitnesses:
    """Slice one block; raises BlockError(status) where the C walker rejects."""
    buf = bytes(raw)
    end = len(buf)
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
        if _uint_at(buf, j, end) <= 1:
            _fail(PACK_EBYRON, "a Byron block")
        pos = _skip(buf, j, end)
        mt, arg, j = _head(buf, pos, end)
        if mt != 4 or arg is None:
            _fail(PACK_ESHAPE, "expected a definite array")
    if arg != 4:
        _fail(PACK_ESHAPE, "a block has 4 items")
    i = _skip(buf, j, end)                       # item 0: the header
    out = BlockWitnesses([], [])

    def body(at):
        mt, _, _ = _head(buf, at, end)
        if mt != 5:
            _fail(PACK_ESHAPE, "a tx body is a map")
        e = _skip(buf, at, end)
        out.tx_spans.append((at, e - at))
        return e

    count, i = _open(buf, i, end, 4)             # item 1: txBodies
    i = _walk(buf, i, end, count, body)
    ntx = len(out.tx_spans)
    count, i = _open(buf, i, end, 4)             # item 2: txWitnesses
    if count is not None and count != ntx:
        _fail(PACK_ESHAPE, "one witness set per tx body")
    sets = [0]

    def entry(t, key):
        nf = 2 if key == 0 else 4

        def one(at):
            mt, arg, f = _head(buf, at, end)
            if mt != 4 or arg != nf:
                _fail(PACK_ESHAPE, "a witness is a definite array(%d)" % nf)
            starts = []
            for _ in range(nf):
                starts.append(f)
                f = _skip(buf, f, end)
            got = [_bytes_at(buf, s, end) for s in starts[:3]]
            if any(g is None for g in got):
                _fail(PACK_ESHAPE, "expected bytes")
            if [len(g) for g in got] != [32, 64, 32][:len(got)]:
                _fail(PACK_ESIZE, "a witness field has the wrong length")
            out.witnesses.append(Witness(t, key, got[0], got[1]))
            return f
        return one

    def wset(at):
        t = sets[0]
        if t == ntx:
            _fail(PACK_ESHAPE, "more witness sets than tx bodies")

        def pair(at):
            key = _uint_at(buf, at, end)
            val = _skip(buf, at, end)
            if key not in (0, 2):
                return _skip(buf, val, end)
            count, first = _open(buf, val, end, 4)
            return _walk(buf, first, end, count, entry(t, key))

        count, first = _open(buf, at, end, 5)
        e = _walk(buf, first, end, count, pair)
        sets[0] += 1
        return e

    i = _walk(buf, i, end, count, wset)
    if sets[0] != ntx:
        _fail(PACK_ESHAPE, "fewer witness sets than tx bodies")
    i = _skip(buf, i, end)                       # item 3: the metadata
    if i != end:
        _fail(PACK_ECBOR, "bytes after the block")
    return out


def witness_status(raw: bytes) -> int:
    """OURO_PACK_* as the walker reports it"""
    try:
        parse_witnesses(raw)
    except BlockError as e:
        return e.status
    return PACK_OK


class WitnessOutC(ctypes.Structure):
    """Mirror of ``ouro_block_witness_out`` (include/ouro_verify.h)."""

    _fields_ = [("tx_cap", ctypes.c_size_t), ("wit_cap", ctypes.c_size_t)] + [
        (f, ctypes.c_void_p) for f in ("tx_begin", "wit_begin", "tx_id", "wit_tx", "wit_kind",
                                       "wit_ok", "wit_vk")]


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def count_block_witnesses(raws, host: bool = False):
    """The slicer's count pass: (status, ntx, nwit) per block, zeros where the
    block does not slice.  raws: a sequence of bytes or a (buf, off, len) triple."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    status = np.zeros(max(n, 1), np.uint8)
    ntx = np.zeros(max(n, 1), np.uint32)
    nwit = np.zeros(max(n, 1), np.uint32)
    name = "ouro_block_witness_count_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n, _ptr(status),
                                       _ptr(ntx), _ptr(nwit))
    _native.check(rc, name)
    return status[:n], ntx[:n], nwit[:n]


@dataclass
class WitnessResult:
    status: np.ndarray       # n: PACK_*
    verdict: np.ndarray      # n: WIT_ALL_OK or 0
    n_bad: np.ndarray        # n: the block's witnesses that do not verify
    tx_begin: np.ndarray     # n + 1: block i owns the tx rows [tx_begin[i], tx_begin[i + 1])
    wit_begin: np.ndarray    # n + 1
    tx_id: np.ndarray        # tx_cap x 32
    wit_tx: np.ndarray       # wit_cap: the witness's global tx row
    wit_kind: np.ndarray     # wit_cap: 0 or 2
    wit_ok: np.ndarray       # wit_cap: 1 = verifies
    wit_vk: np.ndarray       # wit_cap x 32


def verify_block_witnesses(raws, tx_cap: int = None, wit_cap: int = None, host: bool = False):
    """Every key witness of every block verified over its transaction's id: a
    WitnessResult.  tx_cap / wit_cap: the row capacities (default: what the
    count pass finds, so every block fits); a sliced block whose rows pass one
    has status PACK_ECAP and writes nothing.  host=True: the host path alone,
    no device touched."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    if ln.size != n:
        raise ValueError("off / len: one entry per block")
    if tx_cap is None or wit_cap is None:
        _, ntx, nwit = count_block_witnesses((buf, off, ln), host=host)
        tx_cap = int(ntx.sum()) if tx_cap is None else tx_cap
        wit_cap = int(nwit.sum()) if wit_cap is None else wit_cap
    r = WitnessResult(status=np.zeros(max(n, 1), np.uint8), verdict=np.zeros(max(n, 1), np.uint8),
                      n_bad=np.zeros(max(n, 1), np.uint32), tx_begin=np.zeros(n + 1, np.uint64),
                      wit_begin=np.zeros(n + 1, np.uint64),
                      tx_id=np.zeros((max(tx_cap, 1), 32), np.uint8),
                      wit_tx=np.zeros(max(wit_cap, 1), np.uint32),
                      wit_kind=np.zeros(max(wit_cap, 1), np.uint8),
                      wit_ok=np.zeros(max(wit_cap, 1), np.uint8),
                      wit_vk=np.zeros((max(wit_cap, 1), 32), np.uint8))
    out = WitnessOutC(tx_cap, wit_cap, *(a.ctypes.data for a in (r.tx_begin, r.wit_begin, r.tx_id,
                                                                 r.wit_tx, r.wit_kind, r.wit_ok,
                                                                 r.wit_vk)))
    name = "ouro_block_witness_verify_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n,
                                       ctypes.byref(out), _ptr(r.status), _ptr(r.verdict),
                                       _ptr(r.n_bad))
    _native.check(rc, name)
    r.status, r.verdict, r.n_bad = r.status[:n], r.verdict[:n], r.n_bad[:n]
    r.tx_id, r.wit_tx, r.wit_kind = r.tx_id[:tx_cap], r.wit_tx[:wit_cap], r.wit_kind[:wit_cap]
    r.wit_ok, r.wit_vk = r.wit_ok[:wit_cap], r.wit_vk[:wit_cap]
    return r
