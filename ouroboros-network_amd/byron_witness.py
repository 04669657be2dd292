"""Byron transaction witnesses from raw block CBOR: the tx ids and the
ByronDSIGN verification of every witness over its transaction's signed message.

This file DEFINES the rule; csrc/cbor_byron_witness.h mirrors
it item for item, and the tests take their expectations from here, from hashlib
and from the oracle's ByronDSIGN verify, never from the library.

* ``parse_byron_witnesses``: the walker -- byron_block.parse_byron_block (whose
  acceptance everything outside the witness vectors keeps, status for status)
  with a visitor that reads every witness vector;
* ``byron_witness_message``: the bytes a witness signs;
* ``byron_witness_rule``: status, verdict, n_bad, tx ids and rows of one block;
* ``count_byron_block_witnesses``: ouro_byron_block_witness_count_cbor[_host];
* ``verify_byron_block_witnesses``: ouro_byron_block_witness_verify_cbor[_host].

The rule.  A block is one of byron_block.py's two forms; tag 0 is PACK_EBB
(verdict BYW_ALL_OK, no rows), tag >= 2 PACK_ESHELLEY.  Every element of the
txPayload is [tx, witnesses]:
    witnesses = [* [type: uint, #6.24(bytes .cbor [key: bytes, sig: bytes])]]
                definite or indefinite; each element a definite array(2); the
                tag-24 payload a definite byte string whose content is a
                definite array(2) of two definite byte strings and ends exactly
                at the payload's end
    type 0 (VKWitness):      key bytes(64) (an XPub), sig bytes(64)
    type 2 (RedeemWitness):  key bytes(32),           sig bytes(64)
Any other type, major type, tag or array length is PACK_ESHAPE for the block; a
payload whose content is malformed inside it or does not end at its end is
PACK_ECBOR; a wrong string length PACK_ESIZE -- per witness the content is
walked first, then the two types, then the two sizes.  The status is that of
the first offending item in byte order; malformed CBOR anywhere inside a
[tx, witnesses] element is found by the outer walk before the element's
witness vector is read.  A block that does not slice owns no rows.

tx id = Blake2b-256 of the tx item's bytes as they stand (no prefix byte: not
the Merkle leaf).  The signed message is
    tag || CBOR(magic) || 0x58 0x20 || tx_id
with tag 0x01 (SignTx) for type 0 and 0x02 (SignRedeemTx) for type 2, and magic
the configured ProtocolMagicId or the header's own field (mainnet, type 0:
01 1a 2d 96 4a 09 58 20).  Both kinds verify under ByronDSIGN acceptance: type
0 under XPub[0:32], type 2 under the 32-byte redeem key.

Pinned by the reference's golden Byron block: the witness vector's shape
(81 82 00 d8 18 58 85 82 58 40 <64> 58 40 <64>).  NOT pinned by any reference
fixture (restated from cardano-ledger's Cardano.Chain.UTxO.TxWitness and
Cardano.Crypto.Signing.Tag; the reference only names SignTx, at
Byron/Crypto/DSIGN.hs:59): the signed message (the tag bytes and the 58 20
wrapped id), that the tx id hashes the bytes as they stand, that the redeem
kind uses ByronDSIGN's acceptance rules, that an unknown witness type fails the
block's decode.  The golden GenTxId_Byron is the example's input id, not this
transaction's, and pins nothing here.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _native
from .block import BlockError, _fail, _head, _skip
from .byron import PACK_EBB, PACK_ESHELLEY, _magic_arg, cbor_uint  # noqa: F401
from .byron_block import parse_byron_block
from .header import (PACK_ECBOR, PACK_ESHAPE, PACK_ESIZE, PACK_ESPAN, PACK_OK,  # noqa: F401
                     raw_triplet)
from .witness import PACK_ECAP, _walk  # noqa: F401

BYW_ALL_OK = 0x01          # OURO_BYW_ALL_OK
KIND_VK, KIND_REDEEM = 0, 2
SIGN_TAG = {KIND_VK: b"\x01", KIND_REDEEM: b"\x02"}    # SignTx, SignRedeemTx
KEY_BYTES = {KIND_VK: 64, KIND_REDEEM: 32}


@dataclass
class ByronWitness:
    tx: int          # index of its transaction within the block
    kind: int        # 0: VKWitness; 2: RedeemWitness
    key: bytes       # the XPub (64 bytes) or the redeem key (32)
    sig: bytes

    @property
    def vk64(self) -> bytes:
        """the wit_vk row: the key, a redeem key followed by 32 zero bytes"""
        return self.key + bytes(64 - len(self.key))


@dataclass
class ByronBlockWitnesses:
    magic: int                          # the header's protocolMagic field
    tx_spans: List[Tuple[int, int]]     # (offset, length) of every tx
    witnesses: List[ByronWitness]

    def tx_ids(self, raw: bytes) -> List[bytes]:
        return [hashlib.blake2b(raw[o:o + n], digest_size=32).digest() for o, n in self.tx_spans]


def _definite_bytes(buf, i, end):
    """(content start, length) of the definite byte string at i, or None (another type)"""
    mt, arg, j = _head(buf, i, end)
    return None if mt != 2 or arg is None else (j, arg)


def _read_vector(buf: bytes, span: Tuple[int, int], t: int, out: List[ByronWitness]) -> None:
    """The witness vector at `span` (well-formed CBOR, an array: the outer walk
    has been over it) of the block's t-th transaction."""
    end = span[0] + span[1]
    _, count, first = _head(buf, span[0], end)

    def one(at):
        mt, arg, i = _head(buf, at, end)
        if mt != 4 or arg != 2:
            _fail(PACK_ESHAPE, "a witness is a definite array(2)")
        mt, kind, i = _head(buf, i, end)
        if mt != 0 or kind is None:
            _fail(PACK_ESHAPE, "a witness type is a uint")
        if kind not in KEY_BYTES:
            _fail(PACK_ESHAPE, "unknown witness type")
        mt, arg, i = _head(buf, i, end)
        if mt != 6 or arg != 24:
            _fail(PACK_ESHAPE, "expected tag 24")
        pay = _definite_bytes(buf, i, end)
        if pay is None:
            _fail(PACK_ESHAPE, "expected definite CBOR-in-bytes")
        p0, pe = pay[0], pay[0] + pay[1]          # the payload bounds its content
        mt, arg, i = _head(buf, p0, pe)
        if mt != 4 or arg != 2:
            _fail(PACK_ESHAPE, "the payload is a definite array(2)")
        # walked first, then the types, then the sizes
        k0 = i
        k1 = _skip(buf, k0, pe)
        if _skip(buf, k1, pe) != pe:
            _fail(PACK_ECBOR, "the payload's content does not end at its end")
        got = [_definite_bytes(buf, k0, pe), _definite_bytes(buf, k1, pe)]
        if any(g is None for g in got):
            _fail(PACK_ESHAPE, "expected two byte strings")
        if [g[1] for g in got] != [KEY_BYTES[kind], 64]:
            _fail(PACK_ESIZE, "a key or signature of the wrong length")
        out.append(ByronWitness(t, kind, *(bytes(buf[s:s + n]) for s, n in got)))
        return pe

    _walk(buf, first, end, count, one)


def parse_byron_witnesses(raw: bytes) -> Optional[ByronBlockWitnesses]:
    """Slice one block: its tx spans and witnesses, or None for an EBB; raises
    BlockError(status) where the C walker rejects.  The first offending item in
    byte order decides: an error inside a witness vector comes before whatever
    the outer walk meets after that element."""
    buf = bytes(raw)
    wits: List[ByronWitness] = []
    first: List[BlockError] = []

    def visit(k, _tx, wit):
        if first:
            return
        try:
            _read_vector(buf, wit, k, wits)
        except BlockError as e:
            e.in_vector = True      # (the tests tell the two sources apart)
            first.append(e)

    try:
        b = parse_byron_block(buf, visit)
    except BlockError:
        if first:
            raise first[0]
        raise
    if first:
        raise first[0]
    if b is None:
        return None
    return ByronBlockWitnesses(b.magic, b.txs, wits)


def byron_witness_status(raw: bytes) -> int:
    """OURO_PACK_* as the walker reports it"""
    try:
        return PACK_EBB if parse_byron_witnesses(raw) is None else PACK_OK
    except BlockError as e:
        return e.status


def byron_witness_error_in_vector(raw: bytes) -> bool:
    """Whether the block's status comes from inside a witness vector (else it
    is byron_block.parse_byron_block's own)"""
    try:
        parse_byron_witnesses(raw)
    except BlockError as e:
        return getattr(e, "in_vector", False)
    return False


def byron_witness_counts(raw: bytes) -> Tuple[int, int, int]:
    """(status, ntx, nwit) of the count pass: zeros unless the status is PACK_OK"""
    try:
        b = parse_byron_witnesses(raw)
    except BlockError as e:
        return e.status, 0, 0
    if b is None:
        return PACK_EBB, 0, 0
    return PACK_OK, len(b.tx_spans), len(b.witnesses)


def byron_witness_message(magic: int, kind: int, tx_id: bytes) -> bytes:
    """What a witness of `kind` signs: signTag || serialize' (a 32-byte hash)"""
    if len(tx_id) != 32:
        raise ValueError("a tx id has 32 bytes")
    return SIGN_TAG[kind] + cbor_uint(magic) + b"\x58\x20" + tx_id


def byron_witness_rule(raw: bytes, protocol_magic,
                       verify: Callable[[bytes, bytes, bytes], bool]):
    """(status, verdict, n_bad, tx_ids, rows) one block must give; rows:
    (tx, kind, vk64, ok) per witness.  verify(sig, message, key32): ByronDSIGN
    acceptance (the tests pass the oracle's)."""
    magic = _magic_arg(protocol_magic)
    try:
        b = parse_byron_witnesses(raw)
    except BlockError as e:
        return e.status, 0, 0, [], []
    if b is None:
        return PACK_EBB, BYW_ALL_OK, 0, [], []
    m = b.magic if magic < 0 else magic
    ids = b.tx_ids(raw)
    rows = [(w.tx, w.kind, w.vk64,
             bool(verify(w.sig, byron_witness_message(m, w.kind, ids[w.tx]), w.key[:32])))
            for w in b.witnesses]
    bad = sum(1 for r in rows if not r[3])
    return PACK_OK, (BYW_ALL_OK if bad == 0 else 0), bad, ids, rows


class ByronWitnessOutC(ctypes.Structure):
    """Mirror of ``ouro_byron_block_witness_out`` (include/ouro_verify.h)."""

    _fields_ = [("tx_cap", ctypes.c_size_t), ("wit_cap", ctypes.c_size_t)] + [
        (f, ctypes.c_void_p) for f in ("tx_begin", "wit_begin", "tx_id", "wit_tx", "wit_kind",
                                       "wit_ok", "wit_vk")]


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def count_byron_block_witnesses(raws, protocol_magic, host: bool = False):
    """The walker's count pass: (status, ntx, nwit) per block, zeros unless the
    status is PACK_OK.  raws: a sequence of bytes or a (buf, off, len) triple."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    status = np.zeros(max(n, 1), np.uint8)
    ntx = np.zeros(max(n, 1), np.uint32)
    nwit = np.zeros(max(n, 1), np.uint32)
    name = "ouro_byron_block_witness_count_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n,
                                       _magic_arg(protocol_magic), _ptr(status), _ptr(ntx),
                                       _ptr(nwit))
    _native.check(rc, name)
    return status[:n], ntx[:n], nwit[:n]


@dataclass
class ByronWitnessResult:
    status: np.ndarray       # n: PACK_*
    verdict: np.ndarray      # n: BYW_ALL_OK or 0
    n_bad: np.ndarray        # n: the block's witnesses that do not verify
    tx_begin: np.ndarray     # n + 1: block i owns the tx rows [tx_begin[i], tx_begin[i + 1])
    wit_begin: np.ndarray    # n + 1
    tx_id: np.ndarray        # tx_cap x 32
    wit_tx: np.ndarray       # wit_cap: the witness's global tx row
    wit_kind: np.ndarray     # wit_cap: 0 or 2
    wit_ok: np.ndarray       # wit_cap: 1 = verifies
    wit_vk: np.ndarray       # wit_cap x 64: the XPub; a redeem key then 32 zero bytes


def verify_byron_block_witnesses(raws, protocol_magic, tx_cap: int = None, wit_cap: int = None,
                                 host: bool = False) -> ByronWitnessResult:
    """Every witness of every Byron block verified over its transaction's
    signed message: a ByronWitnessResult.  protocol_magic: the node's
    ProtocolMagicId, or byron.HEADER_MAGIC for each header's own field.
    tx_cap / wit_cap: the row capacities (default: what the count pass finds);
    a sliced block whose rows pass one has status PACK_ECAP and writes nothing.
    host=True: the host path alone, no device touched."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    if ln.size != n:
        raise ValueError("off / len: one entry per block")
    if tx_cap is None or wit_cap is None:
        _, ntx, nwit = count_byron_block_witnesses((buf, off, ln), protocol_magic, host=host)
        tx_cap = int(ntx.sum()) if tx_cap is None else tx_cap
        wit_cap = int(nwit.sum()) if wit_cap is None else wit_cap
    r = ByronWitnessResult(
        status=np.zeros(max(n, 1), np.uint8), verdict=np.zeros(max(n, 1), np.uint8),
        n_bad=np.zeros(max(n, 1), np.uint32), tx_begin=np.zeros(n + 1, np.uint64),
        wit_begin=np.zeros(n + 1, np.uint64), tx_id=np.zeros((max(tx_cap, 1), 32), np.uint8),
        wit_tx=np.zeros(max(wit_cap, 1), np.uint32), wit_kind=np.zeros(max(wit_cap, 1), np.uint8),
        wit_ok=np.zeros(max(wit_cap, 1), np.uint8),
        wit_vk=np.zeros((max(wit_cap, 1), 64), np.uint8))
    out = ByronWitnessOutC(tx_cap, wit_cap, *(a.ctypes.data for a in (
        r.tx_begin, r.wit_begin, r.tx_id, r.wit_tx, r.wit_kind, r.wit_ok, r.wit_vk)))
    name = "ouro_byron_block_witness_verify_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n,
                                       _magic_arg(protocol_magic), ctypes.byref(out),
                                       _ptr(r.status), _ptr(r.verdict), _ptr(r.n_bad))
    _native.check(rc, name)
    r.status, r.verdict, r.n_bad = r.status[:n], r.verdict[:n], r.n_bad[:n]
    r.tx_id, r.wit_tx, r.wit_kind = r.tx_id[:tx_cap], r.wit_tx[:wit_cap], r.wit_kind[:wit_cap]
    r.wit_ok, r.wit_vk = r.wit_ok[:wit_cap], r.wit_vk[:wit_cap]
    return r
