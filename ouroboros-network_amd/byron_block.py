"""Byron whole-block storage integrity (verifyBlockIntegrity) from raw block
CBOR: the block signature and the body proof.

* ``parse_byron_block``: a pure-Python restatement of the Byron block slicer
  (csrc/cbor_byron_block.h), written independently of it the way
  block.parse_block stands beside csrc/cbor_block.h; the tests take their
  expectations from it, from hashlib and from the oracle's ByronDSIGN verify,
  never from the library;
* ``merkle_root``: the Merkle root written recursively from its definition
  (``merkle_root_levels`` is the level-by-level form the device uses);
* ``byron_block_rule``: status, OURO_BYB_* bits and root one block must give;
* ``verify_byron_block_integrity``: ouro_byron_block_integrity_verify_cbor[_host]
  (include/ouro_verify.h);
* ``count_byron_blocks``: ouro_byron_block_count_cbor[_host].

The rule.  verifyBlockIntegrity cfg blk = verifyHeaderIntegrity
cfg hdr && blockMatchesHeader hdr blk (ouroboros-consensus-byron/src/Ouroboros/
Consensus/Byron/Ledger/Integrity.hs:63-68).  Block forms:
    [tag, block]                         on disk
    #6.24(bytes .cbor [tag, block])      on the wire
tag 0 = EBB (PACK_EBB: nothing is checked), 1 = regular, 2 and up = Shelley
family (PACK_ESHELLEY).
    regular = [header, body, extra]              definite array(3), ends at its span
    header  = [magic, prevHash, proof, consensusData, extraData]
    proof   = [[txpNumber, txpRoot, txpWitnessesHash], [sscTag, sscHash], dlgHash, updHash]
    body    = [txPayload, sscPayload, dlgPayload, updPayload]      definite array(4)
    txPayload = [* [tx, witnesses]]   definite or indefinite; elements definite
                array(2) of two arrays, recorded as they stand
Every hash is Blake2b-256 over bytes as they stand in the block:
    leaf_k = H(0x00 || tx_k); node(l, r) = H(0x01 || l || r); the root of n
    leaves is H("") for n = 0, the leaf for n = 1, else node(root(first i),
    root(rest)) with i the largest power of two strictly below n;
    txpWitnessesHash = H(0x9f || witnesses_0 || ... || 0xff);
    dlgHash = H(dlgPayload); updHash = H(updPayload); txpNumber = n.
The SSC proof is not compared (the reference's SscProof is a unit).
Pinned by the reference's golden Byron block: the leaf form, the witnesses list
form and the two payload hashes.  NOT pinned by a reference fixture: the tree
shape for n >= 2 and the empty root (restated from cardano-ledger's
Cardano.Chain.Common.Merkle), non-canonical or indefinite encodings inside a
witness vector (hashed here as they stand), that the SSC proof's content is
ignored.  The transaction witnesses are not verified here: byron_witness.py
 verifies them.
"""
from __future__ import annotations

import ctypes
import hashlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _native
from .block import BlockError, _array_items, _bytes_at, _fail, _head, _skip, _uint_at
from .byron import PACK_EBB, PACK_ESHELLEY, WORD32_MAX, _magic_arg, cbor_uint
from .header import (PACK_ECBOR, PACK_ESHAPE, PACK_ESIZE, PACK_ESPAN, PACK_OK,  # noqa: F401
                     raw_triplet)
from .witness import PACK_ECAP, _open, _walk  # noqa: F401

BYB_HDR_OK = 0x01      # verifyHeaderIntegrity
BYB_BODY_OK = 0x02     # blockMatchesHeader: all five below
BYB_TXNUM_OK = 0x04
BYB_TXROOT_OK = 0x08
BYB_TXWIT_OK = 0x10
BYB_DLG_OK = 0x20
BYB_UPD_OK = 0x40
BYB_ALL_OK = 0x7F
_FIVE = BYB_TXNUM_OK | BYB_TXROOT_OK | BYB_TXWIT_OK | BYB_DLG_OK | BYB_UPD_OK


def _h(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


def merkle_root(leaves: List[bytes]) -> bytes:
    """The root of the leaf digests, recursively from the definition."""
    n = len(leaves)
    if n == 0:
        return _h(b"")
    if n == 1:
        return leaves[0]
    i = 1
    while 2 * i < n:
        i *= 2
    return _h(b"\x01" + merkle_root(leaves[:i]) + merkle_root(leaves[i:]))


def merkle_root_levels(leaves: List[bytes]) -> bytes:
    """The same root level by level: pair neighbours, carry an odd last node up
    unchanged (the form csrc/cbor_byron_block.h byron_merkle_root runs)."""
    if not leaves:
        return _h(b"")
    row = list(leaves)
    while len(row) > 1:
        nxt = [_h(b"\x01" + row[k] + row[k + 1]) for k in range(0, len(row) - 1, 2)]
        if len(row) & 1:
            nxt.append(row[-1])
        row = nxt
    return row[0]


@dataclass
class ByronBlock:
    """A regular Byron block as the slicer records it (offsets into the raw block)."""
    magic: int                       # the header's protocolMagic field
    issuer_xpub: bytes               # the delegation certificate's issuer (the genesis key)
    delegate_xpub: bytes             # the signing key
    sig: bytes
    to_sign: bytes                   # 0x85 || prevHash || proof || slotId || difficulty || extra
    tx_num: int                      # the proof's txpNumber
    claimed: Tuple[bytes, bytes, bytes, bytes]   # txpRoot, txpWitnessesHash, dlgHash, updHash
    txs: List[Tuple[int, int]]       # (offset, length) of every tx
    wits: List[Tuple[int, int]]      # ... and of every witness vector
    dlg: Tuple[int, int]
    upd: Tuple[int, int]

    def message(self, magic: int) -> bytes:
        """The signed message under `magic` (-1: the header's own field)"""
        m = self.magic if magic < 0 else magic
        return b"01" + self.issuer_xpub + b"\x09" + cbor_uint(m) + self.to_sign

    def gathered(self, raw: bytes) -> bytes:
        return b"\x9f" + b"".join(raw[o:o + n] for o, n in self.wits) + b"\xff"

    def proof(self, raw: bytes) -> Tuple[bytes, bytes, bytes, bytes]:
        """(root, witnesses hash, dlg hash, upd hash) recomputed from the body"""
        cut = lambda s: raw[s[0]:s[0] + s[1]]  # noqa: E731
        return (merkle_root([_h(b"\x00" + cut(t)) for t in self.txs]), _h(self.gathered(raw)),
                _h(cut(self.dlg)), _h(cut(self.upd)))


def _fixed(buf, i, end, want):
    """A definite array of exactly `want` items (cbor_byron.h fixed_array)"""
    items = _array_items(buf, i, end, want)
    if items is None or len(items) != want:
        _fail(PACK_ESHAPE, f"expected {want} items at {i}")
    return items


def _sized(buf, end, starts, want, what):
    """The definite byte strings at `starts`, each of `want` bytes: any wrong
    type is PACK_ESHAPE, then any wrong size PACK_ESIZE"""
    got = [_bytes_at(buf, s, end) for s in starts]
    if any(g is None for g in got):
        _fail(PACK_ESHAPE, what + ": expected bytes")
    if any(len(g) != want for g in got):
        _fail(PACK_ESIZE, what + f": expected {want} bytes")
    return got


def parse_byron_block(raw: bytes, visit=None) -> Optional[ByronBlock]:
    """Slice one block: a ByronBlock, or None for an EBB; raises
    BlockError(status) where the C walker rejects.  visit(k, tx, wit): called
    for the k-th [tx, witnesses] element once the walk has accepted it, with the
    two (offset, length) spans -- the walker's visitor (byron_witness.py)."""
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
    if mt != 4 or arg != 2:
        _fail(PACK_ESHAPE, "expected [tag, block]")
    tag = _uint_at(buf, j, end)
    if tag >= 2:
        _fail(PACK_ESHELLEY, "a Shelley-family block")
    pos = _skip(buf, j, end)
    if tag == 0:
        if _skip(buf, pos, end) != end:
            _fail(PACK_ECBOR, "bytes after the block")
        return None
    mt, arg, h = _head(buf, pos, end)
    if mt != 4 or arg != 3:
        _fail(PACK_ESHAPE, "a regular block has 3 items")
    # item 0: the header
    f = _fixed(buf, h, end, 5)
    magic = _uint_at(buf, f[0][0], end)
    if magic > WORD32_MAX:
        _fail(PACK_ESHAPE, "protocol magic: Word32")
    cons = _fixed(buf, f[3][0], end, 4)
    bsig = _fixed(buf, cons[3][0], end, 2)
    if _uint_at(buf, bsig[0][0], end) != 2:
        _fail(PACK_ESHAPE, "block signature kind (only delegated, 2)")
    inner = _fixed(buf, bsig[1][0], end, 2)
    cert = _fixed(buf, inner[0][0], end, 4)
    gvk, dvk, sig = _sized(buf, end, [cert[1][0], cert[2][0], inner[1][0]], 64, "key / signature")
    cut = lambda it: buf[it[0]:it[1]]  # noqa: E731
    to_sign = b"\x85" + cut(f[1]) + cut(f[2]) + cut(cons[0]) + cut(cons[2]) + cut(f[4])
    # ... its proof
    p = _fixed(buf, f[2][0], end, 4)
    t = _fixed(buf, p[0][0], end, 3)
    s = _fixed(buf, p[1][0], end, 2)
    tx_num = _uint_at(buf, t[0][0], end)
    if tx_num > WORD32_MAX:
        _fail(PACK_ESHAPE, "txpNumber: Word32")
    _uint_at(buf, s[0][0], end)
    root, wit, _ssc, dlg, upd = _sized(buf, end, [t[1][0], t[2][0], s[1][0], p[2][0], p[3][0]], 32,
                                       "proof hash")
    # item 1: the body
    mt, arg, j = _head(buf, f[4][1], end)
    if mt != 4 or arg != 4:
        _fail(PACK_ESHAPE, "a body has 4 items")
    txs, wits = [], []

    def elem(at):
        mt, arg, a = _head(buf, at, end)
        if mt != 4 or arg != 2:
            _fail(PACK_ESHAPE, "a txPayload element is a definite array(2)")
        spans = []
        for _ in range(2):
            m1, _, _ = _head(buf, a, end)
            if m1 != 4:
                _fail(PACK_ESHAPE, "tx and witnesses are arrays")
            e = _skip(buf, a, end)
            spans.append((a, e - a))
            a = e
        if visit is not None:
            visit(len(txs), spans[0], spans[1])
        txs.append(spans[0])
        wits.append(spans[1])
        return a

    count, first = _open(buf, j, end, 4)
    i = _walk(buf, first, end, count, elem)
    i = _skip(buf, i, end)                       # sscPayload
    segs = []
    for _ in range(2):                           # dlgPayload, updPayload
        e = _skip(buf, i, end)
        segs.append((i, e - i))
        i = e
    i = _skip(buf, i, end)                       # item 2: the extra data
    if i != end:
        _fail(PACK_ECBOR, "bytes after the block")
    return ByronBlock(magic=magic, issuer_xpub=gvk, delegate_xpub=dvk, sig=sig, to_sign=to_sign,
                      tx_num=tx_num, claimed=(root, wit, dlg, upd), txs=txs, wits=wits,
                      dlg=segs[0], upd=segs[1])


def byron_block_status(raw: bytes) -> int:
    """OURO_PACK_* as the walker reports it"""
    try:
        return PACK_EBB if parse_byron_block(raw) is None else PACK_OK
    except BlockError as e:
        return e.status


def byron_block_counts(raw: bytes, protocol_magic) -> Tuple[int, int, int, int]:
    """(status, ntx, gathered witness bytes, message bytes) of the count pass"""
    try:
        b = parse_byron_block(raw)
    except BlockError as e:
        return e.status, 0, 0, 0
    if b is None:
        return PACK_EBB, 0, 0, 0
    return (PACK_OK, len(b.txs), sum(n for _, n in b.wits) + 2,
            len(b.message(_magic_arg(protocol_magic))))


def byron_block_rule(raw: bytes, protocol_magic,
                     verify: Callable[[bytes, bytes, bytes], bool]) -> Tuple[int, int, bytes]:
    """(status, OURO_BYB_* bits, Merkle root) one block must give.
    verify(sig, message, key32): ByronDSIGN acceptance (the tests pass the
    oracle's)."""
    magic = _magic_arg(protocol_magic)
    try:
        b = parse_byron_block(raw)
    except BlockError as e:
        return e.status, 0, bytes(32)
    if b is None:
        return PACK_EBB, BYB_ALL_OK, bytes(32)
    got = b.proof(raw)
    v = BYB_TXNUM_OK if b.tx_num == len(b.txs) else 0
    for bit, x, y in zip((BYB_TXROOT_OK, BYB_TXWIT_OK, BYB_DLG_OK, BYB_UPD_OK), b.claimed, got):
        if x == y:
            v |= bit
    if v & _FIVE == _FIVE:
        v |= BYB_BODY_OK
    if verify(b.sig, b.message(magic), b.delegate_xpub[:32]) and (magic < 0 or b.magic == magic):
        v |= BYB_HDR_OK
    return PACK_OK, v, got[0]


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def count_byron_blocks(raws, protocol_magic, host: bool = False):
    """The slicer's count pass: (status, ntx, gather_bytes, msg_bytes, totals),
    zeros unless a block's status is PACK_OK; totals: the three sums.  raws: a
    sequence of bytes or a (buf, off, len) triple."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    status = np.zeros(max(n, 1), np.uint8)
    cnt = [np.zeros(max(n, 1), np.uint32) for _ in range(3)]
    totals = np.zeros(3, np.uint64)
    name = "ouro_byron_block_count_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n,
                                       _magic_arg(protocol_magic), _ptr(status), _ptr(cnt[0]),
                                       _ptr(cnt[1]), _ptr(cnt[2]), _ptr(totals))
    _native.check(rc, name)
    return status[:n], cnt[0][:n], cnt[1][:n], cnt[2][:n], totals


def verify_byron_block_integrity(raws, protocol_magic, host: bool = False):
    """verifyBlockIntegrity over raw Byron blocks: (verdict, status, tx_root) --
    BYB_* bits per block (0 for one that does not slice, BYB_ALL_OK for an
    EBB), PACK_* per block, and the computed Merkle root (n x 32; zeros unless
    the status is PACK_OK).  protocol_magic: the node's ProtocolMagicId, or
    byron.HEADER_MAGIC for each header's own field.  host=True: the host path
    alone, no device touched."""
    buf, off, ln = raw_triplet(raws)
    n = int(off.size)
    if ln.size != n:
        raise ValueError("off / len: one entry per block")
    status = np.zeros(max(n, 1), np.uint8)
    verdict = np.zeros(max(n, 1), np.uint8)
    tx_root = np.zeros((max(n, 1), 32), np.uint8)
    name = "ouro_byron_block_integrity_verify_cbor" + ("_host" if host else "")
    rc = getattr(_native.load(), name)(_ptr(buf), buf.size, _ptr(off), _ptr(ln), n,
                                       _magic_arg(protocol_magic), _ptr(status), _ptr(verdict),
                                       _ptr(tx_root))
    _native.check(rc, name)
    return verdict[:n], status[:n], tx_root[:n]
