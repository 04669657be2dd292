"""Raw Byron blocks for the whole-block integrity tests (CPU, ASan and GPU), and
what every one of them must give.

Expectations never come from the library: status, counts, bits and root from
byron_block.byron_block_rule / byron_block_counts (the pure-Python restatement
and hashlib), the signature verdict from the oracle's ByronDSIGN verify.

Blocks are built from the parts of the reference's golden Byron block
(tests/golden/reference_blocks.json cardano_disk_Byron_regular): its header
fields, SSC payload and proof, update payload and extra data, around a
txPayload of our own, the proof recomputed from the definition and the header
signed with the oracle under a test key (as pbft_cases.byron_signed signs a
header).

* counts: TX_COUNTS transactions per block, definite and indefinite txPayload,
  both wire forms;
* spans: one transaction of each of TX_LENGTHS bytes, starting at each of the
  four byte alignments of the buffer;
* the golden blocks: the regular one, the EBB, the Shelley-family ones;
* broken: one part broken at a time (BROKEN: kind -> the bits it must clear).
"""
import functools
import hashlib

import numpy as np

import block_cases as BC
import oracle_ffi as O
from hdr_cases import _cbor_head, cbor_bytes, cbor_uint
from ouroboros_network_amd import block as B
from ouroboros_network_amd import byron_block as BB

TX_COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 64, 65, 255, 257]
TX_LENGTHS = [1, 126, 127, 128, 129, 4097]
KEY_SEED = b"\x5b" * 32
GENESIS_XPUB = b"\x17" * 64      # the certificate's issuer: part of the message, not a key we use


def h(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


def arr(*items) -> bytes:
    return _cbor_head(4, len(items)) + b"".join(items)


@functools.lru_cache(maxsize=None)
def golden():
    """the golden Byron blocks: name -> raw"""
    return {b["name"]: bytes.fromhex(b["raw"]) for b in BC.golden()}


@functools.lru_cache(maxsize=None)
def parts():
    """The golden regular block's pieces, as raw CBOR"""
    from ouroboros_network_amd import header as H

    raw = golden()["cardano_disk_Byron_regular"]
    blk = H.array_items(raw, 0)[1]
    hdr, body, extra = H.array_items(raw, blk[0])
    f = H.array_items(raw, hdr[0])
    cons = H.array_items(raw, f[3][0])
    proof = H.array_items(raw, f[2][0])
    pay = H.array_items(raw, body[0])    # (its txPayload is an indefinite list of one element)
    pb = BB.parse_byron_block(raw)
    cut = lambda s: raw[s[0]:s[1]]  # noqa: E731
    span = lambda s: raw[s[0]:s[0] + s[1]]  # noqa: E731
    return dict(magic=cut(f[0]), prev=cut(f[1]), slot=cut(cons[0]), diff=cut(cons[2]),
                hextra=cut(f[4]), ssc_proof=cut(proof[1]), tx=span(pb.txs[0]), wit=span(pb.wits[0]),
                ssc=cut(pay[1]), dlg=cut(pay[2]), upd=cut(pay[3]), extra=cut(extra),
                magic_value=H.uint_at(raw, f[0][0]))


@functools.lru_cache(maxsize=None)
def key():
    pk, sk = O.ed25519_keypair(KEY_SEED)
    return pk + b"\xc7" * 32, sk


def sized_array(total: int, rng) -> bytes:
    """A CBOR array whose encoding is exactly `total` bytes: empty strings,
    then one string that takes the rest"""
    if total == 1:
        return b"\x80"
    for empties in range(3):
        for hw in (1, 2, 3, 5):
            k = total - 1 - empties - hw
            if k >= 0 and len(_cbor_head(2, k)) == hw:
                return bytes([0x81 + empties]) + b"\x40" * empties + cbor_bytes(rng.bytes(k))
    raise ValueError(total)


def make_block(pairs, form=0, indefinite=False, dlg=None, upd=None, tx_num=None, magic=None,
               sign_magic=None):
    """A valid regular block over the (tx, witnesses) pairs: the proof
    recomputed from the definition, the header signed under `sign_magic`
    (default: its own magic field `magic`, default the golden one).
    tx_num: the claimed txpNumber (default: the count).  form 0: on disk,
    1: on the wire."""
    p = parts()
    dlg = p["dlg"] if dlg is None else dlg
    upd = p["upd"] if upd is None else upd
    magic = p["magic_value"] if magic is None else magic
    sign_magic = magic if sign_magic is None else sign_magic
    elems = b"".join(b"\x82" + t + w for t, w in pairs)
    pay = (b"\x9f" + elems + b"\xff") if indefinite else _cbor_head(4, len(pairs)) + elems
    body = b"\x84" + pay + p["ssc"] + dlg + upd
    root = BB.merkle_root([h(b"\x00" + t) for t, _ in pairs])
    wits = h(b"\x9f" + b"".join(w for _, w in pairs) + b"\xff")
    n = len(pairs) if tx_num is None else tx_num
    proof = arr(arr(cbor_uint(n), cbor_bytes(root), cbor_bytes(wits)), p["ssc_proof"],
                cbor_bytes(h(dlg)), cbor_bytes(h(upd)))
    xpub, sk = key()
    msg = (b"01" + GENESIS_XPUB + b"\x09" + cbor_uint(sign_magic) + b"\x85" + p["prev"] + proof +
           p["slot"] + p["diff"] + p["hextra"])
    cert = arr(cbor_uint(0), cbor_bytes(GENESIS_XPUB), cbor_bytes(xpub), cbor_bytes(bytes(64)))
    cons = arr(p["slot"], cbor_bytes(GENESIS_XPUB), p["diff"],
               arr(cbor_uint(2), arr(cert, cbor_bytes(O.ed25519_sign(sk, msg)))))
    header = arr(cbor_uint(magic), p["prev"], proof, cons, p["hextra"])
    blk = b"\x82\x01" + b"\x83" + header + body + p["extra"]
    return b"\xd8\x18" + cbor_bytes(blk) if form else blk


def pairs_of(n, rng, wit_every=3):
    """n transactions of 20 to 90 bytes; the golden witness vector on every
    wit_every-th, an array of random bytes on the others"""
    p = parts()
    return [(sized_array(20 + int(rng.integers(0, 70)), rng),
             p["wit"] if k % wit_every == 0 else sized_array(3 + int(rng.integers(0, 40)), rng))
            for k in range(n)]


def _replace(raw, span, new):
    assert len(new) == span[1]
    return raw[:span[0]] + new + raw[span[0] + span[1]:]


def _flip_in(raw, span):
    """raw with one byte of the span changed so that it slices to the same
    spans (searched from the span's end: payload bytes)"""
    ref = BB.parse_byron_block(raw)
    for pos in range(span[0] + span[1] - 1, span[0] - 1, -1):
        r = bytearray(raw)
        r[pos] ^= 0x04
        try:
            got = BB.parse_byron_block(bytes(r))
        except B.BlockError:
            continue
        if got is not None and (got.txs, got.wits, got.dlg, got.upd) == (ref.txs, ref.wits, ref.dlg,
                                                                          ref.upd):
            return bytes(r)
    raise AssertionError("no shape-keeping flip")


# what each broken kind must clear (BODY_OK goes with each of the five)
BROKEN = {
    "tx_first": BB.BYB_TXROOT_OK, "tx_middle": BB.BYB_TXROOT_OK, "tx_last": BB.BYB_TXROOT_OK,
    "tx_swapped": BB.BYB_TXROOT_OK, "wit_swapped": BB.BYB_TXWIT_OK, "tx_num": BB.BYB_TXNUM_OK,
    "dlg": BB.BYB_DLG_OK, "upd": BB.BYB_UPD_OK, "sig": BB.BYB_HDR_OK, "magic_field": BB.BYB_HDR_OK,
    "magic_signed": BB.BYB_HDR_OK,
}


def must_be(kind):
    """the verdict a broken block of this kind must have under MAGIC"""
    bit = BROKEN[kind]
    body = 0 if bit == BB.BYB_HDR_OK else BB.BYB_BODY_OK
    return BB.BYB_ALL_OK & ~(bit | body)


@functools.lru_cache(maxsize=None)
def broken():
    """[(kind, raw)]: one part broken at a time"""
    rng = np.random.default_rng(606)
    pairs = pairs_of(5, rng, wit_every=2)
    good = make_block(pairs, form=1, dlg=b"\x9f\x01\xff", upd=b"\x82\x80\x81\x05")
    pb = BB.parse_byron_block(good)
    out = [("tx_first", _flip_in(good, pb.txs[0])), ("tx_middle", _flip_in(good, pb.txs[2])),
           ("tx_last", _flip_in(good, pb.txs[4]))]
    # two transactions of one length swapped in place, their witnesses left alone
    same = [(sized_array(40, rng), w) for _, w in pairs]
    g2 = make_block(same, form=0)
    p2 = BB.parse_byron_block(g2)
    cut = lambda r, s: r[s[0]:s[0] + s[1]]  # noqa: E731
    out.append(("tx_swapped", _replace(_replace(g2, p2.txs[1], cut(g2, p2.txs[3])), p2.txs[3],
                                       cut(g2, p2.txs[1]))))
    samew = [(t, sized_array(33, rng)) for t, _ in pairs]
    g3 = make_block(samew, form=0, indefinite=True)
    p3 = BB.parse_byron_block(g3)
    out.append(("wit_swapped", _replace(_replace(g3, p3.wits[0], cut(g3, p3.wits[4])), p3.wits[4],
                                        cut(g3, p3.wits[0]))))
    out.append(("tx_num", make_block(pairs, form=1, tx_num=6)))
    out.append(("dlg", _replace(good, pb.dlg, b"\x9f\x02\xff")))
    out.append(("upd", _replace(good, pb.upd, b"\x82\x80\x81\x06")))
    r = bytearray(good)
    r[good.index(pb.sig) + 9] ^= 0x04
    out.append(("sig", bytes(r)))
    m = parts()["magic_value"]
    # the magic field is the one header field the signature does not cover
    out.append(("magic_field", make_block(pairs, magic=m + 1, sign_magic=m)))
    out.append(("magic_signed", make_block(pairs, magic=m + 1)))
    return out


def expect(raw, magic):
    """(status, verdict, tx_root) one block must give"""
    return BB.byron_block_rule(raw, magic, O.ed25519_verify_byron)


def expected_arrays(raws, magic):
    exp = [expect(r, magic) for r in raws]
    cnt = [BB.byron_block_counts(r, magic) for r in raws]
    return dict(status=np.array([e[0] for e in exp], np.uint8),
                verdict=np.array([e[1] for e in exp], np.uint8),
                tx_root=np.frombuffer(b"".join(e[2] for e in exp),
                                      np.uint8).reshape(-1, 32).copy(),   # (writable)
                ntx=np.array([c[1] for c in cnt], np.uint32),
                gather=np.array([c[2] for c in cnt], np.uint32),
                msg=np.array([c[3] for c in cnt], np.uint32))


def layout(raws, aligns=None):
    """(buf, off, len): the blocks in one buffer, a block with a wanted
    alignment padded so that its first transaction starts there"""
    parts_, off, at = [], [], 0
    for k, raw in enumerate(raws):
        pad = 0
        if aligns is not None and aligns[k] is not None:
            pad = (aligns[k] - (at + BB.parse_byron_block(raw).txs[0][0])) % 4
        parts_ += [bytes(pad), raw]
        off.append(at + pad)
        at += pad + len(raw)
    return (np.frombuffer(b"".join(parts_) + b"\x00", np.uint8), np.array(off, np.uint64),
            np.array([len(r) for r in raws], np.uint32))


@functools.lru_cache(maxsize=None)
def case_set():
    """The whole set in one buffer, with the expected arrays under the golden
    network's magic.  Computed once and shared."""
    rng = np.random.default_rng(605)
    p = parts()
    raws, kinds, aligns = [], [], []

    def add(raw, kind, align=None):
        raws.append(raw)
        kinds.append(kind)
        aligns.append(align)

    for k, n in enumerate(TX_COUNTS):
        add(make_block(pairs_of(n, rng), form=k % 2, indefinite=bool((k // 2) % 2)), "count")
    for li, n in enumerate(TX_LENGTHS):
        for a in range(4):
            wit = p["wit"] if (li + a) % 2 else b"\x80"
            add(make_block([(sized_array(n, rng), wit)], form=(li + a) % 2, indefinite=bool(a & 1)),
                "span", a)
    for name, raw in golden().items():
        add(raw, "golden_byron" if "Byron" in name else "golden_shelley")
    for kind, raw in broken():
        add(raw, kind)
    exp = expected_arrays(raws, p["magic_value"])
    return dict(raws=raws, kinds=kinds, aligns=aligns, triple=layout(raws, aligns),
                magic=p["magic_value"], **exp)


def golden_flips():
    """every single-byte ^0x04 flip of the golden regular block (on disk)"""
    raw = golden()["cardano_disk_Byron_regular"]
    out = []
    for pos in range(len(raw)):
        r = bytearray(raw)
        r[pos] ^= 0x04
        out.append(bytes(r))
    return out


def golden_truncations():
    raw = golden()["cardano_n2n_Byron_regular"]
    return [raw[:cut] for cut in range(len(raw))]
