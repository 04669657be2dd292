"""Raw blocks for the transaction-witness tests (CPU and GPU), and what every
one of them must give.

Expectations never come from the library: the status and the rows from
witness.parse_witnesses (the pure-Python restatement), the tx ids from
hashlib, the witness verdicts from the oracle's ed25519_verify.

A block is the golden Shelley header's bytes (reused unsigned: the walker
skips item 0) followed by generated txBodies, txWitnesses and an empty
metadata map, in all four block encodings.  Tx bodies are maps of the encoded
lengths BODY_LENGTHS, the first body of a block starting at each of the four
byte alignments of the buffer; witnesses are signed with the oracle's Ed25519
signer over the real tx id.

* valid(): 0 transactions; empty witness map; key 0 as an empty array; 1, 2,
  63, 64, 65 witnesses; key 2 alone and both keys; an unknown key (1, a nested
  array) before, between and after; a repeated key 0; indefinite txBodies,
  txWitnesses, witness sets and witness arrays;
* invalid(): [(raw, n_bad)] -- one bit flipped in a sig, a vkey or a tx body;
  a witness moved to another transaction; the Ed25519 acceptance corners of
  edge_cases.py placed as witnesses;
* malformed(): [(raw, status)].
"""
import functools
import hashlib

import numpy as np

import edge_cases as E
import oracle_ffi as O
from block_cases import golden, wrap
from hdr_cases import _cbor_head, cbor_bytes
from ouroboros_network_amd import block as B
from ouroboros_network_amd import witness as W

BODY_LENGTHS = [1, 127, 128, 129, 4097]
WIT_COUNTS = [None, 0, 1, 2, 63, 64, 65]     # None: an empty witness map


def b2b(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


@functools.lru_cache(maxsize=None)
def header_bytes() -> bytes:
    raw = bytes.fromhex(golden()[0]["raw"])   # Shelley on disk: a bare array(4)
    assert raw[0] == 0x84
    return raw[1:B._skip(raw, 1, len(raw))]


def arr(items, indef=False) -> bytes:
    items = list(items)
    if indef:
        return b"\x9f" + b"".join(items) + b"\xff"
    return _cbor_head(4, len(items)) + b"".join(items)


def cmap(pairs, indef=False) -> bytes:
    """pairs: [(encoded key, encoded value)]"""
    body = b"".join(k + v for k, v in pairs)
    return (b"\xbf" + body + b"\xff") if indef else _cbor_head(5, len(pairs)) + body


def uint(k: int) -> bytes:
    return _cbor_head(0, k)


def tx_body(total: int, rng) -> bytes:
    """A map whose encoding is exactly `total` bytes: {0: bytes}"""
    if total == 1:
        return b"\xa0"
    for hw in (1, 2, 3, 5):
        k = total - 2 - hw
        if k >= 0 and len(_cbor_head(2, k)) == hw:
            return b"\xa1\x00" + cbor_bytes(rng.bytes(k))
    raise ValueError(total)


@functools.lru_cache(maxsize=None)
def keypair(k: int):
    return O.ed25519_keypair(hashlib.sha256(b"witness key %d" % k).digest())


def vkey_wit(k: int, txid: bytes) -> bytes:
    pk, sk = keypair(k)
    return arr([cbor_bytes(pk), cbor_bytes(O.ed25519_sign(sk, txid))])


def boot_wit(k: int, txid: bytes, rng) -> bytes:
    pk, sk = keypair(k)
    return arr([cbor_bytes(pk), cbor_bytes(O.ed25519_sign(sk, txid)), cbor_bytes(rng.bytes(32)),
                cbor_bytes(rng.bytes(int(rng.integers(0, 40))))])


def pair_wit(pk: bytes, sig: bytes) -> bytes:
    return arr([cbor_bytes(pk), cbor_bytes(sig)])


UNKNOWN = (uint(1), arr([arr([cbor_bytes(b"script"), uint(7)]), arr([])]))


def make_block(bodies, wsets, form=0, tag=2, indef_bodies=False, indef_sets=False) -> bytes:
    return wrap(b"\x84" + header_bytes() + arr(bodies, indef_bodies) + arr(wsets, indef_sets)
                + b"\xa0", form, tag)


def first_body_offset(raw: bytes) -> int:
    return W.parse_witnesses(raw).tx_spans[0][0]


@functools.lru_cache(maxsize=None)
def valid():
    """[(raw block, wanted alignment of its first tx body in the buffer, or None)]"""
    rng = np.random.default_rng(41)
    out = [(make_block([], [], form=f), None) for f in range(4)]       # 0 transactions
    k = 0
    for align in range(4):
        for li, n0 in enumerate(BODY_LENGTHS):
            lens = [n0, BODY_LENGTHS[(li + 1 + align) % 5], BODY_LENGTHS[(li + 2) % 5]]
            bodies = [tx_body(n, rng) for n in lens]
            assert [len(b) for b in bodies] == lens
            wsets = []
            for t, body in enumerate(bodies):
                cnt = WIT_COUNTS[(k + 3 * t) % 7]
                if cnt is None:
                    wsets.append(cmap([]))
                else:
                    wsets.append(cmap([(uint(0), arr(vkey_wit(100 * k + q, b2b(body))
                                                     for q in range(cnt)))]))
            out.append((make_block(bodies, wsets, form=k % 4, tag=2 + k % 3), align))
            k += 1
    # every witness count in one block, so that none depends on the rotation above
    bodies = [tx_body(40 + t, rng) for t in range(7)]
    wsets = [cmap([]) if c is None else
             cmap([(uint(0), arr(vkey_wit(7000 + 70 * t + q, b2b(bodies[t])) for q in range(c)))])
             for t, c in enumerate(WIT_COUNTS)]
    out.append((make_block(bodies, wsets, form=2, tag=3), None))
    # key 2 alone, both keys, the unknown key before / between / after, a repeated key 0
    bodies = [tx_body(60 + t, rng) for t in range(6)]
    ids = [b2b(b) for b in bodies]
    k0 = lambda t, a, n: (uint(0), arr(vkey_wit(8000 + 10 * t + a + q, ids[t]) for q in range(n)))  # noqa: E731
    k2 = lambda t, a, n: (uint(2), arr(boot_wit(8500 + 10 * t + a + q, ids[t], rng) for q in range(n)))  # noqa: E731
    wsets = [cmap([k2(0, 0, 2)]),
             cmap([k0(1, 0, 2), k2(1, 2, 1)]),
             cmap([UNKNOWN, k0(2, 0, 1)]),
             cmap([k0(3, 0, 1), UNKNOWN, k2(3, 1, 1)]),
             cmap([k0(4, 0, 2), UNKNOWN]),
             cmap([k0(5, 0, 1), k2(5, 1, 1), k0(5, 2, 2)])]
    out.append((make_block(bodies, wsets, form=1), None))
    # indefinite containers: txBodies, txWitnesses, a witness set, witness arrays
    bodies = [tx_body(33, rng), b"\xbf\x00" + cbor_bytes(rng.bytes(20)) + b"\xff", tx_body(35, rng)]
    ids = [b2b(b) for b in bodies]
    wsets = [cmap([(uint(0), arr([vkey_wit(9000, ids[0]), vkey_wit(9001, ids[0])], indef=True))]),
             cmap([(uint(2), arr([boot_wit(9002, ids[1], rng)], indef=True)),
                   (uint(0), arr([], indef=True))], indef=True),
             cmap([], indef=True)]
    out.append((make_block(bodies, wsets, form=3, tag=4, indef_bodies=True, indef_sets=True), 3))
    out.append((make_block(bodies, wsets, indef_bodies=True), None))
    out.append((make_block(bodies, wsets, indef_sets=True), None))
    return out


def torsion_over(msg: bytes):
    """edge_cases.torsion_consistent_cases over a given message: per torsion
    order one signature libsodium accepts and one (R's torsion off by a step)
    it rejects.  [(pk, sig)]"""
    out = []
    seed = 0
    for k in (4, 2, 1):                     # [k]T8 has order 8 / k
        TA = E.smul(k, E.T8)
        found = False
        while not found:                    # (a fitting R exists for about every other nonce)
            seed += 1
            a = int.from_bytes(hashlib.sha512(b"wit-tors-a%d" % seed).digest(), "little") % E.L
            r = int.from_bytes(hashlib.sha512(b"wit-tors-r%d" % seed).digest(), "little") % E.L
            pk = E.enc_pt(E.add(E.smul(a, E.BASE), TA))
            rB = E.smul(r, E.BASE)
            for j in range(8):
                R = E.add(rB, E.smul(j, E.T8))
                Rb = E.enc_pt(R)
                h = int.from_bytes(hashlib.sha512(Rb + pk + msg).digest(), "little") % E.L
                if (j + h * k) % 8 == 0:    # [j]T8 == -[h k]T8
                    out.append((pk, Rb + ((r + h * a) % E.L).to_bytes(32, "little")))
                    Rw = E.enc_pt(E.add(R, E.T8))
                    hw = int.from_bytes(hashlib.sha512(Rw + pk + msg).digest(), "little") % E.L
                    out.append((pk, Rw + ((r + hw * a) % E.L).to_bytes(32, "little")))
                    found = True
                    break
    return out


def _three_tx(rng, counts=(2, 3, 1)):
    bodies = [tx_body(50 + 3 * t, rng) for t in range(3)]
    wits = [[vkey_wit(500 + 10 * t + q, b2b(bodies[t])) for q in range(c)]
            for t, c in enumerate(counts)]
    return bodies, wits


def _sets(wits):
    return [cmap([(uint(0), arr(w))]) for w in wits]


@functools.lru_cache(maxsize=None)
def invalid():
    """[(raw block, the n_bad it is built to give)]"""
    rng = np.random.default_rng(43)
    out = []
    bodies, wits = _three_tx(rng)
    good = make_block(bodies, _sets(wits))
    p = W.parse_witnesses(good)
    # one bit of a signature, of a vkey (payload bytes, found in the block)
    for field, bit in ((p.witnesses[3].sig, 0x01), (p.witnesses[1].vk, 0x10)):
        r = bytearray(good)
        r[good.index(field) + 5] ^= bit
        out.append((bytes(r), 1))
    # one bit of a tx body: every witness of that transaction and no other
    r = bytearray(good)
    o, n = p.tx_spans[1]
    r[o + n - 1] ^= 0x04
    out.append((bytes(r), 3))
    # a witness moved to another transaction
    moved = [wits[0][:1], wits[1] + wits[0][1:], wits[2]]
    out.append((make_block(bodies, _sets(moved), form=2), 1))
    # the acceptance corners as witnesses: the fixed ones as they are (over the
    # tx id the oracle says what each gives), the torsion ones over the tx id
    body = tx_body(90, rng)
    txid = b2b(body)
    corners = [(pk, sig) for pk, sig, _ in E.ed25519_edge_cases() if len(pk) == 32 and len(sig) == 64]
    tors = torsion_over(txid)
    assert [O.ed25519_verify(s, txid, a) for a, s in tors] == [True, False] * 3
    corners += tors
    pk, sk = keypair(1)
    corners.append((pk, O.ed25519_sign(sk, txid)))
    bad = sum(not O.ed25519_verify(sig, txid, pk) for pk, sig in corners)
    assert 0 < bad < len(corners) - 3      # the three consistent torsion cases and the honest one pass
    out.append((make_block([body], [cmap([(uint(0), arr(pair_wit(a, s) for a, s in corners))])],
                           form=1), bad))
    return out


@functools.lru_cache(maxsize=None)
def small_block() -> bytes:
    rng = np.random.default_rng(44)
    bodies = [tx_body(9, rng), tx_body(1, rng)]
    wsets = [cmap([UNKNOWN, (uint(0), arr([vkey_wit(3, b2b(bodies[0]))])),
                   (uint(2), arr([boot_wit(4, b2b(bodies[0]), rng)]))]), cmap([])]
    return make_block(bodies, wsets)


@functools.lru_cache(maxsize=None)
def malformed():
    """[(raw block, the status it must give)]"""
    rng = np.random.default_rng(45)
    bodies, wits = _three_tx(rng)
    sets = _sets(wits)
    txid = b2b(bodies[0])
    pk, sk = keypair(9)
    sig = O.ed25519_sign(sk, txid)
    one = lambda w, key=0: make_block(bodies[:1], [cmap([(uint(key), arr([w]))])])  # noqa: E731
    cc = cbor_bytes(bytes(32))
    out = [
        (make_block(bodies, sets + [cmap([])]), B.PACK_ESHAPE),           # more sets than bodies
        (make_block(bodies, sets[:2]), B.PACK_ESHAPE),                    # fewer
        (make_block(bodies, sets + [cmap([])], indef_sets=True), B.PACK_ESHAPE),
        (make_block(bodies, sets[:2], indef_sets=True), B.PACK_ESHAPE),
        (make_block([bodies[0], arr([uint(1)]), bodies[2]], sets), B.PACK_ESHAPE),  # a body that is no map
        (make_block(bodies[:1], [cmap([(b"\x61a", arr([]))])]), B.PACK_ESHAPE),     # a text key
        (make_block(bodies[:1], [arr([])]), B.PACK_ESHAPE),               # a set that is no map
        (make_block(bodies[:1], [cmap([(uint(0), cmap([]))])]), B.PACK_ESHAPE),     # key 0: no array
        (one(arr([cbor_bytes(pk), cbor_bytes(sig), cc])), B.PACK_ESHAPE),           # a pair of array(3)
        (one(arr([cbor_bytes(pk), cbor_bytes(sig)]), key=2), B.PACK_ESHAPE),        # bootstrap of array(2)
        (one(arr([cbor_bytes(pk), cbor_bytes(sig)], indef=True)), B.PACK_ESHAPE),   # an indefinite pair
        (one(arr([cbor_bytes(pk[:31]), cbor_bytes(sig)])), B.PACK_ESIZE),           # a 31-byte vkey
        (one(arr([cbor_bytes(pk), cbor_bytes(sig[:63])])), B.PACK_ESIZE),           # a 63-byte sig
        (one(arr([cbor_bytes(pk), cbor_bytes(sig), cbor_bytes(bytes(31)), b"\x40"]), key=2),
         B.PACK_ESIZE),                                                             # a 31-byte chain code
        (one(arr([b"\x5f" + cbor_bytes(pk) + b"\xff", cbor_bytes(sig)])), B.PACK_ESHAPE),  # indefinite vkey
        (one(arr([uint(5), cbor_bytes(sig)])), B.PACK_ESHAPE),                      # a vkey that is no string
        (one(arr([cbor_bytes(pk[:31]), uint(5)])), B.PACK_ESHAPE),                  # shape before size
        (small_block() + b"\x00", B.PACK_ECBOR),                                    # a trailing byte
        (wrap(small_block(), 2, tag=0), B.PACK_EBYRON),                             # Byron tags
        (wrap(small_block(), 3, tag=1), B.PACK_EBYRON),
        (b"\x83" + small_block()[1:], B.PACK_ESHAPE),
    ]
    return out


def truncations():
    raw = small_block()
    return [raw[:cut] for cut in range(len(raw))]


def expect(raw: bytes):
    """dict(status, tx_ids, wits [(tx, kind, vk, ok)]) one block must give"""
    try:
        p = W.parse_witnesses(raw)
    except B.BlockError as e:
        return dict(status=e.status, tx_ids=[], wits=[])
    ids = p.tx_ids(raw)
    return dict(status=B.PACK_OK, tx_ids=ids,
                wits=[(w.tx, w.kind, w.vk, O.ed25519_verify(w.sig, ids[w.tx], w.vk))
                      for w in p.witnesses])


def layout(raws, aligns=None):
    """One buffer holding every block, a block with a wanted alignment padded so
    that its first tx body starts there: (buf, off, len)"""
    parts, off, at = [], [], 0
    for k, raw in enumerate(raws):
        pad = 0
        if aligns is not None and aligns[k] is not None:
            pad = (aligns[k] - (at + first_body_offset(raw))) % 4
        parts += [bytes(pad), raw]
        off.append(at + pad)
        at += pad + len(raw)
    buf = np.frombuffer(b"".join(parts) + b"\x00", np.uint8)
    return buf, np.array(off, np.uint64), np.array([len(r) for r in raws], np.uint32)


def expected_arrays(raws):
    """The outputs of the verify entries over `raws` with capacities that fit"""
    memo = {}
    for r in raws:                 # (a tiled batch repeats a few blocks)
        if r not in memo:
            memo[r] = expect(r)
    exp = [memo[r] for r in raws]
    n = len(raws)
    tx_begin, wit_begin = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    ids, wit_tx, kind, vk, ok, n_bad = [], [], [], [], [], np.zeros(n, np.uint32)
    for i, e in enumerate(exp):
        tx_begin[i + 1] = tx_begin[i] + len(e["tx_ids"])
        wit_begin[i + 1] = wit_begin[i] + len(e["wits"])
        ids += e["tx_ids"]
        for t, kd, v, good in e["wits"]:
            wit_tx.append(int(tx_begin[i]) + t)
            kind.append(kd)
            vk.append(v)
            ok.append(1 if good else 0)
            n_bad[i] += 0 if good else 1
    status = np.array([e["status"] for e in exp], np.uint8)
    return dict(status=status, tx_begin=tx_begin, wit_begin=wit_begin,
                tx_id=np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32),
                wit_tx=np.array(wit_tx, np.uint32), wit_kind=np.array(kind, np.uint8),
                wit_vk=np.frombuffer(b"".join(vk), np.uint8).reshape(-1, 32),
                wit_ok=np.array(ok, np.uint8), n_bad=n_bad,
                verdict=((status == B.PACK_OK) & (n_bad == 0)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def case_set():
    """The whole set in one buffer with what it must give; computed once and
    shared (the tests leave it unchanged)."""
    raws = [r for r, _ in valid()]
    aligns = [a for _, a in valid()]
    kinds = ["valid"] * len(raws)
    for b in golden():
        raws.append(bytes.fromhex(b["raw"]))
        kinds.append("byron" if b["byron"] else "golden")
    for r, _ in invalid():
        raws.append(r)
        kinds.append("invalid")
    for r, _ in malformed():
        raws.append(r)
        kinds.append("malformed")
    for r in truncations():
        raws.append(r)
        kinds.append("truncation")
    aligns += [None] * (len(raws) - len(aligns))
    d = expected_arrays(raws)
    d.update(raws=raws, kinds=kinds, triple=layout(raws, aligns))
    return d


def check_result(r, want, n=None):
    """A WitnessResult (or arrays of the same names) against expected_arrays"""
    for f in ("status", "tx_begin", "wit_begin", "n_bad", "verdict"):
        got = np.asarray(getattr(r, f))
        assert got.tolist() == want[f].tolist(), f
    T, Wn = int(want["tx_begin"][-1]), int(want["wit_begin"][-1])
    assert np.array_equal(np.asarray(r.tx_id)[:T], want["tx_id"]), "tx_id"
    for f in ("wit_tx", "wit_kind", "wit_vk", "wit_ok"):
        assert np.array_equal(np.asarray(getattr(r, f))[:Wn], want[f]), f
