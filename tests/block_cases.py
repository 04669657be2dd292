"""Raw blocks for the whole-block integrity tests (CPU and GPU), and what every
one of them must give.

Expectations never come from the library: the slicer status from
block.parse_block (the pure-Python restatement), the body hash from hashlib,
the KES verdict from the oracle's kes_verify.

* golden: the reference's golden block files (tests/golden/reference_blocks.json);
* synthetic: the golden Shelley header's fields with field 8 replaced by the
  computed bbHash and a fresh Sum6KES key, re-signed with the oracle -- the
  way hdr_cases.seeded_raw builds headers -- over segments (CBOR arrays / maps
  of byte strings) of the encoded lengths SEG_LENGTHS, the first segment of
  each length starting at each of the four byte alignments of the buffer, in
  all four block encodings; one block with indefinite-length containers;
* flips: per golden and synthetic block one byte changed in each segment, in
  the bodyHash field, and elsewhere in the header body;
* shapes: truncations, a trailing byte, array(3) / array(5), a tag-24 payload
  longer / shorter than its block, nesting at and past cbor::skip's stack.
"""
import functools
import hashlib
import json
import os

import numpy as np

import oracle_ffi as O
from hdr_cases import _cbor_head, cbor_bytes
from ouroboros_network_amd import block as B
from ouroboros_network_amd import header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPKP = 129600
SEG_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097, 70000]
KES_SEED = b"\x09" * 32


def b2b(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "reference_blocks.json")) as f:
        return json.load(f)["blocks"]


def segment(total: int, rng, as_map: bool) -> bytes:
    """A CBOR array (or map) of byte strings whose encoding is exactly
    `total` bytes: empty strings, then one string that takes the rest."""
    if total == 1:
        return b"\xa0" if as_map else b"\x80"
    for empties in range(9):
        strings = empties + 1
        if as_map and strings % 2:
            continue  # key / value pairs
        items = strings // 2 if as_map else strings
        for hw in (1, 2, 3, 5):
            k = total - 1 - empties - hw
            if k < 0:
                continue
            if len(_cbor_head(2, k)) == hw:
                head = bytes([(0xA0 if as_map else 0x80) | items])
                return head + b"\x40" * empties + cbor_bytes(rng.bytes(k))
    raise ValueError(total)


def wrap(block: bytes, form: int, tag: int = 2) -> bytes:
    """The four block encodings: bare, tag-24, [tag, block], tag-24 of that"""
    if form & 2:
        block = b"\x82" + _cbor_head(0, tag) + block
    if form & 1:
        block = b"\xd8\x18" + cbor_bytes(block)
    return block


@functools.lru_cache(maxsize=None)
def _golden_header_fields():
    raw = bytes.fromhex(golden()[0]["raw"])  # Shelley on disk: bare array(4)
    pb = B.parse_block(raw)
    body = raw[pb.header_body_span[0]:pb.header_body_span[1]]
    f = H.array_items(body, 0)
    return [body[a:b] for a, b in f], pb


def make_block(segs, form=0, tag=2):
    """A valid block over the three encoded segments: bodyHash = bbHash, the
    hot key KES_SEED's, the KES signature over the re-encoded header body at
    the golden header's period."""
    fields, pb = _golden_header_fields()
    fields = list(fields)
    fields[8] = cbor_bytes(b2b(b"".join(b2b(s) for s in segs)))
    fields[9] = cbor_bytes(O.kes_keygen(KES_SEED))
    body = _cbor_head(4, 15) + b"".join(fields)
    t = H.kes_t(pb.slot, SPKP, pb.ocert_kes_period)
    assert t < 64
    sig = O.kes_sign(KES_SEED, t, body)
    header = b"\x82" + body + cbor_bytes(sig)
    return wrap(b"\x84" + header + b"".join(segs), form, tag)


def _first_segment_offset(raw):
    return B.parse_block(raw).segments[0][0]


@functools.lru_cache(maxsize=None)
def synthetic():
    """[(raw block, wanted alignment of its first segment in the buffer)]"""
    rng = np.random.default_rng(77)
    out = []
    k = 0
    for li, n0 in enumerate(SEG_LENGTHS):
        for align in range(4):
            lens = (n0, SEG_LENGTHS[(li + 1 + align) % 13], SEG_LENGTHS[(li + 5 + 2 * align) % 13])
            segs = [segment(n, rng, as_map=bool((k + s) % 2)) for s, n in enumerate(lens)]
            assert [len(s) for s in segs] == list(lens)
            out.append((make_block(segs, form=k % 4, tag=2 + k % 3), align))
            k += 1
    # indefinite-length containers (hashed as they stand; not pinned by a
    # reference fixture): an indefinite array of strings, an indefinite map,
    # an array holding an indefinite byte string
    segs = [b"\x9f" + cbor_bytes(rng.bytes(300)) + b"\x40\xff",
            b"\xbf\x41\x01" + cbor_bytes(rng.bytes(70)) + b"\xff",
            b"\x81\x5f" + cbor_bytes(rng.bytes(130)) + cbor_bytes(rng.bytes(5)) + b"\xff"]
    out.append((make_block(segs, form=3, tag=4), 1))
    return out


def _flip_keeping_shape(raw, lo, hi):
    """raw with one byte of [lo, hi) changed so that it still slices with the
    same spans (searched from the end: payload bytes), or None"""
    want = B.parse_block(raw)
    for pos in range(hi - 1, lo - 1, -1):
        for bit in (0x01, 0x20):
            r = bytearray(raw)
            r[pos] ^= bit
            try:
                got = B.parse_block(bytes(r))
            except B.BlockError:
                continue
            if got.segments == want.segments and got.header_body_span == want.header_body_span:
                return bytes(r)
    return None


def flips(raw):
    """[(kind, flipped block)]: kind 'seg' (a byte of one segment), 'hash' (a
    byte of the bodyHash field), 'body' (another byte of the header body)"""
    pb = B.parse_block(raw)
    out = []
    for o, n in pb.segments:
        r = _flip_keeping_shape(raw, o, o + n)
        assert r is not None
        out.append(("seg", r))
    at = raw.index(pb.body_hash, pb.header_body_span[0])
    r = bytearray(raw)
    r[at + 7] ^= 0x10
    out.append(("hash", bytes(r)))
    r = bytearray(raw)
    r[pb.header_body_span[0] + 12] ^= 0x04   # inside prevHash's payload
    out.append(("body", bytes(r)))
    return out


def shapes():
    """Malformed variants of a bare block and of a wrapped one"""
    g = {b["name"]: bytes.fromhex(b["raw"]) for b in golden()}
    out = []
    for raw in (g["shelley_disk"], g["cardano_n2n_Mary"], g["cardano_disk_Allegra"]):
        for cut in (0, 1, len(raw) // 2, len(raw) - 1):
            out.append(raw[:cut])
        out.append(raw + b"\x00")
    bare = g["shelley_disk"]
    out.append(b"\x83" + bare[1:])
    out.append(b"\x85" + bare[1:])
    out.append(b"\x85" + bare[1:] + b"\x80")
    out.append(b"\x9f" + bare[1:] + b"\xff")            # an indefinite block array
    wire = g["shelley_n2n"]                              # d8 18 59 hi lo block
    assert wire[:3] == b"\xd8\x18\x59"
    n = int.from_bytes(wire[3:5], "big")
    out.append(wire[:3] + (n + 1).to_bytes(2, "big") + wire[5:])           # payload past the span
    out.append(wire[:3] + (n - 1).to_bytes(2, "big") + wire[5:])           # bytes after the payload
    out.append(wire[:3] + (n + 1).to_bytes(2, "big") + wire[5:] + b"\x00")  # payload longer than its block
    out.append(b"\x82\x02" + b"\x82\x02" + bare)        # a tag inside a tag
    out.append(b"\x82\x20" + bare)                      # a negative tag
    out.append(b"\x82\x00" + bare)                      # Byron tags on a Shelley body
    out.append(b"\x82\x01" + bare)
    rng = np.random.default_rng(5)
    ok = [segment(40, rng, False), segment(41, rng, True)]
    for depth in (63, 64, 65, 200):                     # arrays open below the segment itself
        out.append(make_block(ok + [b"\x81" * depth + b"\x80"]))
    out.append(make_block(ok + [b"\x1c"]))              # a reserved head
    out.append(make_block(ok + [b"\x5a\x00\x01\x00\x00ab"]))  # a string past the end
    out.append(make_block(ok + [b"\x80"])[:-1])         # the last segment missing
    return out


def expect(raw):
    """(status, verdict, body_hash) one block must give"""
    try:
        pb = B.parse_block(raw)
    except B.BlockError as e:
        return e.status, 0, bytes(32)
    bb = pb.bb_hash(raw)
    t = min(H.kes_t(pb.slot, SPKP, pb.ocert_kes_period), 0xFFFFFFFF)
    msg = raw[pb.header_body_span[0]:pb.header_body_span[1]]
    kes = O.kes_verify(pb.hot_vk, t, msg, pb.kes_sig)
    return B.PACK_OK, (B.BLK_KES_OK if kes else 0) | (B.BLK_BODY_OK if bb == pb.body_hash else 0), bb


@functools.lru_cache(maxsize=None)
def case_set():
    """The whole set, laid out in one buffer: returns a dict with
    raws, (buf, off, len) -- synthetic blocks padded so that their first
    segment starts at the wanted alignment --, kind per case, and the expected
    status / verdict / body_hash arrays.  Computed once and shared."""
    raws, kinds, aligns = [], [], []
    base = [(bytes.fromhex(b["raw"]), None, "byron" if b["byron"] else "golden") for b in golden()]
    base += [(r, a, "synthetic") for r, a in synthetic()]
    for raw, align, kind in base:
        raws.append(raw)
        kinds.append(kind)
        aligns.append(align)
        if kind == "byron":
            continue
        for fk, r in flips(raw):
            raws.append(r)
            kinds.append("flip_" + fk)
            aligns.append(None)
    for r in shapes():
        raws.append(r)
        kinds.append("shape")
        aligns.append(None)
    parts, off, at = [], [], 0
    for raw, align in zip(raws, aligns):
        pad = 0
        if align is not None:
            pad = (align - (at + _first_segment_offset(raw))) % 4
        parts += [bytes(pad), raw]
        off.append(at + pad)
        at += pad + len(raw)
    buf = np.frombuffer(b"".join(parts) + b"\x00", np.uint8)
    off = np.array(off, np.uint64)
    ln = np.array([len(r) for r in raws], np.uint32)
    exp = [expect(r) for r in raws]
    return dict(raws=raws, kinds=kinds, aligns=aligns, triple=(buf, off, ln),
                status=np.array([e[0] for e in exp], np.uint8),
                verdict=np.array([e[1] for e in exp], np.uint8),
                body_hash=np.frombuffer(b"".join(e[2] for e in exp), np.uint8).reshape(-1, 32))


# ---- messages for the generic hash ----
@functools.lru_cache(maxsize=None)
def hash_spans():
    """(buf, off, len): every length of SEG_LENGTHS and 0 at alignments 0..3,
    then overlapping and identical spans"""
    rng = np.random.default_rng(9)
    buf = np.frombuffer(rng.bytes(80000), np.uint8)
    off, ln = [], []
    for a in range(4):
        for k, n in enumerate([0] + SEG_LENGTHS):
            off.append(4 * (37 * k % 100) + a)
            ln.append(n)
    for k in range(12):                       # overlapping
        off.append(1000 + 50 * k)
        ln.append(300 + k)
    off += [777, 777, 777]                    # identical
    ln += [129, 129, 129]
    return buf, np.array(off, np.uint64), np.array(ln, np.uint32)


def hash_expect(buf, off, ln):
    b = buf.tobytes()
    return np.frombuffer(b"".join(b2b(b[int(o):int(o) + int(n)]) for o, n in zip(off, ln)),
                         np.uint8).reshape(-1, 32)
