"""Raw header streams for the envelope tests (tests/test_envelope_rule.py,
test_gpu_envelope.py): Byron and TPraos wire headers with chosen block numbers,
slots and previous hashes, built from the reference's golden headers by
re-encoding those fields alone.  Signatures are not re-made: the envelope does
not look at them.  Hashes for the links come from hashlib here; expectations
in the tests come from ouroboros_network_amd.envelope."""
import functools
import hashlib
import json
import os

import hdr_cases as C
from ouroboros_network_amd import envelope as E
from ouroboros_network_amd import header as H

HERE = os.path.dirname(os.path.abspath(__file__))
EPOCH_SLOTS = 21600
ALL = E.ENV_ALL_OK


def b2b(m: bytes) -> bytes:
    return hashlib.blake2b(m, digest_size=32).digest()


@functools.lru_cache(maxsize=None)
def fixtures():
    with open(os.path.join(HERE, "golden", "reference_envelope.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def kats():
    with open(os.path.join(HERE, "golden", "reference_kats.json")) as f:
        return json.load(f)


def arr(*items: bytes) -> bytes:
    return C._cbor_head(4, len(items)) + b"".join(items)


# ---- Byron ----------------------------------------------------------------------
def byron_wire(kind: int, item: bytes, form: int) -> bytes:
    """the header item in wire form F1 / F2 / F3 (csrc/cbor_byron.h)"""
    if form == 1:
        return b"\xd8\x18" + C.cbor_bytes(arr(C.cbor_uint(kind), item))
    f2 = arr(arr(C.cbor_uint(kind), C.cbor_uint(len(item))), b"\xd8\x18" + C.cbor_bytes(item))
    return f2 if form == 2 else arr(C.cbor_uint(0), f2)


@functools.lru_cache(maxsize=None)
def _regular_parts():
    item = bytes.fromhex(fixtures()["byron_regular_header"])
    f = H.array_items(item, 0)
    cons = H.array_items(item, f[3][0])
    cut = lambda s: item[s[0]:s[1]]  # noqa: E731
    return cut(f[0]), cut(f[2]), cut(cons[1]), cut(cons[3])


def byron_regular(prev: bytes, epoch: int, in_epoch: int, block_no: int, extra_len: int = 0,
                  form: int = 1, slot_id=None, difficulty=None):
    """(wire header, its hash): the golden regular header with prevHash, slotId,
    difficulty and an extraData attribute blob of extra_len bytes of our own"""
    magic, proof, leader, sig = _regular_parts()
    sid = slot_id if slot_id is not None else arr(C.cbor_uint(epoch), C.cbor_uint(in_epoch))
    diff = difficulty if difficulty is not None else arr(C.cbor_uint(block_no))
    extra = arr(arr(C.cbor_uint(1), C.cbor_uint(0), C.cbor_uint(0)),
                arr(C.cbor_bytes(b"cardano-sl"), C.cbor_uint(1)),
                C._cbor_head(5, 1) + C.cbor_uint(200) + C.cbor_bytes(bytes(extra_len)),
                C.cbor_bytes(bytes(32)))
    item = arr(magic, C.cbor_bytes(prev), proof, arr(sid, leader, diff, sig), extra)
    return byron_wire(1, item, form), b2b(b"\x82\x01" + item)


def byron_ebb(prev: bytes, epoch: int, block_no: int, form: int = 1, extra_len: int = 0,
              consensus=None):
    """(wire header, its hash) of an epoch-boundary header"""
    magic, proof, _, _ = _regular_parts()
    cons = consensus if consensus is not None else \
        arr(C.cbor_uint(epoch), arr(C.cbor_uint(block_no)))
    item = arr(magic, C.cbor_bytes(prev), C.cbor_bytes(bytes(32)), cons,
               arr(C._cbor_head(5, 1) + C.cbor_uint(200) + C.cbor_bytes(bytes(extra_len))))
    return byron_wire(0, item, form), b2b(b"\x82\x00" + item)


# ---- TPraos ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tpraos_parts():
    h0 = H.parse_header(bytes.fromhex(kats()["headers"][0]["raw"]))
    f = H.array_items(h0.body, 0)
    return [h0.body[a:b] for a, b in f], h0.kes_sig


GENESIS = b"\xf6"


def tpraos(prev, slot: int, block_no: int, era=None, body_size=None, prot_major=None,
           pad: int = 0, body_hash_len=None):
    """(wire header, its hash): the first golden Shelley header with fields 0, 1
    and 2 re-encoded (prev: 32 bytes, GENESIS, or the raw CBOR of field 2 when
    not 32 bytes long), optionally fields 7 and 13; pad: field 14 (the minor
    protocol version) as a uint with that many more bytes, and body_hash_len:
    field 8 (no slicer looks at it) as that many bytes, to step the length"""
    fields, sig = _tpraos_parts()
    fields = list(fields)
    fields[0], fields[1] = C.cbor_uint(block_no), C.cbor_uint(slot)
    fields[2] = C.cbor_bytes(prev) if len(prev) == 32 else prev
    if body_size is not None:
        fields[7] = body_size if isinstance(body_size, bytes) else C.cbor_uint(body_size)
    if prot_major is not None:
        fields[13] = C.cbor_uint(prot_major)
    if body_hash_len is not None:
        fields[8] = C.cbor_bytes(bytes(range(body_hash_len)))
    if pad:
        fields[14] = bytes([0x18 + {1: 0, 2: 1, 4: 2, 8: 3}[pad]]) + bytes(pad)
    raw = C.wire_header(fields, sig, era=era)
    inner = b"\x82" + C._cbor_head(4, 15) + b"".join(fields) + C.cbor_bytes(sig)
    return raw, b2b(inner)


# ---- streams --------------------------------------------------------------------
def good_chain(n_byron: int, n_tpraos: int, ebb_every: int = 7, extra_step: int = 1):
    """A chain every link of which is valid, from Origin: an epoch-0 EBB, Byron
    regular headers with an EBB at every epoch start (epochs of `ebb_every`
    regular headers apart), then TPraos headers.  Wire forms, extraData
    lengths and HFC wrapping vary along it.  Returns the raw headers."""
    raws = []
    raw, h = byron_ebb(bytes(32), 0, 0, form=1)
    raws.append(raw)
    block_no, epoch, in_epoch = 0, 0, 0
    last_ebb = True
    while len(raws) < n_byron:
        i = len(raws)
        if not last_ebb and i % ebb_every == 0:
            epoch += 1
            in_epoch = 0
            raw, h = byron_ebb(h, epoch, block_no, form=1 + i % 3, extra_len=(i * extra_step) % 200)
            last_ebb = True
        else:
            block_no += 1
            raw, h = byron_regular(h, epoch, in_epoch, block_no, extra_len=(i * extra_step) % 300,
                                   form=1 + i % 3)
            in_epoch += 1 + i % 2
            last_ebb = False
        raws.append(raw)
    slot = epoch * EPOCH_SLOTS + in_epoch + 5 if raws else 0
    for i in range(n_tpraos):
        block_no += 1
        slot += 1 + (i % 5) * 1000
        raw, h = tpraos(h, slot, block_no, era=(None if i % 3 else 2), pad=(0, 1, 2, 4, 8)[i % 5])
        raws.append(raw)
    return raws


def expect(raws, tip=E.ORIGIN, cfg=None):
    """envelope.py over the stream: (usable flags, hashes, bits, tip_out)"""
    recs, hashes, bits, tip_out = E.validate_envelope(raws, tip, cfg or E.Cfg(EPOCH_SLOTS))
    return [r is not None for r in recs], hashes, bits, tip_out


def spaced(raws, gaps=(0, 1, 2, 3, 5), shift=0):
    """(buf, off, len) with the headers apart by cycling gaps, so that they
    start at every address residue mod 4 whatever their lengths; shift: that
    many more bytes behind the first header, which moves every later one"""
    import numpy as np

    parts, off, at = [], [], 0
    for i, r in enumerate(raws):
        g = gaps[i % len(gaps)] + (shift if i == 1 else 0)
        parts.append(b"\xee" * g)
        at += g
        off.append(at)
        parts.append(r)
        at += len(r)
    return (np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64),
            np.array([len(r) for r in raws], np.uint32))


def signed_chain(prev, slots, first_block_no, nonces, spkp=100, seed=23):
    """TPraos wire headers that verify completely (chain_cases.seeded_raw_at's
    construction: golden VRF and cold keys, oracle proofs and signatures) AND
    link: header i's field 2 is header i - 1's hash (`prev` for the first), its
    block number first_block_no + i.  Returns (raws, last hash)."""
    import numpy as np

    import oracle_ffi as O

    rng = np.random.default_rng(seed)
    fields0, _ = _tpraos_parts()
    cold_pk, cold_sk = O.ed25519_keypair(C.GOLDEN_VRF_SEED)
    _, vrf_sk = O.vrf_keypair(C.GOLDEN_VRF_SEED)
    kes_seed = b"\x05" * 32
    hot = O.kes_keygen(kes_seed)
    out, h = [], prev
    for i, (slot, nonce) in enumerate(zip(slots, nonces)):
        slot = int(slot)
        t = int(rng.integers(0, 64))
        c0 = max(0, slot // spkp - t)
        t = slot // spkp - c0
        counter = int(rng.integers(0, 2**16))
        sigma = O.ed25519_sign(cold_sk, hot + counter.to_bytes(8, "big") + c0.to_bytes(8, "big"))
        certs = []
        for uc in (H.SEED_ETA, H.SEED_L):
            pi = O.vrf_prove(vrf_sk, O.mk_seed(uc, slot, nonce))
            certs.append(b"\x82" + C.cbor_bytes(O.vrf_proof_to_hash(pi)) + C.cbor_bytes(pi))
        f = list(fields0)
        f[0], f[1] = C.cbor_uint(first_block_no + i), C.cbor_uint(slot)
        f[2] = C.cbor_bytes(h) if len(h) == 32 else h
        f[3], f[5], f[6], f[9] = C.cbor_bytes(cold_pk), certs[0], certs[1], C.cbor_bytes(hot)
        f[10], f[11], f[12] = C.cbor_uint(counter), C.cbor_uint(c0), C.cbor_bytes(sigma)
        body = C._cbor_head(4, 15) + b"".join(f)
        sig = O.kes_sign(kes_seed, min(t, 63), body)
        out.append(C.wire_header(f, sig, era=(2 if i % 3 == 0 else None)))
        h = b2b(b"\x82" + body + C.cbor_bytes(sig))
    return out, h


VAL_CFG = E.Cfg(100)  # short Byron epochs: the Byron part ends below slot 990


@functools.lru_cache(maxsize=None)
def validate_stream():
    """A chain for the combined entry: Byron (golden forms with extraData of
    varying length and EBBs; their signatures do not verify), the era switch,
    then TPraos headers over the three epochs of chain_cases.sched3 that verify
    completely and link -- and one of them with a signature flipped, one with a
    wrong previous hash.  Returns (raws, ea, la, crypto expectation, envelope
    expectation)."""
    import numpy as np

    import chain_cases as CC

    byron = good_chain(30, 0, ebb_every=9, extra_step=11)
    last = E.header_record(byron[-1], VAL_CFG)
    assert last.slot < 500
    slots = [last.slot + 1 + 17 * i for i in range(8)] + [990, 999, 1000, 1001, 1500, 4999, 5000,
                                                          5001, 2**40, 2**40 + 1]
    slots = sorted(set(slots))
    nonces = [CC.sched3_nonce(s) for s in slots]
    tp, _ = signed_chain(last.hash, slots, last.block_no + 1, nonces)
    bad = bytearray(tp[5])
    bad[-9] ^= 1                       # inside the KES signature: the hash moves too
    tp[5] = bytes(bad)
    raws = byron + tp
    z = np.zeros((len(byron), 32), np.uint8)
    ea, la = CC.alphas(slots, nonces)
    ea, la = np.concatenate([z, ea]), np.concatenate([z, la])
    return raws, ea, la, CC.expect_chain(raws, ea, la), expect(raws, cfg=VAL_CFG)


def expect_status(raws):
    """the slicer's status per header, from the Python slicers: the exact
    OURO_PACK_* code for a Byron header (byron.byron_status); for a TPraos
    header 0 where header.parse_header accepts it and None (any nonzero code)
    where it does not"""
    from ouroboros_network_amd import byron as B

    out = []
    for r in raws:
        if H.era_class(r) == H.PROTO_PBFT:
            out.append(B.byron_status(r)[0])
        else:
            try:
                H.parse_header(r)
                out.append(0)
            except (H.CBORError, IndexError):
                out.append(None)
    return out


def assert_status(status, raws):
    for i, (got, want) in enumerate(zip(status, expect_status(raws))):
        assert (got != 0) if want is None else (got == want), (i, int(got), want)
