"""Cases for the epoch-nonce schedule and the combined raw entry
(tests/test_epochs.py, test_chain_cbor.py, test_gpu_chain_cbor.py).

Expected values never come from the code under test: TPraos rows are the
pinned host slicer + the oracle's header combiner (test_gpu_cbor._expect) with
explicit per-row alphas built here in Python (header.mk_seed over the row's
slot and the nonce its schedule entry carries); PBFT rows are the Python Byron
slicer + the oracle's donna-style verify (as test_gpu_multi_cbor._byron_cases).
Everything is built once per process and shared.
"""
import functools

import numpy as np

import hdr_cases as C
import oracle_ffi as O
from ouroboros_network_amd import byron as B
from ouroboros_network_amd import header as H
from ouroboros_network_amd.tpraos import EpochNonces

SPKP = 100  # the golden examples' slots per KES period (Examples.hs)
STRICT = 0x3F


@functools.lru_cache(maxsize=None)
def load_kats():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "reference_kats.json")) as f:
        return json.load(f)


def seeded_raw_at(kats, slots, nonces, prove_as=None, spkp=SPKP, era_every=3, seed=17):
    """hdr_cases.seeded_raw with the slot and the epoch nonce given per header:
    raw wire headers that verify completely under mkSeed seedEta / seedL
    slots[i] nonces[i] (None = NeutralNonce) -- the golden VRF and cold keys,
    oracle proofs and signatures.  prove_as[i] = (slot, nonce), when given,
    is what header i's two VRF certificates are proved for instead (another
    header's proofs inside a body that is still signed correctly: OCERT and
    KES hold, both VRFs fail)."""
    rng = np.random.default_rng(seed)
    h0 = H.parse_header(bytes.fromhex(kats["headers"][0]["raw"]))
    f0 = H.array_items(h0.body, 0)
    keep = lambda k: h0.body[f0[k][0]:f0[k][1]]  # noqa: E731
    cold_pk, cold_sk = O.ed25519_keypair(C.GOLDEN_VRF_SEED)
    _, vrf_sk = O.vrf_keypair(C.GOLDEN_VRF_SEED)
    kes_seed = b"\x05" * 32
    hot = O.kes_keygen(kes_seed)
    out = []
    for i, (slot, nonce) in enumerate(zip(slots, nonces)):
        slot = int(slot)
        t = int(rng.integers(0, 64))
        c0 = max(0, slot // spkp - t)
        t = slot // spkp - c0
        counter = int(rng.integers(0, 2**16))
        sigma = O.ed25519_sign(cold_sk, hot + counter.to_bytes(8, "big") + c0.to_bytes(8, "big"))
        pslot, pnonce = (slot, nonce) if prove_as is None or prove_as[i] is None else prove_as[i]
        certs = []
        for uc in (H.SEED_ETA, H.SEED_L):
            pi = O.vrf_prove(vrf_sk, O.mk_seed(uc, int(pslot), pnonce))
            certs.append(b"\x82" + C.cbor_bytes(O.vrf_proof_to_hash(pi)) + C.cbor_bytes(pi))
        fields = [keep(0), C.cbor_uint(slot), keep(2), C.cbor_bytes(cold_pk), keep(4), certs[0],
                  certs[1], keep(7), keep(8), C.cbor_bytes(hot), C.cbor_uint(counter),
                  C.cbor_uint(c0), C.cbor_bytes(sigma), keep(13), keep(14)]
        body = C._cbor_head(4, 15) + b"".join(fields)
        sig = O.kes_sign(kes_seed, min(t, 63), body)
        out.append(C.wire_header(fields, sig, era=(2 if i % era_every == 0 else None)))
    return out


def alphas(slots, nonces):
    """mkSeed seedEta / seedL slot nonce per row, in Python (header.mk_seed)."""
    ea = b"".join(H.mk_seed(H.SEED_ETA, int(s), n) for s, n in zip(slots, nonces))
    la = b"".join(H.mk_seed(H.SEED_L, int(s), n) for s, n in zip(slots, nonces))
    return (np.frombuffer(ea, np.uint8).reshape(-1, 32).copy(),
            np.frombuffer(la, np.uint8).reshape(-1, 32).copy())


def expect_tpraos(raws, ea, la):
    """(verdict, beta_eta, beta_leader, eta_nonce, status): host slicer + oracle"""
    from test_gpu_cbor import _expect

    return _expect(raws, SPKP, ea, la)


# ---- the three-epoch schedule ------------------------------------------------
SCHED3_FIRST = [0, 1000, 5000]
SCHED3_NONCES = [None, b"\x33" * 32, np.random.default_rng(99).bytes(32)]
SCHED3_SLOTS = [0, 999, 1000, 1001, 4999, 5000, 2**40, 2**64 - 1]


def sched3():
    return EpochNonces(first_slot=SCHED3_FIRST,
                       nonce=[n or bytes(32) for n in SCHED3_NONCES],
                       neutral=[n is None for n in SCHED3_NONCES])


def sched3_nonce(slot):
    """the schedule's answer for a slot, worked out here (not by the library)"""
    j = max(k for k, f in enumerate(SCHED3_FIRST) if f <= slot)
    return SCHED3_NONCES[j]


@functools.lru_cache(maxsize=None)
def _epoch3(swapped):
    kats = load_kats()
    slots = list(SCHED3_SLOTS)
    nonces = [sched3_nonce(s) for s in slots]
    prove_as = None
    if swapped:  # rows 999 <-> 1000 and 4999 <-> 5000 carry each other's proofs
        prove_as = [None] * len(slots)
        for a, b in ((1, 2), (4, 5)):
            prove_as[a], prove_as[b] = (slots[b], nonces[b]), (slots[a], nonces[a])
    raws = seeded_raw_at(kats, slots, nonces, prove_as)
    ea, la = alphas(slots, nonces)
    return raws, np.array(slots, np.uint64), ea, la, expect_tpraos(raws, ea, la)


def epoch3(swapped=False):
    """(raws, slots, eta_alpha, leader_alpha, want) of the three-epoch headers"""
    return _epoch3(bool(swapped))


# ---- a long schedule: first_slot = 0, 10, 20, ... ------------------------------
def sched_k(k):
    rng = np.random.default_rng(1000 + k)
    nonce = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    return EpochNonces(first_slot=np.arange(k, dtype=np.uint64) * 10, nonce=nonce), nonce


@functools.lru_cache(maxsize=None)
def sched_k_cases(k):
    """headers for entries at both ends and in the middle of a k-entry schedule,
    on each entry's first and last slot"""
    kats = load_kats()
    E, nonce = sched_k(k)
    entries = sorted({j for j in (0, 1, 2047, 2048, 4094, 4095) if j < k})
    slots, nonces = [], []
    for j in entries:
        # the last entry has no end: its "last" slot is taken far above it
        last = 10 * j + 9 if j + 1 < k else 2**50 + j
        for s in (10 * j, last):
            slots.append(s)
            nonces.append(nonce[j].tobytes())
    raws = seeded_raw_at(kats, slots, nonces, seed=k)
    ea, la = alphas(slots, nonces)
    return E, raws, np.array(slots, np.uint64), expect_tpraos(raws, ea, la)


# ---- PBFT expectations and mixed streams -----------------------------------------
def expect_byron(raws):
    """(verdict 0 / 1, status) per header: byron.byron_status + the oracle"""
    want, st = [], []
    for r in raws:
        s, h = B.byron_status(r)
        st.append(s)
        if s == B.PACK_EBB:
            want.append(1)
        elif s != B.PACK_OK:
            want.append(0)
        else:
            want.append(int(O.ed25519_verify_byron(h.sig, h.message(B.HEADER_MAGIC),
                                                   h.delegate_xpub[:32])))
    return np.array(want, np.uint8), np.array(st, np.uint8)


def expect_chain(raws, ea, la):
    """The combined entry's expected arrays for `raws` (ea / la: n x 32, the
    PBFT rows' entries ignored): (proto, status, verdict, beta_eta, beta_leader,
    eta_nonce); the class of a row by the Python classifier, which
    test_chain_cbor.py pins against both Python slicers."""
    n = len(raws)
    proto = np.array([H.era_class(r) for r in raws], np.uint8)
    status = np.zeros(n, np.uint8)
    verdict = np.zeros(n, np.uint8)
    be = np.zeros((n, 64), np.uint8)
    bl = np.zeros((n, 64), np.uint8)
    en = np.zeros((n, 32), np.uint8)
    ti = np.nonzero(proto == H.PROTO_TPRAOS)[0]
    bi = np.nonzero(proto == H.PROTO_PBFT)[0]
    if ti.size:
        v, e, l, nn, st = expect_tpraos([raws[i] for i in ti], ea[ti], la[ti])
        ok = st == H.PACK_OK
        status[ti], verdict[ti] = st, v
        # (a rejected header's outputs are unspecified zeros in the library)
        be[ti[ok]], bl[ti[ok]], en[ti[ok]] = e[ok], l[ok], nn[ok]
    if bi.size:
        verdict[bi], status[bi] = expect_byron([raws[i] for i in bi])
    return proto, status, verdict, be, bl, en


def assert_chain_equal(got, want):
    """got = verify_chain_cbor(..., nonce=True); TPraos outputs compared on the
    rows that slice, PBFT outputs must be zero"""
    proto, status, verdict, be, bl, en = got
    np.testing.assert_array_equal(proto, want[0])
    np.testing.assert_array_equal(status, want[1])
    np.testing.assert_array_equal(verdict, want[2])
    ok = (want[0] == H.PROTO_PBFT) | (want[1] == H.PACK_OK)
    np.testing.assert_array_equal(be[ok], want[3][ok])
    np.testing.assert_array_equal(bl[ok], want[4][ok])
    np.testing.assert_array_equal(en[ok], want[5][ok])


@functools.lru_cache(maxsize=None)
def fixtures15():
    """the 8 Byron wire fixtures then the 7 Shelley ones, their golden alphas
    (zero rows for the Byron ones), and the expected arrays"""
    kats = load_kats()
    raws = [bytes.fromhex(w["raw"]) for w in kats["byron_wire"]] + \
        [bytes.fromhex(h["raw"]) for h in kats["headers"]]
    z = bytes(32)
    ea = np.frombuffer(b"".join([z] * 8 + [bytes.fromhex(h["eta_alpha"]) for h in kats["headers"]]),
                       np.uint8).reshape(-1, 32).copy()
    la = np.frombuffer(b"".join([z] * 8 + [bytes.fromhex(h["leader_alpha"])
                                           for h in kats["headers"]]),
                       np.uint8).reshape(-1, 32).copy()
    kinds = [w["kind"] for w in kats["byron_wire"]]
    return raws, ea, la, kinds, expect_chain(raws, ea, la)


@functools.lru_cache(maxsize=None)
def corruptions():
    """one regular Byron fixture and one Shelley fixture, each followed by every
    single-byte ^0x04 corruption of it, interleaved into one stream (about
    1,600 rows; every byte of a Shelley header is signed, so only the fixture
    itself is valid in that class)"""
    kats = load_kats()
    byr = next(bytes.fromhex(w["raw"]) for w in kats["byron_wire"] if w["kind"] == "regular")
    h = kats["headers"][0]
    she = bytes.fromhex(h["raw"])
    a, l = bytes.fromhex(h["eta_alpha"]), bytes.fromhex(h["leader_alpha"])

    def flips(g):
        out = [g]  # the fixture itself first: each class has a valid row
        for pos in range(len(g)):
            m = bytearray(g)
            m[pos] ^= 0x04
            out.append(bytes(m))
        return out

    fb, fs = flips(byr), flips(she)
    raws, ea, la = [], [], []
    for i in range(max(len(fb), len(fs))):  # one by one while both last
        for src, al in ((fs, (a, l)), (fb, (bytes(32), bytes(32)))):
            if i < len(src):
                raws.append(src[i])
                ea.append(al[0])
                la.append(al[1])
    ea = np.frombuffer(b"".join(ea), np.uint8).reshape(-1, 32).copy()
    la = np.frombuffer(b"".join(la), np.uint8).reshape(-1, 32).copy()
    return raws, ea, la, expect_chain(raws, ea, la)


@functools.lru_cache(maxsize=None)
def three_epoch_stream():
    """the three-epoch seeded Shelley headers with Byron fixtures spliced in at
    the front, in the middle and at the end; expectations from per-row alphas"""
    kats = load_kats()
    raws, slots, ea, la, _ = epoch3()
    wires = [bytes.fromhex(w["raw"]) for w in kats["byron_wire"]]
    z = np.zeros((1, 32), np.uint8)
    out, oea, ola = [], [], []

    def put(r, e, l):
        out.append(r)
        oea.append(e)
        ola.append(l)

    for w in wires[:3]:
        put(w, z, z)
    half = len(raws) // 2
    for i in range(half):
        put(raws[i], ea[i:i + 1], la[i:i + 1])
    for w in wires[3:6]:
        put(w, z, z)
    for i in range(half, len(raws)):
        put(raws[i], ea[i:i + 1], la[i:i + 1])
    for w in wires[6:]:
        put(w, z, z)
    ea2, la2 = np.concatenate(oea), np.concatenate(ola)
    return out, expect_chain(out, ea2, la2)
