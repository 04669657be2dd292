"""Cases for the ledger-view checks (tests/test_ledger_rule.py,
test_ocert_counter_fold.py, test_gpu_ledger.py): view schedules and header rows
chosen for the rule's branches and the searches' edges, and a signed, linked
chain forged by four pools (envelope_cases.signed_chain's construction with the
pool's own cold and VRF keys).  Expectations come from ledger.rule / fold_rule
(hashlib, bisect, oracle/leader.py, a dict), never from the library."""
import functools
import importlib.util
import os
from fractions import Fraction

import numpy as np

from ouroboros_network_amd import ledger as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("oracle_leader",
                                               os.path.join(ROOT, "oracle", "leader.py"))
OL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(OL)

RES = 10**34
SPKP, MAX_EVO = 100, 64
G_MAIN = L.Globals(SPKP, MAX_EVO, OL.active_slot_log(Fraction(1, 20)))
G_ONE = L.Globals(SPKP, MAX_EVO, 0, f_is_one=True)
G_BAD = [L.Globals(SPKP, MAX_EVO, 1), L.Globals(SPKP, MAX_EVO, -8 * RES - 1)]
G_EDGE = L.Globals(SPKP, MAX_EVO, -8 * RES)
D63 = (2**62 - 57, 2**63 - 25)


class Key:
    """a pool's two verification keys (any 32 bytes: the rule only hashes them)"""

    def __init__(self, rng):
        self.cold = rng.bytes(32)
        self.vrf = rng.bytes(32)
        self.id = L.pool_id(self.cold)
        self.vrf_hash = L.vrf_key_hash(self.vrf)

    def pool(self, sigma, vrf_hash=None):
        return L.Pool(self.id, vrf_hash or self.vrf_hash, sigma)


def _sigma(rng):
    den = int(rng.integers(1, 2**63))
    return (int(rng.integers(0, den + 1)), den)


def _beta(rng):
    """a leader output: uniform, or small enough that a middling stake wins"""
    b = bytearray(rng.bytes(64))
    z = int(rng.integers(0, 4))
    b[:z] = bytes(z)
    return bytes(b)


def _key_with(rng, pred):
    while True:
        k = Key(rng)
        if pred(k.id):
            return k


@functools.lru_cache(maxsize=None)
def main_views():
    """Entries with 0, 1, 2, 3, 1,025, 1 and 6 pools and d = 0, 1/2, 3/10, a
    63-bit fraction, 0, 1, 0.  Entry 6 holds ids that differ from a real pool's
    only in byte 0 or only in byte 27, and a 0x7f / 0x80 pair in byte 0; one
    pool is in entries 2 and 4 with different stake and VRF hash.  Returns
    (views, keys per entry)."""
    rng = np.random.default_rng(4242)
    sizes = [0, 1, 2, 3, 1025, 1]
    ds = [(0, 1), (1, 2), (3, 10), D63, (0, 7), (1, 1), (0, 1)]
    keys = [[Key(rng) for _ in range(s)] for s in sizes]
    dup = keys[2][0]
    keys[4][0] = dup
    entries = []
    for j, ks in enumerate(keys):
        pools = [k.pool(_sigma(rng)) for k in ks]
        if j == 4:  # the shared pool again, registered with another VRF key and stake
            pools[0] = dup.pool((1, 3), vrf_hash=L.vrf_key_hash(b"another key" + bytes(21)))
        entries.append(L.Entry(1000 * j, ds[j], tuple(pools)))
    # entry 6: neighbours in the order that differ in one byte only
    a = _key_with(rng, lambda i: 0 < i[27] < 255 and 0 < i[0] < 255)
    s7f = _key_with(rng, lambda i: i[0] == 0x7f)
    ghosts = [bytes([a.id[0] - 1]) + a.id[1:], bytes([a.id[0] + 1]) + a.id[1:],
              a.id[:27] + bytes([a.id[27] - 1]), a.id[:27] + bytes([a.id[27] + 1]),
              b"\x80" + s7f.id[1:]]
    pools = [a.pool((1, 2)), s7f.pool((2, 3))] + [L.Pool(g, bytes(32), (1, 5)) for g in ghosts]
    entries.append(L.Entry(6000, ds[6], tuple(pools)))
    keys.append([a, s7f])
    return L.LedgerViews(entries), keys


def _row(key_cold, key_vrf, slot, beta, c0, counter=0):
    return (key_cold, key_vrf, int(slot), beta, int(c0), int(counter))


@functools.lru_cache(maxsize=None)
def main_rows():
    """About 2,000 rows over main_views: every pool of the small entries and the
    first, last and random rows of the large one, right and wrong VRF keys,
    unknown issuers, 40 consecutive slots from each entry's first, the slot
    at and below each boundary, the period edges."""
    views, keys = main_views()
    rng = np.random.default_rng(777)
    rows = []
    stranger = Key(rng)
    for j, e in enumerate(views.entries):
        ks = {k.id: k for k in keys[j]}
        order = [ks[p.pool_id] for p in e.pools if p.pool_id in ks]
        pick = order if len(order) <= 8 else \
            [order[0], order[1], order[-2], order[-1]] + \
            [order[int(i)] for i in rng.integers(0, len(order), 400)]
        # 40 consecutive slots from the entry's first, and the slot below it
        for s in range(40):
            k = pick[s % len(pick)] if pick else stranger
            rows.append(_row(k.cold, k.vrf, e.first_slot + s, _beta(rng), (e.first_slot + s) // SPKP))
        if j:
            k = pick[0] if pick else stranger
            rows.append(_row(k.cold, k.vrf, e.first_slot - 1, _beta(rng), e.first_slot // SPKP - 1))
        for k in pick:
            slot = e.first_slot + int(rng.integers(0, 1000))
            kp = slot // SPKP
            rows.append(_row(k.cold, k.vrf, slot, _beta(rng), kp))
            rows.append(_row(k.cold, stranger.vrf, slot, _beta(rng), kp))      # wrong VRF key
            rows.append(_row(stranger.cold, k.vrf, slot, _beta(rng), kp))      # unknown issuer
            # a pool of another entry is unknown here
            other = keys[(j + 1) % len(keys)]
            if other:
                rows.append(_row(other[-1].cold, other[-1].vrf, slot, _beta(rng), kp))
    # the period edges, on a slot that is no overlay slot (entry 6, d = 0)
    k = keys[6][0]
    for slot in (123456, 2**64 - 1):
        kp = slot // SPKP
        for c0 in (kp + 1, kp, kp - 1, kp - MAX_EVO + 1, kp - MAX_EVO, 0, 2**64 - MAX_EVO,
                   2**64 - MAX_EVO + 1, 2**64 - 1):
            rows.append(_row(k.cold, k.vrf, slot, _beta(rng), c0))
    # the same on an overlay slot (entry 5, d = 1): only the period is evaluated
    k = keys[5][0]
    for c0 in (51, 50, 0):
        rows.append(_row(k.cold, k.vrf, 5050, _beta(rng), c0))
    # far slots: the last entry applies
    for k in keys[6]:
        rows.append(_row(k.cold, k.vrf, 2**64 - 1, _beta(rng), (2**64 - 1) // SPKP))
        rows.append(_row(k.cold, k.vrf, 2**40, bytes(64), 2**40 // SPKP))
    return rows


def columns(rows):
    """rows -> the SoA arrays (issuer_vk, vrf_vk, slot, leader_output, c0, counter)"""
    n = len(rows)
    iv = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(n, 32).copy()
    vv = np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(n, 32).copy()
    lo = np.frombuffer(b"".join(r[3] for r in rows), np.uint8).reshape(n, 64).copy()
    return (iv, vv, np.array([r[2] for r in rows], np.uint64), lo,
            np.array([r[4] for r in rows], np.uint64), np.array([r[5] for r in rows], np.uint64))


def expect(views, g, rows):
    out = [L.rule(views, g, r[0], r[1], r[2], r[3], r[4], oracle=OL) for r in rows]
    return np.array([b for b, _ in out], np.uint8), np.array([r for _, r in out], np.uint32)


@functools.lru_cache(maxsize=None)
def main_expect():
    """(bits, rows) of main_rows under G_MAIN, computed once"""
    return expect(main_views()[0], G_MAIN, main_rows())


def views_k(k):
    """k entries, first_slot = 0, 10, 20, ..., each with the same two pools"""
    rng = np.random.default_rng(50 + k)
    ks = [Key(rng), Key(rng)]
    entries = [L.Entry(10 * j, (0, 1), tuple(x.pool((1 + j % 3, 3 + j % 5)) for x in ks))
               for j in range(k)]
    return L.LedgerViews(entries), ks


# ---- a signed, linked chain of four pools -------------------------------------------
def pool_keys(i):
    """pool i's cold and VRF key pairs (the oracle's, from fixed seeds)"""
    import oracle_ffi as O

    cold_pk, cold_sk = O.ed25519_keypair(bytes([0x40 + i]) * 32)
    vrf_pk, vrf_sk = O.vrf_keypair(bytes([0x60 + i]) * 32)
    return cold_pk, cold_sk, vrf_pk, vrf_sk


def signed_chain4(prev, slots, first_block_no, nonces, pool_of, counters, spkp=SPKP):
    """envelope_cases.signed_chain with header i forged by pool pool_of[i] (its
    own cold and VRF keys) under OCERT counter counters[i].  Returns (raws,
    last hash)."""
    import envelope_cases as EC
    import hdr_cases as C
    import oracle_ffi as O
    from ouroboros_network_amd import header as H

    fields0, _ = EC._tpraos_parts()
    kes_seed = b"\x05" * 32
    hot = O.kes_keygen(kes_seed)
    out, h = [], prev
    for i, (slot, nonce) in enumerate(zip(slots, nonces)):
        slot = int(slot)
        cold_pk, cold_sk, vrf_pk, vrf_sk = pool_keys(pool_of[i])
        t = i % 60
        c0 = max(0, slot // spkp - t)
        t = slot // spkp - c0
        counter = int(counters[i])
        sigma = O.ed25519_sign(cold_sk, hot + counter.to_bytes(8, "big") + c0.to_bytes(8, "big"))
        certs = []
        for uc in (H.SEED_ETA, H.SEED_L):
            pi = O.vrf_prove(vrf_sk, O.mk_seed(uc, slot, nonce))
            certs.append(b"\x82" + C.cbor_bytes(O.vrf_proof_to_hash(pi)) + C.cbor_bytes(pi))
        f = list(fields0)
        f[0], f[1] = C.cbor_uint(first_block_no + i), C.cbor_uint(slot)
        f[2] = C.cbor_bytes(h) if len(h) == 32 else h
        f[3], f[4] = C.cbor_bytes(cold_pk), C.cbor_bytes(vrf_pk)
        f[5], f[6], f[9] = certs[0], certs[1], C.cbor_bytes(hot)
        f[10], f[11], f[12] = C.cbor_uint(counter), C.cbor_uint(c0), C.cbor_bytes(sigma)
        body = C._cbor_head(4, 15) + b"".join(f)
        sig = O.kes_sign(kes_seed, min(t, 63), body)
        out.append(C.wire_header(f, sig, era=(2 if i % 3 == 0 else None)))
        h = EC.b2b(b"\x82" + body + C.cbor_bytes(sig))
    return out, h


N_BYRON, N_TPRAOS = 250, 40
G_CHAIN = L.Globals(SPKP, MAX_EVO, -8 * RES)  # f = 1 - e^-8: a whole stake almost always leads


@functools.lru_cache(maxsize=None)
def chain_stream():
    """250 Byron headers (chunk 0 of 256 is mixed), then 40 signed, linked TPraos
    headers over three epochs forged by pools 0..3 and by pool 4, which no view
    knows; pool 1 is registered with a wrong VRF hash in the middle epoch, pool
    3 has a stake of 2^-60; in the middle epoch d = 1/20 makes every other
    header's slot an overlay slot.  Pool 0's counter falls once inside chunk 1 and
    pool 2's falls across the chunk boundary (header 255 -> 256).  Returns a
    dict: raws, epochs, views, counters, and the rows of the TPraos headers."""
    import envelope_cases as EC
    from ouroboros_network_amd import envelope as E
    from ouroboros_network_amd import header as H
    from ouroboros_network_amd.tpraos import EpochNonces

    byron = EC.good_chain(N_BYRON, 0, ebb_every=9, extra_step=11)
    last = E.header_record(byron[-1], EC.VAL_CFG)
    base = last.slot + 1
    slots = [base + 10 * i for i in range(N_TPRAOS)]
    first = [0, base + 100, base + 250]
    eta = [None, b"\x33" * 32, b"\x77" * 32]
    nonce_of = lambda s: eta[max(j for j, f in enumerate(first) if f <= s)]  # noqa: E731
    pool_of = [(0, 1, 2, 3, 0, 2, 4, 1)[i % 8] for i in range(N_TPRAOS)]
    pool_of[5], pool_of[6] = 2, 2      # headers 255 and 256 of the stream: pool 2
    counters = [10 + i // 8 for i in range(N_TPRAOS)]
    counters[5], counters[6] = 9, 8    # falls across the chunk boundary
    counters[20] = 3                   # pool 0 falls inside chunk 1
    tp, _ = signed_chain4(last.hash, slots, last.block_no + 1, [nonce_of(s) for s in slots],
                          pool_of, counters)
    ids = []
    for i in range(5):
        cold_pk, _, vrf_pk, _ = pool_keys(i)
        ids.append((L.pool_id(cold_pk), L.vrf_key_hash(vrf_pk)))
    sig = [(1, 1), (1, 1), (1, 2), (1, 2**60)]
    entries = []
    for j, f in enumerate(first):
        pools = [L.Pool(ids[i][0], ids[i][1] if (i, j) != (1, 1) else b"\x01" * 32, sig[i])
                 for i in range(4)]
        entries.append(L.Entry(f, [(0, 1), (1, 20), (0, 1)][j], tuple(pools)))
    views = L.LedgerViews(entries)
    rows = []
    for r in tp:
        h = H.parse_header(r)
        rows.append(_row(h.issuer_vk, h.vrf_vk, h.slot, h.leader_output, h.ocert_kes_period,
                         h.ocert_counter))
    known = {ids[0][0]: 10, ids[2][0]: 7}       # pool 1 and 3: in the table, no counter yet
    return dict(raws=byron + tp, n_byron=len(byron),
                epochs=EpochNonces(first_slot=first, nonce=[n or bytes(32) for n in eta],
                                   neutral=[n is None for n in eta]),
                views=views, rows=rows, known=known,
                table_ids=[i[0] for i in ids[:4]] + [b"\xfe" * 28])


def chain_expect(s):
    """(ledger, pool_row, counters after) of the whole stream, in Python"""
    bits, rows = expect(s["views"], G_CHAIN, s["rows"])
    bits, known = L.fold_rule(s["views"], bits, rows, [r[5] for r in s["rows"]], s["known"])
    nb = s["n_byron"]
    return (np.concatenate([np.zeros(nb, np.uint8), bits]),
            np.concatenate([np.full(nb, L.LV_NO_POOL, np.uint32), rows]), known)
