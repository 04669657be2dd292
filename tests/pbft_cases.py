"""Cases for the Byron ledger-view checks (tests/test_pbft_rule.py,
test_pbft_asan.py, test_gpu_pbft.py).

Expected values never come from the code under test: ids are hashlib's
(pbft.key_hash), verdicts are pbft.pbft_rule's -- bisect, a deque and a dict
following PBFT/State.hs.  Everything is built once per process and shared,
and nothing here is changed after it is built.
"""
import functools
import json
import os

import numpy as np

from ouroboros_network_amd import pbft as P

HERE = os.path.dirname(os.path.abspath(__file__))
OK, ECBOR, EBB, ESHELLEY = 0, 1, 6, 7   # OURO_PACK_*: regular, unsliced, boundary, TPraos


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "reference_pbft.json")) as f:
        return json.load(f)


def golden_views(window=5, threshold=2):
    """the golden ledger state's delegation map as a one-entry schedule"""
    pairs = [(bytes.fromhex(d), bytes.fromhex(g)) for g, d in golden()["delegation_map"]]
    return P.PBftViews([(0, pairs)], window, threshold)


@functools.lru_cache(maxsize=None)
def keys(n, seed=1):
    """n seeded XPubs (n x 64) and their ids by hashlib"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    ids = [P.key_hash(k[i].tobytes()) for i in range(n)]
    k.setflags(write=False)
    return k, ids


def gen_id(i):
    """the id of genesis key i (any 28 distinct bytes serve: the lookup never hashes it)"""
    return bytes([0xA0 + i]) * 28


# slots at which the entries of a k-entry schedule begin
FIRST = (0, 1000, 2000)


@functools.lru_cache(maxsize=None)
def schedule(ngen, k, window, threshold):
    """ngen genesis keys over k entries.  Entry 0: genesis i -> delegate i.
    Entry 1: genesis 0 moves to a NEW delegate (key ngen); its old delegate is
    nobody's.  Entry 2: that old delegate (key 0) comes back as the delegate of
    the LAST genesis key, whose own delegate leaves -- the same delegate id
    maps to another genesis key than in entry 0 (for ngen = 1: to the same)."""
    _, ids = keys(16)
    maps = [{i: i for i in range(ngen)}]          # genesis index -> key index
    if k > 1:
        m = dict(maps[0])
        m[0] = ngen
        maps.append(m)
    if k > 2:
        m = dict(maps[1])
        m[ngen - 1] = 0
        maps.append(m)
    entries = [(FIRST[j], [(ids[d], gen_id(g)) for g, d in m.items()])
               for j, m in enumerate(maps[:k])]
    return P.PBftViews(entries, window, threshold)


@functools.lru_cache(maxsize=None)
def rows(n, ngen, k, seed):
    """n rows over the span of a k-entry schedule: delegates of every entry
    (known in one entry, unknown in another), keys no entry knows, EBBs,
    TPraos and unsliced rows; slots mostly ascending, with repeats and an
    occasional step back.  Returns (delegate_vk n x 64, slot, status)."""
    rng = np.random.default_rng(seed)
    kk, _ = keys(16)
    vk = np.zeros((n, 64), np.uint8)
    slot = np.zeros(n, np.uint64)
    status = np.zeros(n, np.uint8)
    s = 0
    span = FIRST[k - 1] + 1000
    for i in range(n):
        u = rng.random()
        status[i] = OK if u < 0.70 else EBB if u < 0.80 else ESHELLEY if u < 0.90 else ECBOR
        v = rng.random()
        # a delegate of some entry (keys 0 .. ngen), or a key nobody delegates to
        vk[i] = kk[int(rng.integers(0, ngen + 1))] if v < 0.85 else kk[int(rng.integers(9, 16))]
        w = rng.random()
        step = 0 if w < 0.15 else -int(rng.integers(1, 4)) if w < 0.25 else int(
            rng.integers(1, max(2, 3 * span // n)))
        s = max(0, s + step)
        slot[i] = s
    for a in (vk, slot, status):
        a.setflags(write=False)
    return vk, slot, status


def mixed_wave(ngen=3, k=3):
    """64 rows, one wave, every outcome in it: known and unknown delegates of
    each entry, a boundary row, a TPraos row, an unsliced row"""
    kk, _ = keys(16)
    vk = np.zeros((64, 64), np.uint8)
    slot = np.zeros(64, np.uint64)
    status = np.zeros(64, np.uint8)
    for i in range(64):
        vk[i] = kk[i % (ngen + 1)] if i % 5 else kk[9 + i % 7]
        slot[i] = FIRST[(i // 8) % k] + i
        status[i] = (OK, OK, OK, EBB, OK, ESHELLEY, OK, ECBOR)[i % 8]
    return vk, slot, status


def tile(arrs, n):
    """the first n rows of the arrays repeated"""
    m = arrs[0].shape[0]
    reps = (n + m - 1) // m
    return tuple(np.ascontiguousarray(np.concatenate([a] * reps)[:n]) for a in arrs)


def outcome(bits, status):
    """the name of a row's outcome from its bits (after a fold) and its status"""
    b = int(bits)
    if status == ESHELLEY:
        return "tpraos"
    if status == ECBOR:
        return "unsliced"
    if b & P.PBFT_BOUNDARY:
        return "boundary"
    if b == 0:
        return "unknown_delegate"
    if not b & P.PBFT_SLOT_OK:
        return "slot_back"
    if not b & P.PBFT_WINDOW_OK:
        return "over_threshold"
    return "all_ok"


# ---- signed Byron chains for the chain entry -------------------------------------
# ByronDSIGN verifies a plain Ed25519 signature under XPub[0:32], so the
# oracle's ed25519_sign over the slicer's message makes valid headers for test
# keys.  CHAIN_CFG: short Byron epochs, so a chain of a few hundred headers
# spans several of them.

def chain_cfg():
    from ouroboros_network_amd import envelope as E

    return E.Cfg(100)


@functools.lru_cache(maxsize=None)
def chain_keys(n=4):
    """n delegates: (XPub, signing key) -- an Ed25519 key and 32 bytes of chain
    code -- and their ids by hashlib"""
    import oracle_ffi as O

    out = []
    for i in range(n):
        pk, sk = O.ed25519_keypair(bytes([0x40 + i]) * 32)
        xpub = pk + bytes([0xC0 + i]) * 32
        out.append((xpub, sk, P.key_hash(xpub)))
    return out


def chain_views(window, threshold, ndlg=3):
    """delegates 0 .. ndlg - 1 of chain_keys for genesis keys 0 .. ndlg - 1 (the
    last key of chain_keys is nobody's delegate)"""
    ks = chain_keys()
    return P.PBftViews([(0, [(ks[i][2], gen_id(i)) for i in range(ndlg)])], window, threshold)


def byron_signed(prev, epoch, in_epoch, block_no, who, form=1):
    """(wire header, its hash): a regular Byron header of delegate `who` of
    chain_keys, its block signature valid under the header's own magic"""
    import hdr_cases as C
    import envelope_cases as EC
    import oracle_ffi as O
    from ouroboros_network_amd import byron as B

    xpub, sk, _ = chain_keys()[who]
    gx = bytes([0x10 + who]) * 64   # the certificate's issuer: part of the message, not a key we use
    magic, proof, _, _ = EC._regular_parts()
    arr, u, bs = EC.arr, C.cbor_uint, C.cbor_bytes
    extra = arr(arr(u(1), u(0), u(0)), arr(bs(b"cardano-sl"), u(1)), C._cbor_head(5, 0),
                bs(bytes(32)))

    def item(sig):
        cert = arr(u(0), bs(gx), bs(xpub), bs(bytes(64)))
        cons = arr(arr(u(epoch), u(in_epoch)), bs(gx), arr(u(block_no)),
                   arr(u(2), arr(cert, bs(sig))))
        return arr(magic, bs(prev), proof, cons, extra)

    msg = B.parse_byron_header(EC.byron_wire(1, item(bytes(64)), form)).message(B.HEADER_MAGIC)
    it = item(O.ed25519_sign(sk, msg))
    return EC.byron_wire(1, it, form), EC.b2b(b"\x82\x01" + it)


def byron_chain(spec, prev=bytes(32), block_no=0):
    """raw headers of a linked chain: spec items ("r", epoch, in_epoch, who) or
    ("e", epoch)"""
    import envelope_cases as EC

    raws = []
    for it in spec:
        if it[0] == "e":
            raw, prev = EC.byron_ebb(prev, it[1], block_no)
        else:
            block_no += 1
            raw, prev = byron_signed(prev, it[1], it[2], block_no, it[3], form=1 + len(raws) % 3)
        raws.append(raw)
    return raws


def expect_pbft(raws, views, cfg, state):
    """pbft_rule over a raw chain: the Python Byron slicer's status and
    delegate key, the Python envelope record's slot; a TPraos header is status
    ESHELLEY to the rule"""
    from ouroboros_network_amd import byron as B
    from ouroboros_network_amd import envelope as E
    from ouroboros_network_amd import header as H

    vk, slot, status = [], [], []
    for raw in raws:
        st, h, s = ESHELLEY, None, 0
        if H.era_class(raw) == H.PROTO_PBFT:
            st, h = B.byron_status(raw)
            rec = E.header_record(raw, cfg)
            s = rec.slot if rec is not None else 0
        vk.append(h.delegate_xpub if h is not None else bytes(64))
        slot.append(s)
        status.append(st)
    return P.pbft_rule(views, vk, slot, status, state)


def trivial_ledger():
    """the ledger views a pure Byron chain needs beside it: one entry, no pools"""
    import ledger_cases as LC
    from ouroboros_network_amd import ledger as L

    return L.LedgerViews([L.Entry(0, (0, 1), ())]), LC.G_CHAIN, LC.SPKP


@functools.lru_cache(maxsize=None)
def chain3():
    """A pure Byron chain of 3 x 256 headers for 256-header chunks under window
    300, threshold 120, three delegates: header 256 (the second chunk's first)
    and header 512 are EBBs; delegates take turns 0, 1, 2 up to header 210, then
    delegate 0 signs every header of 211 .. 340 but a few -- its count passes
    120 a little after the chunk boundary at 256, from signatures on both sides
    of it -- and turns again after that; the window is full at its 300th signer,
    inside the second chunk.  Header 700 is signed by a key nobody delegated to."""
    spec, e, s = [], 0, 0
    for i in range(768):
        s += 1
        if s >= 100:
            e, s = e + 1, 0
        if i in (256, 512):
            spec.append(("e", e))
            continue
        who = 3 if i == 700 else (0 if 210 < i <= 340 and i % 9 else i % 3)
        spec.append(("r", e, s, who))
    return tuple(byron_chain(spec))
