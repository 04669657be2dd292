"""Shared inputs and the plain-Python restatement for the forging-side tests
(test_prove_rule.py, test_leader_schedule.py, test_gpu_leader_schedule.py):
checkIsLeader (Shelley/Protocol.hs:366-413) restated as oracle_ffi.mk_seed ->
oracle_ffi.vrf_prove -> vrf_proof_to_hash -> oracle/leader.py
check_leader_value, with ledger.py's overlay rule for d > 0.  The oracle is the
checker here, never the thing under test.  Every oracle proof is computed once
and shared (functools.lru_cache)."""
import ctypes
import functools
import importlib.util
import os
from fractions import Fraction

import numpy as np

import oracle_ffi as O
from ouroboros_network_amd import _native
from ouroboros_network_amd import ledger as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("oracle_leader_forge",
                                               os.path.join(ROOT, "oracle", "leader.py"))
OL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(OL)

# alpha lengths across the SHA-512 padding and block boundaries of the 34-byte
# prefix (34 + 77 = 111 is the last one-block message; 34 + 94 = 128)
ALPHA_LENS = [0, 1, 32, 111, 112, 127, 128, 300, 77, 78, 93, 94, 95]
ISSUE_LENS = ALPHA_LENS[:8]

NO_POOL = 0xFFFFFFFF
ETA0 = bytes((7 * i + 3) & 0xFF for i in range(32))
FIRST_SLOT = 4_492_937          # arbitrary, odd, no multiple of anything below
L_HALF = OL.active_slot_log(Fraction(1, 2))
SEED_L = O.mk_nonce_from_number(1)
SEED_ETA = O.mk_nonce_from_number(0)


@functools.lru_cache(maxsize=None)
def keys(n=200, seed=20261021):
    """n seeded (pk, sk) pairs from the oracle's key generation."""
    rng = np.random.default_rng(seed)
    return [O.vrf_keypair(rng.bytes(32)) for _ in range(n)]


def pool_key():
    return keys()[0][1]


def prove_inputs(n, lens=ISSUE_LENS, seed=5):
    """n alphas, lengths cycling through `lens`, laid out so that the spans'
    byte alignments cycle through 0..3; returns (alphas, buf, off, len) with
    the last span ending at the last byte of buf."""
    rng = np.random.default_rng(seed)
    alphas = [rng.bytes(lens[i % len(lens)]) for i in range(n)]
    # (item i = q len(lens) + k gets alignment (k + q) % 4: every length meets every alignment)
    parts, off, at = [], np.zeros(n, np.uint64), 0
    for i, a in enumerate(alphas):
        want = (i + i // len(lens)) % 4
        pad = (want - at) % 4
        parts.append(b"\xa5" * pad)
        at += pad
        off[i] = at
        parts.append(a)
        at += len(a)
    buf = np.frombuffer(b"".join(parts), np.uint8).copy() if at else np.zeros(0, np.uint8)
    ln = np.array([len(a) for a in alphas], np.uint32)
    return alphas, buf, off, ln


@functools.lru_cache(maxsize=None)
def oracle_prove(sk: bytes, alpha: bytes):
    pi = O.vrf_prove(sk, alpha)
    return pi, O.vrf_proof_to_hash(pi)


def prove_raw(n, sk_rows, nkeys, buf, off, ln, host, want_beta=True, lib=None):
    """The C entry itself: (rc, proof (n, 80), beta (n, 64))."""
    lib = lib or _native.load()
    sk = np.frombuffer(b"".join(sk_rows), np.uint8).copy()
    proof = np.zeros((n, 80), np.uint8)
    beta = np.zeros((n, 64), np.uint8)
    fn = lib.ouro_vrf03_prove_batch_host if host else lib.ouro_vrf03_prove_batch
    rc = fn(n, O.p(sk), nkeys, O.p(buf) if buf.size else None, buf.size, O.p(off), O.p(ln),
            O.p(proof), O.p(beta) if want_beta else None)
    return rc, proof, beta


def mk_alpha(slot: int, eta0, leader: bool) -> bytes:
    return O.mk_seed(SEED_L if leader else SEED_ETA, slot, eta0)


# ---- the schedule's parameter sets --------------------------------------------
def param_sets(n=300):
    half = Fraction(1, 2)
    base = dict(eta0=ETA0, first_slot=FIRST_SLOT, sigma=half, L=L_HALF, f_is_one=False,
                d=Fraction(0), asc_inv=0, ngen=0, epoch_first_slot=0)
    sets = {
        "half": {},
        "sigma0": dict(sigma=Fraction(0)),
        "f_is_one": dict(f_is_one=True),
        "neutral": dict(eta0=None),
        "overlay": dict(d=half, asc_inv=20, ngen=7, epoch_first_slot=FIRST_SLOT - 1_237),
        "d_one": dict(d=Fraction(1), asc_inv=20, ngen=7, epoch_first_slot=FIRST_SLOT - 1_237),
        "slot0": dict(first_slot=0),
        "slot_max": dict(first_slot=2**64 - n),
    }
    return {k: dict(base, **v) for k, v in sets.items()}


def params_c(ps):
    """(LeaderParamsC, keepalive) of a parameter set."""
    nonce = None if ps["eta0"] is None else np.frombuffer(ps["eta0"], np.uint8).copy()
    L = ps["L"] & ((1 << 128) - 1)
    lo, hi = L & ((1 << 64) - 1), L >> 64
    if hi >= 1 << 63:
        hi -= 1 << 64
    p = _native.LeaderParamsC(
        epoch_nonce=None if nonce is None else O.p(nonce),
        epoch_first_slot=ps["epoch_first_slot"], sigma_num=ps["sigma"].numerator,
        sigma_den=ps["sigma"].denominator, act_log_hi=hi, act_log_lo=lo,
        f_is_one=1 if ps["f_is_one"] else 0, d_num=ps["d"].numerator, d_den=ps["d"].denominator,
        asc_inv=ps["asc_inv"], ngen=ps["ngen"])
    return p, nonce


def sched_raw(sk, ps, n, host, want_gen=True, want_beta=True, first_slot=None, lib=None):
    """The C entry itself: (rc, cls, gen_index, beta)."""
    lib = lib or _native.load()
    p, keep = params_c(ps)
    cls = np.full(n, 0xEE, np.uint8)
    gen = np.full(n, 0xEEEEEEEE, np.uint32)
    beta = np.zeros((n, 64), np.uint8)
    fn = lib.ouro_tpraos_leader_schedule_host if host else lib.ouro_tpraos_leader_schedule
    fs = ps["first_slot"] if first_slot is None else first_slot
    rc = fn(sk, ctypes.byref(p), ctypes.c_uint64(fs), n, O.p(cls),
            O.p(gen) if want_gen else None, O.p(beta) if want_beta else None)
    del keep
    return rc, cls, gen, beta


def restate(sk, ps, n, first_slot=None):
    """checkIsLeader for n slots, in plain Python over the oracle."""
    fs = ps["first_slot"] if first_slot is None else first_slot
    d = (ps["d"].numerator, ps["d"].denominator)
    cls = np.zeros(n, np.uint8)
    gen = np.full(n, NO_POOL, np.uint32)
    beta = np.zeros((n, 64), np.uint8)
    for i in range(n):
        slot = fs + i
        b = oracle_prove(sk, mk_alpha(slot, ps["eta0"], True))[1]
        beta[i] = np.frombuffer(b, np.uint8)
        if d[0] and LG.is_overlay_slot(ps["epoch_first_slot"], d, slot):
            ix = LG.classify_overlay_slot(ps["epoch_first_slot"], d, ps["asc_inv"], ps["ngen"],
                                          slot)
            cls[i] = 3 if ix is None else 2
            if ix is not None:
                gen[i] = ix
        else:
            cls[i] = 1 if OL.check_leader_value(b, ps["sigma"], ps["L"], ps["f_is_one"]) else 0
    return cls, gen, beta


def vrfs_raw(sk, eta0, slots, host, lib=None):
    """The C entry itself: (rc, eta_proof, eta_output, leader_proof, leader_output)."""
    lib = lib or _native.load()
    slot = np.asarray(slots, np.uint64).copy()
    m = slot.shape[0]
    nonce = None if eta0 is None else np.frombuffer(eta0, np.uint8).copy()
    ep, lp = np.zeros((m, 80), np.uint8), np.zeros((m, 80), np.uint8)
    eo, lo = np.zeros((m, 64), np.uint8), np.zeros((m, 64), np.uint8)
    fn = lib.ouro_tpraos_leader_vrfs_host if host else lib.ouro_tpraos_leader_vrfs
    rc = fn(sk, None if nonce is None else O.p(nonce), m, O.p(slot) if m else None, O.p(ep),
            O.p(eo), O.p(lp), O.p(lo))
    return rc, ep, eo, lp, lo


def check_vrfs(sk, eta0, slots, got):
    """Both proofs and outputs of every slot against the oracle's."""
    rc, ep, eo, lp, lo = got
    assert rc == 0
    for j, s in enumerate(slots):
        we, wl = oracle_prove(sk, mk_alpha(int(s), eta0, False)), \
            oracle_prove(sk, mk_alpha(int(s), eta0, True))
        assert bytes(ep[j]) == we[0] and bytes(eo[j]) == we[1], j
        assert bytes(lp[j]) == wl[0] and bytes(lo[j]) == wl[1], j
