"""Ledger-view header checks -- what ``SL.updateChainDepState``
(ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:433-442)
checks with the epoch's ``LedgerView`` beside the signatures: ledger-specs'
OVERLAY rule (the issuer is a registered pool, its VRF key is the registered
one, its leader value is below the threshold for ITS stake) and OCERT rule (the
certificate's KES period bounds, the per-pool counter).  With a
``GenesisDelegs`` schedule the OVERLAY rule's other branch runs on overlay
slots: ``classify_overlay_slot`` (ledger-specs lookupInOverlaySchedule), the
scheduled genesis key's delegate and its VRF key hash (pbftVrfChecks), and the
delegate's counter.

``ledger_checks`` / ``counter_fold`` call the library (``csrc/ledger_view.h``,
``k_ledger_checks``, ``ouro_ocert_counter_fold``); there is no CPU fallback
other than the library's own host path.  ``rule`` / ``fold_rule`` restate the
same rules in plain Python -- hashlib for the two hashes, bisect for the lookup,
``oracle/leader.py`` for the threshold, a dict for the counters -- for the
tests' expected side; nothing in them comes from the library.

Pinned by the reference's fixtures (tests/test_ledger_rule.py): hashKey =
Blake2b-224 and hashVerKeyVRF = Blake2b-256.  NOT pinned by anything in the
reference tree: isOverlaySlot's formula and classifyOverlaySlot's arithmetic
(ledger-specs is un-vendored; the reference shows only the call and the shape
of its result, Shelley/Protocol.hs:366-406) and, as for leader.py,
checkLeaderValue.
"""
from __future__ import annotations

import bisect
import ctypes
import hashlib
import importlib.util
import os
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from ._native import (LV_ALL_OK, LV_BADARG, LV_COUNTER_OK, LV_KES_PERIOD_OK, LV_LEADER_OK,
                      LV_NO_POOL, LV_OVERLAY, LV_OVERLAY_ACTIVE, LV_POOL_KNOWN, LV_VRF_KEY_OK)
from ._pack import ptr

__all__ = ["LedgerViews", "Globals", "Counters", "GenesisDelegs", "GenDeleg", "ledger_checks",
           "counter_fold", "rule", "fold_rule", "pool_id", "vrf_key_hash", "is_overlay_slot",
           "classify_overlay_slot", "LV_ALL_OK", "LV_BADARG", "LV_COUNTER_OK", "LV_KES_PERIOD_OK",
           "LV_LEADER_OK", "LV_NO_POOL", "LV_OVERLAY", "LV_OVERLAY_ACTIVE", "LV_POOL_KNOWN",
           "LV_VRF_KEY_OK"]


@dataclass(frozen=True)
class Pool:
    """One row of an entry's pool distribution."""

    pool_id: bytes            # 28: hashKey of the cold key
    vrf_hash: bytes           # 32: hashVerKeyVRF of the registered VRF key
    sigma: Tuple[int, int]    # relative stake, numerator / denominator


@dataclass(frozen=True)
class Entry:
    """The ledger view from ``first_slot`` on (taken as its epoch's first
    slot): the decentralisation parameter d and the pool distribution."""

    first_slot: int
    d: Tuple[int, int]
    pools: Tuple[Pool, ...]


class LedgerViews:
    """A ledger-view schedule (``ouro_ledger_views``): entries by ascending
    first_slot, the first at slot 0.  Pools are sorted by id here; everything
    else is passed as given, so that the library's own checks can be tested."""

    def __init__(self, entries: Sequence[Entry], sort: bool = True):
        self.entries = [Entry(e.first_slot, tuple(e.d),
                              tuple(sorted(e.pools, key=lambda p: p.pool_id) if sort else e.pools))
                        for e in entries]
        k = len(self.entries)
        rows = [p for e in self.entries for p in e.pools]
        self.first_slot = np.array([e.first_slot for e in self.entries], np.uint64)
        self.d_num = np.array([e.d[0] for e in self.entries], np.uint64)
        self.d_den = np.array([e.d[1] for e in self.entries], np.uint64)
        self.pool_begin = np.zeros(k + 1, np.uint32)
        for j, e in enumerate(self.entries):
            self.pool_begin[j + 1] = self.pool_begin[j] + len(e.pools)
        m = max(len(rows), 1)
        self.pool_id = np.zeros((m, 28), np.uint8)
        self.vrf_hash = np.zeros((m, 32), np.uint8)
        self.sigma_num = np.zeros(m, np.uint64)
        self.sigma_den = np.ones(m, np.uint64)
        for r, p in enumerate(rows):
            self.pool_id[r] = np.frombuffer(p.pool_id, np.uint8)
            self.vrf_hash[r] = np.frombuffer(p.vrf_hash, np.uint8)
            self.sigma_num[r], self.sigma_den[r] = p.sigma
        self.rows = len(rows)

    def c_struct(self) -> _native.LedgerViewsC:
        return _native.LedgerViewsC(len(self.entries), *(a.ctypes.data for a in (
            self.first_slot, self.d_num, self.d_den, self.pool_begin, self.pool_id, self.vrf_hash,
            self.sigma_num, self.sigma_den)))

    def all_pool_ids(self) -> List[bytes]:
        return sorted({p.pool_id for e in self.entries for p in e.pools})


@dataclass(frozen=True)
class Globals:
    """``ouro_ledger_globals``: slotsPerKESPeriod, maxKESEvo and the
    ActiveSlotCoeff's fields (leader.ActiveSlotCoeff)."""

    slots_per_kes_period: int
    max_kes_evo: int
    un_active_slot_log: int
    f_is_one: bool = False

    def c_struct(self) -> _native.LedgerGlobalsC:
        v = self.un_active_slot_log & ((1 << 128) - 1)
        hi = v >> 64
        if hi >= 1 << 63:
            hi -= 1 << 64
        return _native.LedgerGlobalsC(self.slots_per_kes_period, self.max_kes_evo, hi,
                                      v & ((1 << 64) - 1), 1 if self.f_is_one else 0)


class Counters:
    """The OCERT counters of a chain state (``ouro_ocert_counters``): a table
    of pool ids (sorted here unless sort=False) with a counter where present.
    ``known``: {pool id: counter}; ``ids``: every id the table has a row for."""

    def __init__(self, ids: Sequence[bytes], known: Optional[Dict[bytes, int]] = None,
                 sort: bool = True):
        self.ids = sorted(ids) if sort else list(ids)
        known = known or {}
        m = max(len(self.ids), 1)
        self.pool_id = np.zeros((m, 28), np.uint8)
        self.counter = np.zeros(m, np.uint64)
        self.present = np.zeros(m, np.uint8)
        for i, p in enumerate(self.ids):
            self.pool_id[i] = np.frombuffer(p, np.uint8)
            if p in known:
                self.counter[i], self.present[i] = known[p], 1

    def c_struct(self) -> _native.OcertCountersC:
        return _native.OcertCountersC(len(self.ids), self.pool_id.ctypes.data,
                                      self.counter.ctypes.data, self.present.ctypes.data)

    def as_dict(self) -> Dict[bytes, int]:
        return {p: int(self.counter[i]) for i, p in enumerate(self.ids) if self.present[i]}

    def after(self, counter: np.ndarray, present: np.ndarray) -> "Counters":
        c = Counters(self.ids, sort=False)
        c.counter[:len(self.ids)] = counter[:len(self.ids)]
        c.present[:len(self.ids)] = present[:len(self.ids)]
        return c


@dataclass(frozen=True)
class GenDeleg:
    """One genesis key and the GenDelegPair it maps to."""

    genesis_id: bytes      # 28: hashKey of the genesis key
    delegate_id: bytes     # 28: genDelegKeyHash, the delegate's cold key hash
    delegate_vrf: bytes    # 32: genDelegVrfHash


class GenesisDelegs:
    """A genesis-delegation schedule (``ouro_genesis_delegs``): one tuple of
    GenDeleg per view entry, sorted by genesis id here (Map.keysSet's order)
    unless sort=False, and asc_inv = floor(1 / f)."""

    def __init__(self, entries: Sequence[Sequence[GenDeleg]], asc_inv: int, sort: bool = True):
        self.entries = [tuple(sorted(e, key=lambda x: x.genesis_id) if sort else e)
                        for e in entries]
        self.asc_inv = int(asc_inv)
        k = len(self.entries)
        rows = [x for e in self.entries for x in e]
        self.gen_begin = np.zeros(k + 1, np.uint32)
        for j, e in enumerate(self.entries):
            self.gen_begin[j + 1] = self.gen_begin[j] + len(e)
        m = max(len(rows), 1)
        self.genesis_id = np.zeros((m, 28), np.uint8)
        self.delegate_id = np.zeros((m, 28), np.uint8)
        self.delegate_vrf = np.zeros((m, 32), np.uint8)
        for r, x in enumerate(rows):
            self.genesis_id[r] = np.frombuffer(x.genesis_id, np.uint8)
            self.delegate_id[r] = np.frombuffer(x.delegate_id, np.uint8)
            self.delegate_vrf[r] = np.frombuffer(x.delegate_vrf, np.uint8)
        self.rows = len(rows)

    def c_struct(self) -> _native.GenesisDelegsC:
        return _native.GenesisDelegsC(len(self.entries), self.gen_begin.ctypes.data,
                                      self.genesis_id.ctypes.data, self.delegate_id.ctypes.data,
                                      self.delegate_vrf.ctypes.data, self.asc_inv)

    def all_delegate_ids(self) -> List[bytes]:
        return sorted({x.delegate_id for e in self.entries for x in e})


def _rows(issuer_vk, vrf_vk, slot, leader_output, c0, counter):
    iv = np.ascontiguousarray(issuer_vk, np.uint8).reshape(-1, 32)
    n = iv.shape[0]
    vv = np.ascontiguousarray(vrf_vk, np.uint8).reshape(n, 32)
    sl = np.ascontiguousarray(slot, np.uint64).reshape(n)
    lo = np.ascontiguousarray(leader_output, np.uint8).reshape(n, 64)
    c0 = np.ascontiguousarray(c0, np.uint64).reshape(n)
    ct = None if counter is None else np.ascontiguousarray(counter, np.uint64).reshape(n)
    return n, iv, vv, sl, lo, c0, ct


def ledger_checks(issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, views: LedgerViews,
                  g: Globals, *, ocert_counter=None, counters: Optional[Counters] = None,
                  genesis: Optional[GenesisDelegs] = None, host: bool = False):
    """The ledger-view checks of n sliced TPraos header rows (the columns of a
    HeaderBatch / pack_cbor).  Returns (ledger, pool_row[, counters_after]):
    the LV_* bits and each issuer's view row (LV_NO_POOL: none); with
    ``counters`` (and ocert_counter) the counter fold runs too and the updated
    table is returned.  With ``genesis`` overlay rows take the delegate branch
    (ouro_tpraos_ledger_checks_overlay) and their pool_row is a genesis row.
    host=True: the library's host path."""
    n, iv, vv, sl, lo, c0, ct = _rows(issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period,
                                      ocert_counter)
    ledger = np.zeros(max(n, 1), np.uint8)
    rows = np.zeros(max(n, 1), np.uint32)
    cv, cg = views.c_struct(), g.c_struct()
    cc = co = po = None
    if counters is not None:
        cc = counters.c_struct()
        co, po = np.zeros_like(counters.counter), np.zeros_like(counters.present)
    name = "ouro_tpraos_ledger_checks" + ("_host" if host else "")
    gen = ()
    if genesis is not None:
        name = "ouro_tpraos_ledger_checks_overlay" + ("_host" if host else "")
        c_gen = genesis.c_struct()
        gen = (ctypes.byref(c_gen),)
    rc = getattr(_native.load(), name)(
        n, ptr(iv), ptr(vv), ptr(sl), ptr(lo), ptr(c0), None if ct is None else ptr(ct),
        ctypes.byref(cv), *gen, ctypes.byref(cg), None if cc is None else ctypes.byref(cc),
        None if co is None else ptr(co), None if po is None else ptr(po), ptr(ledger), ptr(rows))
    _native.check(rc, name)
    out = (ledger[:n], rows[:n])
    return out + (counters.after(co, po),) if counters is not None else out


def counter_fold(ledger, pool_row, ocert_counter, views: LedgerViews, counters: Counters,
                 genesis: Optional[GenesisDelegs] = None):
    """``ouro_ocert_counter_fold``: LV_COUNTER_OK into a copy of ``ledger`` in
    stream order and the table afterwards; with ``genesis``
    (``ouro_ocert_counter_fold_overlay``) the delegates' rows too.  Returns
    (ledger, counters_after)."""
    led = np.array(ledger, np.uint8).reshape(-1)
    n = led.shape[0]
    rows = np.ascontiguousarray(pool_row, np.uint32).reshape(n)
    ct = np.ascontiguousarray(ocert_counter, np.uint64).reshape(n)
    cv, cc = views.c_struct(), counters.c_struct()
    co, po = np.zeros_like(counters.counter), np.zeros_like(counters.present)
    buf = led if n else np.zeros(1, np.uint8)
    name, gen = "ouro_ocert_counter_fold", ()
    if genesis is not None:
        name += "_overlay"
        c_gen = genesis.c_struct()
        gen = (ctypes.byref(c_gen),)
    rc = getattr(_native.load(), name)(n, ptr(rows) if n else None, ptr(ct) if n else None,
                                       ctypes.byref(cv), *gen, ctypes.byref(cc), ptr(co), ptr(po),
                                       ptr(buf))
    _native.check(rc, name)
    return led, counters.after(co, po)


# ---- the rules restated (the tests' expected side) -----------------------------

def pool_id(issuer_vk: bytes) -> bytes:
    """ledger-specs hashKey: Blake2b-224 of the 32-byte cold key."""
    return hashlib.blake2b(bytes(issuer_vk), digest_size=28).digest()


def vrf_key_hash(vrf_vk: bytes) -> bytes:
    """hashVerKeyVRF: Blake2b-256 of the 32-byte VRF key."""
    return hashlib.blake2b(bytes(vrf_vk), digest_size=32).digest()


def is_overlay_slot(first_slot: int, d: Tuple[int, int], slot: int) -> bool:
    """ledger-specs isOverlaySlot: ceil(s d) < ceil((s + 1) d), s = slot - firstSlot."""
    s, dd = slot - first_slot, Fraction(d[0], d[1])
    ceil = lambda x: -((-x.numerator) // x.denominator)  # noqa: E731
    return ceil(s * dd) < ceil((s + 1) * dd)


def classify_overlay_slot(first_slot: int, d: Tuple[int, int], asc_inv: int, ngen: int,
                          slot: int) -> Optional[int]:
    """ledger-specs classifyOverlaySlot on an overlay slot (the caller has
    checked is_overlay_slot): None on a non-active slot, else the index of the
    scheduled genesis key in the sorted key set -- position = ceil(s d), active
    iff position mod ascInv == 0, index (position div ascInv) mod ngen."""
    x = (slot - first_slot) * Fraction(d[0], d[1])
    position = -((-x.numerator) // x.denominator)
    if position % asc_inv != 0:
        return None
    return (position // asc_inv) % ngen


def _oracle_leader():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "oracle",
                        "leader.py")
    spec = importlib.util.spec_from_file_location("ouro_oracle_leader", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_RES = 10**34


def rule(views: LedgerViews, g: Globals, issuer_vk: bytes, vrf_vk: bytes, slot: int,
         leader_output: bytes, c0: int, oracle=None,
         genesis: Optional[GenesisDelegs] = None) -> Tuple[int, int]:
    """(LV_* bits without COUNTER_OK, pool_row) of one header row; with
    ``genesis`` an overlay row takes the delegate branch and its row is a
    genesis row."""
    oracle = oracle or _oracle_leader()
    bits, row = 0, LV_NO_POOL
    kp = slot // g.slots_per_kes_period
    if c0 <= kp < c0 + g.max_kes_evo and c0 <= (1 << 64) - g.max_kes_evo:
        bits |= LV_KES_PERIOD_OK
    j = bisect.bisect_right([e.first_slot for e in views.entries], slot) - 1
    e = views.entries[j]
    if is_overlay_slot(e.first_slot, e.d, slot):
        bits |= LV_OVERLAY
        if genesis is None:
            return bits, row
        gen = genesis.entries[j]
        ix = classify_overlay_slot(e.first_slot, e.d, genesis.asc_inv, len(gen), slot)
        if ix is None:
            return bits, row                      # NotActiveSlotOVERLAY
        bits |= LV_OVERLAY_ACTIVE
        if pool_id(issuer_vk) != gen[ix].delegate_id:
            return bits, row                      # WrongGenesisColdKeyOVERLAY
        bits |= LV_POOL_KNOWN | LV_LEADER_OK      # (no threshold on an overlay slot)
        if vrf_key_hash(vrf_vk) == gen[ix].delegate_vrf:
            bits |= LV_VRF_KEY_OK                 # else WrongGenesisVRFKeyOVERLAY
        return bits, int(genesis.gen_begin[j]) + ix
    ids = [p.pool_id for p in e.pools]
    pid = pool_id(issuer_vk)
    r = bisect.bisect_left(ids, pid)
    if r == len(ids) or ids[r] != pid:
        return bits, row
    p = e.pools[r]
    bits |= LV_POOL_KNOWN
    row = int(views.pool_begin[j]) + r
    if vrf_key_hash(vrf_vk) == p.vrf_hash:
        bits |= LV_VRF_KEY_OK
    if g.f_is_one:
        bits |= LV_LEADER_OK
    elif not (-8 * _RES <= g.un_active_slot_log <= 0):
        bits |= LV_BADARG
    elif oracle.check_leader_value(bytes(leader_output), Fraction(*p.sigma),
                                   g.un_active_slot_log):
        bits |= LV_LEADER_OK
    return bits, row


def fold_rule(views: LedgerViews, ledger: Sequence[int], pool_row: Sequence[int],
              ocert_counter: Sequence[int], known: Dict[bytes, int],
              genesis: Optional[GenesisDelegs] = None):
    """The counter fold with a dict: (ledger with COUNTER_OK, the dict after).
    With ``genesis`` an overlay row's key is its delegate's id."""
    ids = [p.pool_id for e in views.entries for p in e.pools]
    gids = [] if genesis is None else [x.delegate_id for e in genesis.entries for x in e]
    known = dict(known)
    out = []
    for b, r, n_i in zip(ledger, pool_row, ocert_counter):
        b = int(b)
        if (b & LV_POOL_KNOWN) and (genesis is not None or not (b & LV_OVERLAY)):
            key = gids[int(r)] if b & LV_OVERLAY else ids[int(r)]
            m0 = known.get(key, 0)  # currentIssueNo: in the pool distribution / in genDelegs
            b = b | LV_COUNTER_OK if m0 <= int(n_i) else b & ~LV_COUNTER_OK
            known[key] = int(n_i)
        out.append(b)
    return np.array(out, np.uint8), known
