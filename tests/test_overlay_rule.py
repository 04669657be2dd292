"""The genesis-delegate branch of the ledger-view checks on overlay slots
(csrc/ledger_view.h with an ouro_genesis_delegs schedule; include/ouro_verify.h
OURO_LV_OVERLAY_ACTIVE) without a GPU: the host-compiled lane routine and the
library's _host entries against the Python restatement (ledger.rule /
fold_rule with ``genesis``: hashlib, Fraction, a dict) on ~2,100 seeded rows
that reach every outcome, the fold over delegates, every OURO_EINVAL, and the
chain entry's host path on a signed chain that pools and delegates forge
together."""
import ctypes
import os

import numpy as np
import pytest

import ledger_cases as LC
import overlay_cases as OC
from ouroboros_network_amd import _native
from ouroboros_network_amd import header as H
from ouroboros_network_amd import ledger as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")
K, V, Ld, P, C = (L.LV_POOL_KNOWN, L.LV_VRF_KEY_OK, L.LV_LEADER_OK, L.LV_KES_PERIOD_OK,
                  L.LV_COUNTER_OK)
O, A = L.LV_OVERLAY, L.LV_OVERLAY_ACTIVE


@pytest.fixture(scope="module")
def dh():
    lib = ctypes.CDLL(SO)
    lib.dh_ledger_check_overlay.restype = ctypes.c_int
    lib.dh_ledger_check_overlay.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64,
                                            ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.dh_classify_overlay_slot.restype = ctypes.c_int64
    lib.dh_classify_overlay_slot.argtypes = [ctypes.c_uint64] * 4 + [ctypes.c_uint32]
    return lib


def lane(dh, views, g, genesis, row):
    cv, cg, cgen = views.c_struct(), g.c_struct(), genesis.c_struct()
    out = ctypes.c_uint32(7)
    bits = dh.dh_ledger_check_overlay(ctypes.addressof(cv), ctypes.addressof(cg),
                                      ctypes.addressof(cgen), row[0], row[1], row[2], row[3],
                                      row[4], ctypes.addressof(out))
    return bits, out.value


def test_constants():
    assert A == 0x20 and L.LV_ALL_OK == 0x1f and not L.LV_ALL_OK & (A | O | L.LV_BADARG)


def test_classify_overlay_slot_formula(dh):
    """position = ceil(s d) from is_overlay_slot's own division, active iff
    position mod asc_inv == 0, index (position div asc_inv) mod ngen: d = 1,
    1/2, 3/10, 1 / (2^63 - 25), a 63-bit fraction and 0, asc_inv = 1, 20, 3 and
    a large one, ngen = 1, 5, 7, s up to 2^64 - 1"""
    rng = np.random.default_rng(17)
    ds = [(1, 1), (1, 2), (3, 10), (1, OC.DEN63), LC.D63, (0, 1), (2**64 - 2, 2**64 - 1)]
    ss = list(range(60)) + [OC.DEN63 - 1, OC.DEN63, OC.DEN63 + 1, 2 * OC.DEN63, 2**63, 2**63 - 1,
                            2**64 - 1, 2**64 - 2, 2**32, 2**32 - 1] + \
        [int(x) for x in rng.integers(0, 2**63, 60)]
    seen = set()
    for d in ds:
        for asc_inv in (1, 20, 3, 2**40 + 1):
            for ngen in (1, 5, 7):
                for s in ss:
                    got = dh.dh_classify_overlay_slot(s, d[0], d[1], asc_inv, ngen)
                    if not L.is_overlay_slot(0, d, s):
                        want = -1
                    else:
                        ix = L.classify_overlay_slot(0, d, asc_inv, ngen, s)
                        want = -2 if ix is None else ix
                    assert got == want, (d, asc_inv, ngen, s)
                    seen.add(min(want, 0) if want < 0 else 1)
    assert seen == {-1, -2, 1}
    # d = 1/2, asc_inv = 20, 7 keys: slot 40 t is active and key t mod 7 is scheduled
    assert [dh.dh_classify_overlay_slot(40 * t, 1, 2, 20, 7) for t in range(9)] == \
        [0, 1, 2, 3, 4, 5, 6, 0, 1]
    assert dh.dh_classify_overlay_slot(2, 1, 2, 20, 7) == -2
    assert dh.dh_classify_overlay_slot(1, 1, 2, 20, 7) == -1


def test_the_set_reaches_every_outcome():
    """a condition on the generator: at least 50 rows of each outcome"""
    count = {o: 0 for o in OC.OUTCOMES}
    n = 0
    for _, rows, bits, _ in OC.all_rows():
        n += len(rows)
        for b in bits:
            for o in OC.outcome(b):
                count[o] += 1
    assert 1900 <= n <= 2300
    assert all(c >= 50 for c in count.values()), count
    # d, ngen and the large s are all in the set
    v = OC.views()[0]
    assert {e.d for e in v.entries} == {(1, 1), (1, 2), (3, 10), (0, 1), (1, OC.DEN63)}
    assert {len(e) for e in OC.views()[3][1].entries} == {0, 1, 5, 7}
    slots = {r[2] for _, rows, _, _ in OC.all_rows() for r in rows}
    assert 4000 + OC.DEN63 in slots and 2**64 - 1 in slots and OC.FAR in slots and 0 in slots
    assert {e.first_slot for e in v.entries} <= slots
    assert {e.first_slot - 1 for e in v.entries[1:]} <= slots


def test_lane_routine_equals_the_rule_on_every_row(dh):
    v, _, _, gens = OC.views()
    seen = set()
    for a, rows, bits, prow in OC.all_rows():
        for r, b, p in zip(rows, bits, prow):
            assert lane(dh, v, LC.G_MAIN, gens[a], r) == (int(b), int(p)), (a, r[2:])
            seen.add(int(b))
    for want in (O | P, O, O | A | P, O | A, O | A | K | Ld | P, O | A | K | Ld | V | P,
                 O | A | K | Ld | V):
        assert want in seen, hex(want)
    # never on an overlay row: BADARG, LEADER_OK without POOL_KNOWN, ACTIVE without OVERLAY
    for b in seen:
        if b & O:
            assert not b & L.LV_BADARG and bool(b & Ld) == bool(b & K)
        else:
            assert not b & A


def test_host_entry_equals_the_rule():
    """ouro_tpraos_ledger_checks_overlay_host on every row, and under the other
    globals: overlay rows never see the leader check's BADARG"""
    v, _, _, gens = OC.views()
    for a, rows, bits, prow in OC.all_rows():
        cols = LC.columns(rows)
        got = L.ledger_checks(*cols[:5], v, LC.G_MAIN, genesis=gens[a], host=True)
        np.testing.assert_array_equal(got[0], bits)
        np.testing.assert_array_equal(got[1], prow)
    a, rows, _, _ = OC.all_rows()[1]
    sub = rows[::5]
    for g in [LC.G_ONE] + LC.G_BAD:
        want = OC.expect(v, g, sub, gens[a])
        got = L.ledger_checks(*LC.columns(sub)[:5], v, g, genesis=gens[a], host=True)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        ov = (want[0] & O) != 0
        assert ov.any() and not (want[0][ov] & L.LV_BADARG).any()


def test_a_valid_header_has_all_ok_on_either_kind_of_slot():
    v, pkeys, dkeys, gens = OC.views()
    gen = gens[1]
    table = OC.table_for(v, gen)
    d, p = dkeys[0][3], pkeys[3][0]            # entry 0, d = 1: slot 3 schedules key 3 of 5
    rows = [LC._row(d.cold, d.vrf, 3, b"\xff" * 64, 0, 0),
            LC._row(p.cold, p.vrf, 3005, bytes(64), 30, 0)]
    cols = LC.columns(rows)
    got = L.ledger_checks(*cols[:5], v, LC.G_ONE, genesis=gen, ocert_counter=cols[5],
                          counters=table, host=True)
    assert got[0][0] == L.LV_ALL_OK | O | A and got[0][1] == L.LV_ALL_OK
    assert got[1][0] == 3 and got[1][1] == int(v.pool_begin[3]) + \
        [q.pool_id for q in v.entries[3].pools].index(p.id)
    # anyone else on that overlay slot: never ALL_OK
    for k in [dkeys[0][2], pkeys[0][0], p]:
        cols = LC.columns([LC._row(k.cold, k.vrf, 3, bytes(64), 0, 0)])
        b = L.ledger_checks(*cols[:5], v, LC.G_ONE, genesis=gen, ocert_counter=cols[5],
                            counters=table, host=True)[0][0]
        assert b & L.LV_ALL_OK != L.LV_ALL_OK and b == O | A | P


def test_pool_on_overlay_slot_and_delegate_on_pool_slot(dh):
    v, pkeys, dkeys, gens = OC.views()
    gen = gens[1]
    e = v.entries[1]                           # d = 1/2: even s overlay, odd s not
    both = pkeys[1][0]                         # delegate 0, also a pool of entry 1
    other = next(k for k in dkeys[1] if k.id != both.id)
    pool = pkeys[1][1]
    ix = [k.id for k in dkeys[1]].index(both.id)
    s_pool = 1001
    s_both = next(s for s in range(1000, 1100, 2)
                  if OC.classify(e, 1, 7, s) == ix)
    s_other = next(s for s in range(1000, 1100, 2) if OC.classify(e, 1, 7, s) != ix)
    for key, slot, want in [
            (pool, s_both, O | A | P),                              # a pool on an overlay slot
            (other, s_pool, P),                                     # a delegate that is no pool
            (both, s_pool, K | V | P),                              # a delegate that is one (+ leader)
            (both, s_both, O | A | K | V | Ld | P),                 # scheduled
            (both, s_other, O | A | P)]:                            # not its slot
        row = (key.cold, key.vrf, slot, b"\xff" * 64, slot // LC.SPKP)
        got = lane(dh, v, LC.G_MAIN, gen, row)
        assert got == L.rule(v, LC.G_MAIN, *row, oracle=LC.OL, genesis=gen)
        assert got[0] & ~Ld == want & ~Ld if not got[0] & O else got[0] == want, (slot, hex(got[0]))
    # on the pool slot the row is the POOL's row, on its overlay slot the genesis row
    r1 = lane(dh, v, LC.G_MAIN, gen, (both.cold, both.vrf, s_pool, bytes(64), 10))[1]
    r2 = lane(dh, v, LC.G_MAIN, gen, (both.cold, both.vrf, s_both, bytes(64), 10))[1]
    assert v.pool_begin[1] <= r1 < v.pool_begin[2] and r2 == int(gen.gen_begin[1]) + ix


# ---- the fold ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """one entry, d = 1/2, asc_inv = 1, two delegates (rows 0, 1 by genesis id)
    and two pools"""
    rng = np.random.default_rng(33)
    pa, pb, da, db = (LC.Key(rng) for _ in range(4))
    views = L.LedgerViews([L.Entry(0, (1, 2), (pa.pool((1, 1)), pb.pool((1, 1))))])
    gen = L.GenesisDelegs([(L.GenDeleg(b"\x01" * 28, da.id, da.vrf_hash),
                            L.GenDeleg(b"\x02" * 28, db.id, db.vrf_hash))], 1)
    pools = sorted([pa, pb], key=lambda k: k.id)
    return views, gen, pools, (da, db)


def run_fold(views, gen, table, ledger, rows, ctr):
    got, after = L.counter_fold(ledger, rows, ctr, views, table, genesis=gen)
    want, known = L.fold_rule(views, ledger, rows, ctr, table.as_dict(), genesis=gen)
    np.testing.assert_array_equal(got, want)
    assert after.as_dict() == known
    return got, after


def test_delegate_counter_absent_equal_rising_falling(small):
    views, gen, pools, (da, db) = small
    table = OC.table_for(views, gen, {db.id: 5})
    D = O | A | K
    # delegate a (row 0): absent (0 <= 0), equal, rising, falling; b (row 1): 5 then 4 falls
    rows = [0, 0, 0, 0, 1, 1]
    ctr = [0, 0, 7, 6, 5, 4]
    got, after = run_fold(views, gen, table, [D] * 6, rows, ctr)
    assert [bool(x & C) for x in got] == [True, True, True, False, True, False]
    assert after.as_dict() == {da.id: 6, db.id: 4}
    # the plain fold still skips every overlay row
    got2, after2 = L.counter_fold([D] * 6, rows, ctr, views, table)
    assert list(got2) == [D] * 6 and after2.as_dict() == {db.id: 5}
    # and so does this one when the row is not POOL_KNOWN
    got3, after3 = run_fold(views, gen, table, [O | A, O, O | P], [L.LV_NO_POOL] * 3, [1, 1, 1])
    assert list(got3) == [O | A, O, O | P] and after3.as_dict() == {db.id: 5}


def test_pool_and_delegate_rows_interleaved_and_aliased_outputs(small):
    views, gen, pools, (da, db) = small
    table = OC.table_for(views, gen, {pools[0].id: 2})
    D = O | A | K
    # view row 0 and genesis row 0 are different keys with counters of their own
    ledger = np.array([K, D, K, D, K, D, K | C], np.uint8)
    rows = np.array([0, 0, 0, 0, 1, 1, 0], np.uint32)
    ctr = np.array([2, 9, 3, 8, 0, 1, 2], np.uint64)
    got, after = run_fold(views, gen, table, ledger, rows, ctr)
    assert [bool(x & C) for x in got] == [True, True, True, False, True, True, False]
    assert after.as_dict() == {pools[0].id: 2, pools[1].id: 0, da.id: 8, db.id: 1}
    # counter_out / present_out aliasing the table's own arrays
    t = OC.table_for(views, gen, {pools[0].id: 2})
    cv, cg, cc = views.c_struct(), gen.c_struct(), t.c_struct()
    led = ledger.copy()
    rc = _native.load().ouro_ocert_counter_fold_overlay(
        len(led), rows.ctypes.data, ctr.ctypes.data, ctypes.byref(cv), ctypes.byref(cg),
        ctypes.byref(cc), t.counter.ctypes.data, t.present.ctypes.data, led.ctypes.data)
    assert rc == _native.OURO_OK
    np.testing.assert_array_equal(led, got)
    assert t.as_dict() == after.as_dict()


def test_a_key_that_is_pool_and_delegate_shares_one_counter():
    v, pkeys, dkeys, gens = OC.views()
    gen = gens[1]
    both = pkeys[1][0]
    ix = [k.id for k in dkeys[1]].index(both.id)
    prow = [p.pool_id for p in v.entries[1].pools].index(both.id) + int(v.pool_begin[1])
    grow = int(gen.gen_begin[1]) + ix
    table = OC.table_for(v, gen)
    got, after = run_fold(v, gen, table, [K, O | A | K, K], [prow, grow, prow], [4, 3, 3])
    assert [bool(x & C) for x in got] == [True, False, True] and after.as_dict() == {both.id: 3}


def test_host_entry_runs_the_fold_over_both(small):
    views, gen, pools, (da, db) = small
    pa = pools[0]
    rows = [LC._row(da.cold, da.vrf, 0, bytes(64), 0, 4),      # s = 0: key 0 scheduled
            LC._row(pa.cold, pa.vrf, 1, bytes(64), 0, 1),
            LC._row(db.cold, db.vrf, 2, bytes(64), 0, 0),      # s = 2: position 1, key 1
            LC._row(da.cold, da.vrf, 4, bytes(64), 0, 3),      # falls
            LC._row(db.cold, db.vrf, 4, bytes(64), 0, 9)]      # not its slot: not folded
    cols = LC.columns(rows)
    table = OC.table_for(views, gen, {da.id: 4})
    bits, prow = OC.expect(views, LC.G_ONE, rows, gen)
    want, known = L.fold_rule(views, bits, prow, cols[5], table.as_dict(), genesis=gen)
    got = L.ledger_checks(*cols[:5], views, LC.G_ONE, genesis=gen, ocert_counter=cols[5],
                          counters=table, host=True)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], prow)
    assert got[2].as_dict() == known == {da.id: 3, pa.id: 1, db.id: 0}
    assert [bool(x & C) for x in want] == [True, True, True, False, False]
    assert list(prow) == [0, int(prow[1]), 1, 0, L.LV_NO_POOL]


# ---- the argument checks ----------------------------------------------------------------
def _einval(views, gen, counters=None):
    z32, z64 = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)
    with pytest.raises(ValueError):
        L.ledger_checks(z32, z32, [0], z64, [0], views, LC.G_MAIN, genesis=gen, counters=counters,
                        ocert_counter=[0] if counters is not None else None, host=True)
    if counters is not None:
        with pytest.raises(ValueError):
            L.counter_fold([0], [0], [0], views, counters, genesis=gen)


def test_every_einval(small):
    views, gen, pools, (da, db) = small
    g = [L.GenDeleg(b"\x01" * 28, da.id, da.vrf_hash), L.GenDeleg(b"\x02" * 28, db.id, db.vrf_hash)]
    G = L.GenesisDelegs
    z32, z64 = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)
    ok = lambda gen, v=views, **kw: L.ledger_checks(  # noqa: E731
        z32, z32, [0], z64, [0], v, LC.G_MAIN, genesis=gen, host=True, **kw)
    ok(gen)
    _einval(views, G([g, g], 1))                                   # k != views->k
    _einval(views, G([], 1))
    _einval(views, G([g], 0))                                      # asc_inv == 0
    _einval(views, G([g[::-1]], 1, sort=False))                    # genesis ids out of order
    _einval(views, G([[g[0], g[0]]], 1, sort=False))               # not strictly ascending
    _einval(views, G([[]], 1))                                     # d > 0 and no rows
    two = L.LedgerViews([L.Entry(0, (0, 1), ()), L.Entry(9, (1, 2), ())])
    ok(G([[], g], 1), two)                                         # d = 0 and no rows is fine
    _einval(two, G([g, []], 1))
    # sorted within an entry only: the second entry out of order is refused
    two_d = L.LedgerViews([L.Entry(0, (1, 2), ()), L.Entry(9, (1, 2), ())])
    ok(G([g, g], 1), two_d)
    _einval(two_d, G([g, g[::-1]], 1, sort=False))
    bad = G([g], 1)
    bad.gen_begin[0] = 1
    _einval(views, bad)                                            # gen_begin[0] != 0
    bad = G([g, g], 1)
    bad.gen_begin[1], bad.gen_begin[2] = 2, 1
    _einval(two_d, bad)                                            # decreasing
    bad = G([g], 1)
    bad.gen_begin[1] = _native.LV_GEN_ROWS_MAX + 1
    _einval(views, bad)                                            # more rows than the cap
    # the counters table must have a row for every delegate id (and every pool id)
    ids = [p.id for p in pools]
    ok(gen, counters=L.Counters(ids + [da.id, db.id]), ocert_counter=[0])
    _einval(views, gen, counters=L.Counters(ids + [da.id]))
    _einval(views, gen, counters=L.Counters(ids + [db.id]))
    _einval(views, gen, counters=L.Counters([da.id, db.id]))
    # null arrays
    lib = _native.load()
    cv, cg = views.c_struct(), LC.G_MAIN.c_struct()
    p = np.zeros(64, np.uint8).ctypes.data
    for field in ("gen_begin", "genesis_id", "delegate_id", "delegate_vrf"):
        cgen = gen.c_struct()
        args = [1, p, p, p, p, p, None, ctypes.byref(cv), ctypes.byref(cgen), ctypes.byref(cg), None,
                None, None, p, None]
        assert lib.ouro_tpraos_ledger_checks_overlay_host(*args) == _native.OURO_OK
        setattr(cgen, field, None)
        assert lib.ouro_tpraos_ledger_checks_overlay_host(*args) == _native.OURO_EINVAL, field
    # the chain entry refuses the same before anything runs
    s = OC.chain_stream()
    import envelope_cases as EC
    with pytest.raises(ValueError):
        H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                     genesis=G([g], 1), cfg=EC.VAL_CFG, epochs=s["epochs"],
                                     host=True)
    with pytest.raises(ValueError):
        H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                     genesis=s["genesis"],
                                     counters=L.Counters(s["table_ids"][:4]), cfg=EC.VAL_CFG,
                                     epochs=s["epochs"], host=True)


def test_null_schedule_is_byte_identical_to_the_existing_entries():
    """the _overlay entries with genesis = NULL on ledger_cases.main_rows, with
    the fold: every output equals the existing entry's"""
    views, _ = LC.main_views()
    rows = LC.main_rows()
    cols = LC.columns(rows)
    table = L.Counters(views.all_pool_ids(), {views.all_pool_ids()[0]: 1})
    ctr = (np.arange(len(rows)) % 3).astype(np.uint64)
    old = L.ledger_checks(*cols[:5], views, LC.G_MAIN, ocert_counter=ctr, counters=table, host=True)
    lib = _native.load()
    cv, cg, cc = views.c_struct(), LC.G_MAIN.c_struct(), table.c_struct()
    n = len(rows)
    led, prow = np.full(n, 0xAA, np.uint8), np.full(n, 5, np.uint32)
    co, po = np.zeros_like(table.counter), np.zeros_like(table.present)
    rc = lib.ouro_tpraos_ledger_checks_overlay_host(
        n, *(c.ctypes.data for c in cols[:5]), ctr.ctypes.data, ctypes.byref(cv), None,
        ctypes.byref(cg), ctypes.byref(cc), co.ctypes.data, po.ctypes.data, led.ctypes.data,
        prow.ctypes.data)
    assert rc == _native.OURO_OK
    assert led.tobytes() == old[0].tobytes() and prow.tobytes() == old[1].tobytes()
    assert co.tobytes() == old[2].counter.tobytes() and po.tobytes() == old[2].present.tobytes()
    bits, want_rows = LC.main_expect()
    np.testing.assert_array_equal(led & ~np.uint8(C), bits)
    # the fold entry likewise
    f_old = L.counter_fold(bits, want_rows, ctr, views, table)
    led2 = bits.copy()
    rc = lib.ouro_ocert_counter_fold_overlay(n, want_rows.ctypes.data, ctr.ctypes.data,
                                             ctypes.byref(cv), None, ctypes.byref(cc),
                                             co.ctypes.data, po.ctypes.data, led2.ctypes.data)
    assert rc == _native.OURO_OK and led2.tobytes() == f_old[0].tobytes()
    assert co.tobytes() == f_old[1].counter.tobytes()


# ---- the chain entry's host path -----------------------------------------------------------
def test_chain_entry_on_the_host_path():
    """ouro_chain_validate_ledger_overlay_cbor_host on the chain that four pools
    and two delegates forge under d = 1/2: bits, rows and counters from the
    Python rule; crypto, envelope and the non-overlay rows byte-identical to
    ouro_chain_validate_ledger_cbor_host"""
    import envelope_cases as EC

    s = OC.chain_stream()
    table = L.Counters(s["table_ids"], s["known"])
    kw = dict(counters=table, cfg=EC.VAL_CFG, epochs=s["epochs"], nonce=True, host=True)
    got = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       genesis=s["genesis"], **kw)
    ref = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN, **kw)
    for x, y in zip(ref[0], got[0]):
        assert x.tobytes() == y.tobytes()
    assert ref[1].tobytes() == got[1].tobytes() and ref[2].tobytes() == got[2].tobytes()
    assert ref[3] == got[3] and ref[4] == got[4]
    nb = s["n_byron"]
    assert (got[0][2][nb:] & 0x0F == 0x0F).all()        # every TPraos header verifies
    ledger, prow, known = OC.chain_expect(s)
    np.testing.assert_array_equal(got[5], ledger)
    np.testing.assert_array_equal(got[6], prow)
    assert got[7].as_dict() == known
    # without the schedule: the reference call is what it always was, and equal off the overlay
    ledger0, prow0, known0 = OC.chain_expect(s, genesis=False)
    np.testing.assert_array_equal(ref[5], ledger0)
    assert ref[7].as_dict() == known0
    plain = (ledger & O) == 0
    np.testing.assert_array_equal(got[5][plain], ref[5][plain])
    np.testing.assert_array_equal(got[6][plain], ref[6][plain])
    tp = ledger[nb:]
    # the cases the chain was built for
    assert tp[3] == O | P                                # an inactive overlay slot
    assert tp[9] == O | A | P and tp[12] == O | A | P    # the wrong delegate; a pool
    assert tp[5] == L.LV_ALL_OK | O | A                  # stream header 255
    assert tp[6] == (L.LV_ALL_OK | O | A) & ~C           # 256: the counter fell across the chunk
    assert tp[20] == (L.LV_ALL_OK | O | A) & ~C          # delegate 1's counter falls
    assert (tp == L.LV_ALL_OK).sum() >= 15 and (tp == L.LV_ALL_OK | O | A).sum() >= 12
    assert {int(r) for r in prow[nb:][(tp & (O | K)) == (O | K)]} == {0, 1, 2, 3, 4, 5}
