"""The ledger-view header checks (csrc/ledger_view.h; include/ouro_verify.h
OURO_LV_*) without a GPU: the two hashes pinned on the reference's fixtures,
the host-compiled lane routine and the library's host entry against the
Python restatement (ledger.rule: hashlib, bisect, oracle/leader.py) branch by
branch, and every OURO_EINVAL."""
import ctypes
import hashlib
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import ledger_cases as LC
from ouroboros_network_amd import _native
from ouroboros_network_amd import header as H
from ouroboros_network_amd import ledger as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")


@pytest.fixture(scope="module")
def dh():
    lib = ctypes.CDLL(SO)
    lib.dh_ledger_check.restype = ctypes.c_int
    lib.dh_ledger_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                                    ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p,
                                    ctypes.c_uint64, ctypes.c_void_p]
    lib.dh_is_overlay_slot.restype = ctypes.c_int
    lib.dh_is_overlay_slot.argtypes = [ctypes.c_uint64] * 3
    lib.dh_blake2b224_32.restype = None
    lib.dh_blake2b224_32.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(ROOT, "tests", "golden", "reference_ledger_view.json")) as f:
        return json.load(f)


def lane(dh, views, g, row):
    cv, cg = views.c_struct(), g.c_struct()
    out = ctypes.c_uint32(7)
    bits = dh.dh_ledger_check(ctypes.addressof(cv), ctypes.addressof(cg), row[0], row[1], row[2],
                              row[3], row[4], ctypes.addressof(out))
    return bits, out.value


def test_reference_fixtures_pin_the_two_hashes(fx, kats, dh):
    """hashVerKeyVRF = Blake2b-256 and hashKey = Blake2b-224: the golden
    headers' keys against Result_StakeDistribution's VRF hash and the pool id
    in the golden GenTx; the device routine for the 28-byte digest too"""
    sd = fx["stake_distribution"]
    assert len(bytes.fromhex(sd["pool_id"])) == 28 and sd["stake"] == [1, 1]
    assert sd["vrf_hash"].startswith("c5e21ab1") and sd["vrf_hash"].endswith("7b4c")
    assert fx["gen_tx_pool_id"].startswith("0d6a577e") and fx["gen_tx_pool_id"].endswith("fb06")
    assert sd["pool_id"] in fx["chain_dep_state_counters"]
    for h in kats["headers"]:
        p = H.parse_header(bytes.fromhex(h["raw"]))
        assert L.vrf_key_hash(p.vrf_vk).hex() == sd["vrf_hash"]
        assert L.pool_id(p.issuer_vk).hex() == fx["gen_tx_pool_id"]
        out = ctypes.create_string_buffer(28)
        dh.dh_blake2b224_32(p.issuer_vk, out)
        assert out.raw.hex() == fx["gen_tx_pool_id"]


def test_blake2b224_lane_routine(dh):
    rng = np.random.default_rng(3)
    for m in [bytes(32), b"\xff" * 32] + [rng.bytes(32) for _ in range(200)]:
        out = ctypes.create_string_buffer(28)
        dh.dh_blake2b224_32(m, out)
        assert out.raw == hashlib.blake2b(m, digest_size=28).digest()


def test_golden_view_accepts_the_golden_header(fx, kats, dh):
    """the fixture's distribution keyed by the golden header's pool id: known,
    right VRF key, and with a stake of 1 it leads whenever f = 1"""
    sd = fx["stake_distribution"]
    p = H.parse_header(bytes.fromhex(kats["headers"][0]["raw"]))
    views = L.LedgerViews([L.Entry(0, (0, 1), (L.Pool(bytes.fromhex(fx["gen_tx_pool_id"]),
                                                      bytes.fromhex(sd["vrf_hash"]),
                                                      tuple(sd["stake"])),))])
    row = (p.issuer_vk, p.vrf_vk, p.slot, p.leader_output, p.ocert_kes_period)
    want = L.rule(views, LC.G_ONE, *row, oracle=LC.OL)
    assert lane(dh, views, LC.G_ONE, row) == want
    assert want[0] & (L.LV_POOL_KNOWN | L.LV_VRF_KEY_OK | L.LV_LEADER_OK) == 0x07 and want[1] == 0


def test_overlay_slot_formula(dh):
    """ceil(s d) < ceil((s + 1) d) in exact integers: d = 0, 1, 1/2, 3/10 and a
    63-bit fraction over 40 consecutive slots and at large s"""
    rng = np.random.default_rng(5)
    ds = [(0, 1), (1, 1), (1, 2), (3, 10), LC.D63, (2**63 - 26, 2**63 - 25), (1, 2**63 - 25),
          (2**64 - 2, 2**64 - 1), (7, 7)]
    for d in ds:
        ss = list(range(40)) + [2**64 - 1, 2**64 - 2, 2**63, 2**32 - 1, 2**32] + \
            [int(x) for x in rng.integers(0, 2**63, 40)]
        got = [dh.dh_is_overlay_slot(s, d[0], d[1]) for s in ss]
        want = [int(L.is_overlay_slot(0, d, s)) for s in ss]
        assert got == want, d
    assert [dh.dh_is_overlay_slot(s, 3, 10) for s in range(10)] == [1, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert sum(dh.dh_is_overlay_slot(s, 1, 2) for s in range(40)) == 20


def test_lane_routine_equals_the_rule_branch_by_branch(dh):
    views, _ = LC.main_views()
    rows = LC.main_rows()
    bits, prow = LC.main_expect()
    seen = set()
    for r, b, p in zip(rows, bits, prow):
        assert lane(dh, views, LC.G_MAIN, r) == (int(b), int(p)), r[2:]
        seen.add(int(b))
    # every branch was reached: unknown, overlay, known with each of the other bits both ways
    K, V, Ld, P, O = (L.LV_POOL_KNOWN, L.LV_VRF_KEY_OK, L.LV_LEADER_OK, L.LV_KES_PERIOD_OK,
                      L.LV_OVERLAY)
    for want in (P, O, O | P, K | P, K | V | P, K | Ld | P, K | V | Ld | P, K | V | Ld,
                 K | V):
        assert want in seen, hex(want)
    assert 1800 <= len(rows) <= 2600


def test_first_and_last_row_and_one_byte_neighbours(dh):
    views, keys = LC.main_views()
    rng = np.random.default_rng(11)
    for j in (4, 6):
        e = views.entries[j]
        by_id = {k.id: k for k in keys[j]}
        for r in (0, len(e.pools) - 1):
            k = by_id.get(e.pools[r].pool_id)
            if k is None:
                continue
            got = lane(dh, views, LC.G_MAIN, (k.cold, k.vrf, e.first_slot + 3, LC._beta(rng), 0))
            assert got[1] == int(views.pool_begin[j]) + r and got[0] & L.LV_POOL_KNOWN
    # entry 6: the real pools sit between ids that differ in byte 0 or byte 27 only,
    # and 0x7f.. sorts below 0x80.. (unsigned bytes)
    e = views.entries[6]
    ids = [p.pool_id for p in e.pools]
    a, s7f = keys[6]
    ia, i7 = ids.index(a.id), ids.index(s7f.id)
    assert ids[ia - 1][:27] == a.id[:27] and ids[ia + 1][:27] == a.id[:27]
    assert ids[i7 + 1] == b"\x80" + s7f.id[1:] or b"\x80" + s7f.id[1:] in ids[i7 + 1:]
    for k, i in ((a, ia), (s7f, i7)):
        got = lane(dh, views, LC.G_MAIN, (k.cold, k.vrf, 6500, bytes(64), 65))
        assert got == (L.LV_ALL_OK & ~L.LV_COUNTER_OK, int(views.pool_begin[6]) + i)


def test_same_pool_in_two_entries(dh):
    views, keys = LC.main_views()
    dup = keys[2][0]
    beta = bytes(64)
    b2, r2 = lane(dh, views, LC.G_MAIN, (dup.cold, dup.vrf, 2001, beta, 20))
    b4, r4 = lane(dh, views, LC.G_MAIN, (dup.cold, dup.vrf, 4001, beta, 40))
    assert (b2, r2) == L.rule(views, LC.G_MAIN, dup.cold, dup.vrf, 2001, beta, 20, oracle=LC.OL)
    assert (b4, r4) == L.rule(views, LC.G_MAIN, dup.cold, dup.vrf, 4001, beta, 40, oracle=LC.OL)
    assert b2 & L.LV_VRF_KEY_OK and not b4 & L.LV_VRF_KEY_OK and r2 != r4
    assert views.pool_begin[2] <= r2 < views.pool_begin[3] <= views.pool_begin[4] <= r4


@pytest.mark.parametrize("k", [1, 3, 4096])
def test_slot_at_and_below_each_boundary(dh, k):
    views, ks = LC.views_k(k)
    rng = np.random.default_rng(k)
    for j in sorted({0, 1, 2, k // 2, k - 2, k - 1} & set(range(k))):
        for slot in (10 * j, 10 * j - 1, 10 * j + 9):
            if slot < 0:
                continue
            for key in ks:
                row = (key.cold, key.vrf, slot, LC._beta(rng), slot // LC.SPKP)
                want = L.rule(views, LC.G_MAIN, *row, oracle=LC.OL)
                assert lane(dh, views, LC.G_MAIN, row) == want
                assert 2 * min(slot // 10, k - 1) <= want[1] < 2 * min(slot // 10, k - 1) + 2


def test_period_edges(dh):
    views, ks = LC.views_k(1)
    k = ks[0]
    for slot in (6400, 6499, 2**64 - 1):
        kp = slot // LC.SPKP
        for c0, ok in ((kp + 1, False), (kp, True), (kp - LC.MAX_EVO + 1, True),
                       (kp - LC.MAX_EVO, False)):
            bits, _ = lane(dh, views, LC.G_MAIN, (k.cold, k.vrf, slot, bytes(64), c0))
            assert bool(bits & L.LV_KES_PERIOD_OK) == ok, (slot, c0)
    # the sum does not wrap: a c0 above 2^64 - max_kes_evo fails whatever the slot
    for c0 in (2**64 - LC.MAX_EVO + 1, 2**64 - 1):
        bits, _ = lane(dh, views, LC.G_MAIN, (k.cold, k.vrf, 2**64 - 1, bytes(64), c0))
        assert not bits & L.LV_KES_PERIOD_OK
    g0 = L.Globals(LC.SPKP, 0, LC.G_MAIN.un_active_slot_log)
    assert not lane(dh, views, g0, (k.cold, k.vrf, 0, bytes(64), 0))[0] & L.LV_KES_PERIOD_OK


def test_badarg_and_f_is_one(dh):
    views, ks = LC.views_k(1)
    k = ks[0]
    row = (k.cold, k.vrf, 5, b"\xff" * 64, 0)
    for g in LC.G_BAD:
        want = L.rule(views, g, *row, oracle=LC.OL)
        assert lane(dh, views, g, row) == want
        assert want[0] & L.LV_BADARG and not want[0] & L.LV_LEADER_OK
    for g in (LC.G_ONE, LC.G_EDGE, LC.G_MAIN):
        want = L.rule(views, g, *row, oracle=LC.OL)
        assert lane(dh, views, g, row) == want and not want[0] & L.LV_BADARG
    assert lane(dh, views, LC.G_ONE, row)[0] & L.LV_LEADER_OK
    # an unknown pool never reaches the leader check: no BADARG either
    assert lane(dh, views, LC.G_BAD[0], (bytes(32), k.vrf, 5, bytes(64), 0))[0] == \
        L.LV_KES_PERIOD_OK


def test_host_entry_equals_the_rule():
    """ouro_tpraos_ledger_checks_host on the ~2,000 rows, with and without
    pool_row's companion outputs, and under the other globals"""
    views, _ = LC.main_views()
    rows = LC.main_rows()
    cols = LC.columns(rows)
    bits, prow = LC.main_expect()
    got = L.ledger_checks(*cols[:5], views, LC.G_MAIN, host=True)
    np.testing.assert_array_equal(got[0], bits)
    np.testing.assert_array_equal(got[1], prow)
    sub = rows[::9]
    for g in [LC.G_ONE, LC.G_EDGE] + LC.G_BAD:
        want = LC.expect(views, g, sub)
        got = L.ledger_checks(*LC.columns(sub)[:5], views, g, host=True)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    # n = 0 is fine
    e = L.ledger_checks(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), [],
                        np.zeros((0, 64), np.uint8), [], views, LC.G_MAIN, host=True)
    assert e[0].size == 0


def _einval(views, g=LC.G_MAIN, counters=None, **kw):
    z32, z64 = np.zeros((1, 32), np.uint8), np.zeros((1, 64), np.uint8)
    with pytest.raises(ValueError):
        L.ledger_checks(z32, z32, [0], z64, [0], views, g, counters=counters,
                        ocert_counter=[0] if counters is not None else None, host=True, **kw)


def test_every_einval():
    rng = np.random.default_rng(1)
    a, b = sorted([LC.Key(rng), LC.Key(rng)], key=lambda k: k.id)
    P = lambda k, s=(1, 2): k.pool(s)  # noqa: E731
    E = L.Entry
    ok = L.LedgerViews([E(0, (0, 1), (P(a), P(b)))])
    L.ledger_checks(np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), [0],
                    np.zeros((1, 64), np.uint8), [0], ok, LC.G_MAIN, host=True)
    _einval(L.LedgerViews([]))                                             # k = 0
    _einval(L.LedgerViews([E(j, (0, 1), ()) for j in range(_native.EPOCHS_MAX + 1)]))
    _einval(L.LedgerViews([E(1, (0, 1), ())]))                             # first_slot[0] != 0
    _einval(L.LedgerViews([E(0, (0, 1), ()), E(5, (0, 1), ()), E(5, (0, 1), ())]))
    _einval(L.LedgerViews([E(0, (0, 1), ()), E(5, (0, 1), ()), E(4, (0, 1), ())]))
    _einval(L.LedgerViews([E(0, (0, 0), ())]))                             # d_den == 0
    _einval(L.LedgerViews([E(0, (2, 1), ())]))                             # d_num > d_den
    _einval(L.LedgerViews([E(0, (0, 1), (P(a, (1, 0)),))]))                # sigma_den == 0
    _einval(L.LedgerViews([E(0, (0, 1), (P(a, (3, 2)),))]))                # sigma_num > sigma_den
    _einval(L.LedgerViews([E(0, (0, 1), (P(b), P(a)))], sort=False))       # out of order
    _einval(L.LedgerViews([E(0, (0, 1), (P(a), P(a)))], sort=False))       # not strictly
    # sorted within an entry only: the same order in two entries is fine, the
    # second entry out of order is not
    _einval(L.LedgerViews([E(0, (0, 1), (P(a), P(b))), E(9, (0, 1), (P(b), P(a)))], sort=False))
    v = L.LedgerViews([E(0, (0, 1), (P(a), P(b)))])
    v.pool_begin[0] = 1
    _einval(v)                                                             # pool_begin[0] != 0
    v = L.LedgerViews([E(0, (0, 1), (P(a), P(b))), E(7, (0, 1), ())])
    v.pool_begin[1], v.pool_begin[2] = 2, 1
    _einval(v)                                                             # decreasing
    v = L.LedgerViews([E(0, (0, 1), ())])
    v.pool_begin[1] = _native.LV_ROWS_MAX + 1
    _einval(v)                                                             # too many rows
    _einval(ok, g=L.Globals(0, 64, 0))                                     # spkp == 0
    # the counters table: out of order, or lacking a view pool
    _einval(ok, counters=L.Counters([b.id, a.id], sort=False))
    _einval(ok, counters=L.Counters([a.id]))
    _einval(ok, counters=L.Counters([]))
    # null arrays
    lib = _native.load()
    cv, cg = ok.c_struct(), LC.G_MAIN.c_struct()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    args = [1, p, p, p, p, p, None, ctypes.byref(cv), ctypes.byref(cg), None, None, None, p, None]
    assert lib.ouro_tpraos_ledger_checks_host(*args) == _native.OURO_OK
    for i in (1, 2, 3, 4, 5, 7, 8, 12):
        bad = list(args)
        bad[i] = None
        assert lib.ouro_tpraos_ledger_checks_host(*bad) == _native.OURO_EINVAL, i
    cv2 = ok.c_struct()
    cv2.pool_id = None
    args[7] = ctypes.byref(cv2)
    assert lib.ouro_tpraos_ledger_checks_host(*args) == _native.OURO_EINVAL
