"""The OCERT counter fold (ouro_ocert_counter_fold; ledger-specs OCERT rule,
CounterTooSmallOCERT) against a dict in Python (ledger.fold_rule), and the
host path of the chain entry that runs it (ouro_chain_validate_ledger_cbor_host)
on a signed chain of four pools."""
import numpy as np
import pytest

import ledger_cases as LC
from ouroboros_network_amd import header as H
from ouroboros_network_amd import ledger as L

K = L.LV_POOL_KNOWN
OK = L.LV_COUNTER_OK


@pytest.fixture(scope="module")
def two_pools():
    rng = np.random.default_rng(8)
    a, b, c = sorted([LC.Key(rng) for _ in range(3)], key=lambda k: k.id)
    views = L.LedgerViews([L.Entry(0, (0, 1), (a.pool((1, 2)), b.pool((1, 2)))),
                           L.Entry(100, (0, 1), (b.pool((1, 3)), c.pool((1, 3))))])
    return views, (a, b, c)


def run(views, table, ledger, rows, ctr):
    got, after = L.counter_fold(ledger, rows, ctr, views, table)
    want, known = L.fold_rule(views, ledger, rows, ctr, table.as_dict())
    np.testing.assert_array_equal(got, want)
    assert after.as_dict() == known
    return got, after


def test_equal_rising_and_falling(two_pools):
    views, (a, b, c) = two_pools
    table = L.Counters([a.id, b.id, c.id], {a.id: 5})
    # rows: a = 0, b = 1 (entry 0); b = 2, c = 3 (entry 1)
    rows = [0, 0, 0, 0, 1, 1, 2, 3, 3]
    ctr = [5, 6, 6, 4, 0, 0, 1, 2**64 - 1, 2**64 - 2]
    got, after = run(views, table, [K] * 9, rows, ctr)
    # a: 5 <= 5, 5 <= 6, 6 <= 6, 6 > 4; b absent then present (0, 0, rising to 1 through
    # its row in the other entry); c absent: 0 <= 2^64 - 1, then falling
    assert [bool(x & OK) for x in got] == [True, True, True, False, True, True, True, True, False]
    assert after.as_dict() == {a.id: 4, b.id: 1, c.id: 2**64 - 2}   # stored as given


def test_absent_then_present_and_zero(two_pools):
    views, (a, b, c) = two_pools
    table = L.Counters([a.id, b.id, c.id])
    got, after = run(views, table, [K, K], [0, 0], [0, 0])
    assert all(x & OK for x in got) and after.as_dict() == {a.id: 0}
    # present with counter 7: 3 falls
    got, _ = run(views, L.Counters([a.id, b.id, c.id], {a.id: 7}), [K], [0], [3])
    assert not got[0] & OK


def test_skipped_rows_do_not_move_the_state(two_pools):
    views, (a, b, c) = two_pools
    table = L.Counters([a.id, b.id, c.id], {a.id: 5, b.id: 9})
    ledger = [0, L.LV_OVERLAY | L.LV_KES_PERIOD_OK, L.LV_KES_PERIOD_OK, L.LV_OVERLAY | K,
              K | L.LV_VRF_KEY_OK]
    rows = [L.LV_NO_POOL, L.LV_NO_POOL, L.LV_NO_POOL, 0, 1]
    got, after = run(views, table, ledger, rows, [1, 1, 1, 1, 9])
    assert list(got[:4]) == ledger[:4] and got[4] == ledger[4] | OK
    assert after.as_dict() == {a.id: 5, b.id: 9}
    # a COUNTER_OK bit that comes in set on a falling row is cleared
    got, _ = run(views, table, [K | OK], [0], [4])
    assert got[0] == K


def test_chaining_two_calls_equals_one(two_pools):
    views, (a, b, c) = two_pools
    rng = np.random.default_rng(21)
    n = 300
    rows = rng.integers(0, 4, n)
    ctr = rng.integers(0, 6, n)
    ledger = np.where(rng.integers(0, 5, n) == 0, L.LV_KES_PERIOD_OK, K).astype(np.uint8)
    table = L.Counters([a.id, b.id, c.id], {b.id: 2})
    one, after1 = run(views, table, ledger, rows, ctr)
    for cut in (0, 1, 137, n):
        g1, mid = L.counter_fold(ledger[:cut], rows[:cut], ctr[:cut], views, table)
        g2, after2 = L.counter_fold(ledger[cut:], rows[cut:], ctr[cut:], views, mid)
        np.testing.assert_array_equal(np.concatenate([g1, g2]), one)
        assert after2.as_dict() == after1.as_dict()


def test_table_must_hold_every_view_pool(two_pools):
    views, (a, b, c) = two_pools
    for ids in ([a.id, b.id], [b.id, c.id], [a.id, c.id], []):
        with pytest.raises(ValueError):
            L.counter_fold([K], [0], [0], views, L.Counters(ids))
    with pytest.raises(ValueError):   # out of order
        L.counter_fold([K], [0], [0], views, L.Counters([c.id, b.id, a.id], sort=False))
    # a table with more pools than the views is fine
    extra = L.Counters([a.id, b.id, c.id, b"\xff" * 28], {b"\xff" * 28: 3})
    _, after = run(views, extra, [K], [3], [1])
    assert after.as_dict() == {c.id: 1, b"\xff" * 28: 3}


def test_host_entry_runs_the_fold(two_pools):
    """ouro_tpraos_ledger_checks_host with counters: bits and fold in one call"""
    views, (a, b, c) = two_pools
    rows = [LC._row(a.cold, a.vrf, 5, bytes(64), 0, 4), LC._row(a.cold, a.vrf, 6, bytes(64), 0, 3),
            LC._row(c.cold, c.vrf, 7, bytes(64), 0, 9), LC._row(c.cold, c.vrf, 107, bytes(64), 1, 0)]
    cols = LC.columns(rows)
    table = L.Counters([a.id, b.id, c.id], {a.id: 4})
    bits, prow = LC.expect(views, LC.G_MAIN, rows)
    want, known = L.fold_rule(views, bits, prow, cols[5], table.as_dict())
    got = L.ledger_checks(*cols[:5], views, LC.G_MAIN, ocert_counter=cols[5], counters=table,
                          host=True)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], prow)
    assert got[2].as_dict() == known == {a.id: 3, c.id: 0}
    assert [bool(x & OK) for x in want] == [True, False, False, True]


def test_chain_entry_on_the_host_path():
    """ouro_chain_validate_ledger_cbor_host on the signed four-pool chain behind
    250 Byron headers: the ledger bits, rows and counters from the Python
    rule; everything else byte-identical to ouro_chain_validate_cbor_host"""
    import envelope_cases as EC

    s = LC.chain_stream()
    table = L.Counters(s["table_ids"], s["known"])
    got = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       counters=table, cfg=EC.VAL_CFG, epochs=s["epochs"],
                                       nonce=True, host=True)
    ref = H.validate_chain_cbor(s["raws"], LC.SPKP, -1, cfg=EC.VAL_CFG, epochs=s["epochs"],
                                nonce=True, host=True)
    for x, y in zip(ref[0], got[0]):
        assert x.tobytes() == y.tobytes()
    assert ref[1].tobytes() == got[1].tobytes() and ref[2].tobytes() == got[2].tobytes()
    assert ref[3] == got[3] and ref[4] == got[4]
    nb = s["n_byron"]
    assert (got[0][2][nb:] & 0x0F == 0x0F).all()        # every TPraos header verifies
    ledger, prow, known = LC.chain_expect(s)
    np.testing.assert_array_equal(got[5], ledger)
    np.testing.assert_array_equal(got[6], prow)
    assert got[7].as_dict() == known
    tp = ledger[nb:]
    # the cases the chain was built for are all there
    assert (tp & L.LV_POOL_KNOWN == 0).sum() >= 3                       # the unregistered pool
    assert ((tp & 0x03) == 0x01).sum() >= 1                             # a wrong VRF hash
    assert ((tp & 0x47) == 0x03).sum() >= 3                             # the 2^-60 stake: NO
    assert ((tp & 0x17) == 0x07).sum() >= 2                             # falling counters
    assert not tp[6] & OK and not tp[20] & OK
    assert (tp & L.LV_OVERLAY).any() and (tp == 0x1f).sum() >= 10
    # without counters: no fold, COUNTER_OK clear
    got2 = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                        cfg=EC.VAL_CFG, epochs=s["epochs"], host=True)
    np.testing.assert_array_equal(got2[5], ledger & ~np.uint8(OK))
    assert got2[7] is None
    # the globals' slots per KES period must be the call's
    with pytest.raises(ValueError):
        H.validate_chain_ledger_cbor(s["raws"], LC.SPKP + 1, -1, s["views"], LC.G_CHAIN,
                                     cfg=EC.VAL_CFG, epochs=s["epochs"], host=True)
