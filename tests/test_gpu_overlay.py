"""The genesis-delegate branch of the ledger-view checks on the device
(k_ledger_checks_overlay through ouro_tpraos_ledger_checks_overlay, the
device-pointer form behind ouro_ledger_views_upload_overlay, and the stage
behind the header kernel in ouro_chain_validate_ledger_overlay_cbor) against
the Python rule (ledger.rule / fold_rule with ``genesis``) on the rows of
tests/test_overlay_rule.py and on the chain that pools and delegates forge
together."""
import ctypes

import numpy as np
import pytest

import envelope_cases as EC
import ledger_cases as LC
import overlay_cases as OC
from ouroboros_network_amd import _native
from ouroboros_network_amd import header as H
from ouroboros_network_amd import ledger as L

pytestmark = pytest.mark.gpu


def test_all_rows_on_the_device(gpu_lib):
    v, _, _, gens = OC.views()
    for a, rows, bits, prow in OC.all_rows():
        got = L.ledger_checks(*LC.columns(rows)[:5], v, LC.G_MAIN, genesis=gens[a])
        np.testing.assert_array_equal(got[0], bits)
        np.testing.assert_array_equal(got[1], prow)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wave_and_a_block(gpu_lib, n):
    """n rows spread over the cases of each schedule; the other globals too"""
    v, _, _, gens = OC.views()
    for a, rows, bits, prow in OC.all_rows():
        idx = [(i * 37 + n) % len(rows) for i in range(n)]
        sub = [rows[i] for i in idx]
        got = L.ledger_checks(*LC.columns(sub)[:5], v, LC.G_MAIN, genesis=gens[a])
        np.testing.assert_array_equal(got[0], bits[idx])
        np.testing.assert_array_equal(got[1], prow[idx])
    for g in (LC.G_ONE, LC.G_BAD[0]):
        want = OC.expect(v, g, sub, gens[a])
        got = L.ledger_checks(*LC.columns(sub)[:5], v, g, genesis=gens[a])
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_one_wave_whose_lanes_mix_every_outcome(gpu_lib):
    """64 rows, the six outcomes round robin: neighbouring lanes take the pool
    search, the delegate compare, or neither, and meet again at the VRF hash"""
    v, _, _, gens = OC.views()
    a, rows, bits, prow = OC.all_rows()[1]
    by = {o: [i for i, b in enumerate(bits) if o in OC.outcome(b)] for o in OC.OUTCOMES}
    idx = [by[OC.OUTCOMES[i % 6]][i // 6] for i in range(64)]
    assert {o for i in idx for o in OC.outcome(bits[i])} == set(OC.OUTCOMES)
    got = L.ledger_checks(*LC.columns([rows[i] for i in idx])[:5], v, LC.G_MAIN, genesis=gens[a])
    np.testing.assert_array_equal(got[0], bits[idx])
    np.testing.assert_array_equal(got[1], prow[idx])


def test_long_schedule_and_the_fold(gpu_lib):
    """k = 4,096 entries of 7 genesis rows each, at both ends and in the middle,
    with the counter fold over pools and delegates in the same call"""
    v, ks, ds, gen = OC.views_k(4096)
    assert gen.rows == 7 * 4096
    rng = np.random.default_rng(6)
    rows = []
    for j in (0, 1, 2047, 2048, 4094, 4095):
        for s in range(10):                      # d = 1/2, asc_inv = 1: even s schedules key s / 2
            k = ds[(s // 2) % 7] if s % 2 == 0 and s != 4 else ks[s % 2]
            rows.append(LC._row(k.cold, k.vrf, 10 * j + s, LC._beta(rng), (10 * j + s) // LC.SPKP,
                                int(rng.integers(0, 3))))
    cols = LC.columns(rows)
    bits, prow = OC.expect(v, LC.G_MAIN, rows, gen)
    assert {int(p) for p in prow} >= {0, 7 * 4095 + 4, 7 * 2048 + 1}
    table = OC.table_for(v, gen, {ds[0].id: 1, ks[0].id: 2})
    want, known = L.fold_rule(v, bits, prow, cols[5], table.as_dict(), genesis=gen)
    got = L.ledger_checks(*cols[:5], v, LC.G_MAIN, genesis=gen, ocert_counter=cols[5],
                          counters=table)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], prow)
    assert got[2].as_dict() == known
    assert (want & L.LV_COUNTER_OK).any() and ((want & 0x51) == 0x41).any()


def test_device_pointer_form(gpu_lib):
    import torch

    v, _, _, gens = OC.views()
    a, rows, bits, prow = OC.all_rows()[2]
    cols = LC.columns(rows)
    dev = torch.device("cuda", 0)
    d = [torch.tensor(c.view(np.int64) if c.dtype == np.uint64 else c, device=dev)
         for c in cols[:5]]
    n = len(rows)
    cv, cg, cgen = v.c_struct(), LC.G_MAIN.c_struct(), gens[a].c_struct()
    stream = torch.cuda.current_stream()
    for gen_arg, want in ((ctypes.byref(cgen), (bits, prow)),
                          (None, LC.expect(v, LC.G_MAIN, rows))):    # NULL: the plain upload
        ledger = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        prow_d = torch.full((n,), 5, dtype=torch.int32, device=dev)
        h = ctypes.c_void_p()
        _native.check(gpu_lib.ouro_ledger_views_upload_overlay(ctypes.byref(cv), gen_arg,
                                                               ctypes.byref(h)),
                      "ouro_ledger_views_upload_overlay")
        try:
            args = [ctypes.c_void_p(stream.cuda_stream), n] + [t.data_ptr() for t in d] + \
                [h, ctypes.byref(cg), ledger.data_ptr(), prow_d.data_ptr()]
            _native.check(gpu_lib.ouro_tpraos_ledger_checks_device(*args),
                          "ouro_tpraos_ledger_checks_device")
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ledger.cpu().numpy(), want[0])
            np.testing.assert_array_equal(prow_d.cpu().numpy().view(np.uint32), want[1])
        finally:
            gpu_lib.ouro_ledger_views_free(h)
    # a bad schedule is refused by the upload
    bad = L.GenesisDelegs(gens[a].entries, 0).c_struct()
    h = ctypes.c_void_p()
    assert gpu_lib.ouro_ledger_views_upload_overlay(ctypes.byref(cv), ctypes.byref(bad),
                                                    ctypes.byref(h)) == _native.OURO_EINVAL


def check_chain(s, **kw):
    table = L.Counters(s["table_ids"], s["known"])
    got = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       genesis=s["genesis"], counters=table, cfg=EC.VAL_CFG,
                                       epochs=s["epochs"], nonce=True, **kw)
    ledger, prow, known = OC.chain_expect(s)
    np.testing.assert_array_equal(got[5], ledger)
    np.testing.assert_array_equal(got[6], prow)
    assert got[7].as_dict() == known
    return got


@pytest.mark.parametrize("slots", [1, 3, 6])
def test_chain_entry_in_256_header_chunks(gpu_lib, small_chunks, slots):
    """Byron headers in front, chunk 0 mixed, delegate 0's counter step across
    the chunk boundary; crypto, envelope and the non-overlay ledger rows
    byte-identical to ouro_chain_validate_ledger_cbor"""
    s = OC.chain_stream()
    small_chunks(CHUNK=256, SLOTS=slots)
    got = check_chain(s)
    table = L.Counters(s["table_ids"], s["known"])
    ref = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       counters=table, cfg=EC.VAL_CFG, epochs=s["epochs"],
                                       nonce=True)
    for x, y in zip(ref[0], got[0]):
        assert x.tobytes() == y.tobytes()
    assert ref[1].tobytes() == got[1].tobytes() and ref[2].tobytes() == got[2].tobytes()
    assert ref[3] == got[3] and ref[4] == got[4]
    plain = (got[5] & L.LV_OVERLAY) == 0
    np.testing.assert_array_equal(ref[5] & L.LV_OVERLAY, got[5] & L.LV_OVERLAY)
    assert got[5][plain].tobytes() == ref[5][plain].tobytes()
    assert got[6][plain].tobytes() == ref[6][plain].tobytes()
    nb = s["n_byron"]
    assert nb < 256 < len(s["raws"]) and (got[0][2][nb:] & 0x0F == 0x0F).all()
    tp = got[5][nb:]
    full = L.LV_ALL_OK | L.LV_OVERLAY | L.LV_OVERLAY_ACTIVE
    assert tp[5] == full and tp[6] == full & ~L.LV_COUNTER_OK       # headers 255 and 256


def test_chain_entry_in_one_chunk(gpu_lib):
    check_chain(OC.chain_stream())


@pytest.mark.device_error
def test_device_error_recomputes_on_the_host_path(gpu_lib):
    s = OC.chain_stream()
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1", OURO_CBOR_CHUNK="256"):
        check_chain(s)
        msg = gpu_lib.ouro_last_error().decode()
        assert "recomputed on the host path" in msg, msg
    v, _, _, gens = OC.views()
    a, rows, bits, prow = OC.all_rows()[0]
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1"):
        got = L.ledger_checks(*LC.columns(rows[:300])[:5], v, LC.G_MAIN, genesis=gens[a])
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
    np.testing.assert_array_equal(got[0], bits[:300])
    np.testing.assert_array_equal(got[1], prow[:300])
