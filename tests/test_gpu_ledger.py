"""The ledger-view checks on the device (k_ledger_checks through
ouro_tpraos_ledger_checks, its device-pointer form, and the stage behind the
header kernel in ouro_chain_validate_ledger_cbor) against the Python rule
(ledger.rule / fold_rule) on the cases of tests/test_ledger_rule.py and on a
signed, linked chain of four pools."""
import ctypes

import numpy as np
import pytest

import envelope_cases as EC
import ledger_cases as LC
from ouroboros_network_amd import _native
from ouroboros_network_amd import header as H
from ouroboros_network_amd import ledger as L

pytestmark = pytest.mark.gpu


def test_all_cases_on_the_device(gpu_lib):
    views, _ = LC.main_views()
    cols = LC.columns(LC.main_rows())
    bits, prow = LC.main_expect()
    got = L.ledger_checks(*cols[:5], views, LC.G_MAIN)
    np.testing.assert_array_equal(got[0], bits)
    np.testing.assert_array_equal(got[1], prow)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wave_and_a_block(gpu_lib, n):
    """n rows spread over the cases; the other globals on the same rows"""
    views, _ = LC.main_views()
    rows = LC.main_rows()
    idx = [(i * 37 + n) % len(rows) for i in range(n)]
    sub = [rows[i] for i in idx]
    bits, prow = LC.main_expect()
    got = L.ledger_checks(*LC.columns(sub)[:5], views, LC.G_MAIN)
    np.testing.assert_array_equal(got[0], bits[idx])
    np.testing.assert_array_equal(got[1], prow[idx])
    for g in (LC.G_ONE, LC.G_BAD[0]):
        want = LC.expect(views, g, sub)
        got = L.ledger_checks(*LC.columns(sub)[:5], views, g)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_long_schedule_and_the_fold(gpu_lib):
    """k = 4,096 entries at both ends and in the middle, with the counter fold
    in the same call"""
    views, ks = LC.views_k(4096)
    rng = np.random.default_rng(6)
    rows = []
    for j in (0, 1, 2047, 2048, 4094, 4095):
        for slot in (10 * j, 10 * j + 9, max(10 * j - 1, 0)):
            k = ks[len(rows) % 2]
            rows.append(LC._row(k.cold, k.vrf, slot, LC._beta(rng), slot // LC.SPKP,
                                int(rng.integers(0, 3))))
    cols = LC.columns(rows)
    bits, prow = LC.expect(views, LC.G_MAIN, rows)
    table = L.Counters([k.id for k in ks], {ks[0].id: 1})
    want, known = L.fold_rule(views, bits, prow, cols[5], table.as_dict())
    got = L.ledger_checks(*cols[:5], views, LC.G_MAIN, ocert_counter=cols[5], counters=table)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], prow)
    assert got[2].as_dict() == known


def test_device_pointer_form(gpu_lib):
    import torch

    views, _ = LC.main_views()
    rows = LC.main_rows()[:700]
    cols = LC.columns(rows)
    bits, prow = LC.main_expect()
    dev = torch.device("cuda", 0)
    d = [torch.tensor(c.view(np.int64) if c.dtype == np.uint64 else c, device=dev)
         for c in cols[:5]]
    n = len(rows)
    ledger = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    prow_d = torch.full((n,), 5, dtype=torch.int32, device=dev)
    cv, cg = views.c_struct(), LC.G_MAIN.c_struct()
    h = ctypes.c_void_p()
    _native.check(gpu_lib.ouro_ledger_views_upload(ctypes.byref(cv), ctypes.byref(h)),
                  "ouro_ledger_views_upload")
    try:
        stream = torch.cuda.current_stream()
        args = [ctypes.c_void_p(stream.cuda_stream), n] + [t.data_ptr() for t in d] + \
            [h, ctypes.byref(cg), ledger.data_ptr(), prow_d.data_ptr()]
        _native.check(gpu_lib.ouro_tpraos_ledger_checks_device(*args),
                      "ouro_tpraos_ledger_checks_device")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ledger.cpu().numpy(), bits[:n])
        np.testing.assert_array_equal(prow_d.cpu().numpy().view(np.uint32), prow[:n])
        # refused before anything is enqueued
        bad = list(args)
        bad[2] = d[0].data_ptr() + 1
        assert gpu_lib.ouro_tpraos_ledger_checks_device(*bad) == _native.OURO_EINVAL
        bad = list(args)
        bad[7] = None
        assert gpu_lib.ouro_tpraos_ledger_checks_device(*bad) == _native.OURO_EINVAL
    finally:
        gpu_lib.ouro_ledger_views_free(h)
    bad = L.LedgerViews([L.Entry(3, (0, 1), ())]).c_struct()
    assert gpu_lib.ouro_ledger_views_upload(ctypes.byref(bad), ctypes.byref(h)) == \
        _native.OURO_EINVAL


def check_chain(s, **kw):
    table = L.Counters(s["table_ids"], s["known"])
    got = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       counters=table, cfg=EC.VAL_CFG, epochs=s["epochs"],
                                       nonce=True, **kw)
    ledger, prow, known = LC.chain_expect(s)
    np.testing.assert_array_equal(got[5], ledger)
    np.testing.assert_array_equal(got[6], prow)
    assert got[7].as_dict() == known
    return got


@pytest.mark.parametrize("slots", [1, 3, 6])
def test_chain_entry_in_256_header_chunks(gpu_lib, small_chunks, slots):
    """Byron headers in front, chunk 0 mixed, a counter step across the chunk
    boundary; crypto and envelope byte-identical to ouro_chain_validate_cbor"""
    s = LC.chain_stream()
    small_chunks(CHUNK=256, SLOTS=slots)
    got = check_chain(s)
    ref = H.validate_chain_cbor(s["raws"], LC.SPKP, -1, cfg=EC.VAL_CFG, epochs=s["epochs"],
                                nonce=True)
    for x, y in zip(ref[0], got[0]):
        assert x.tobytes() == y.tobytes()
    assert ref[1].tobytes() == got[1].tobytes() and ref[2].tobytes() == got[2].tobytes()
    assert ref[3] == got[3] and ref[4] == got[4]
    nb = s["n_byron"]
    assert nb < 256 < len(s["raws"]) and (got[0][2][nb:] & 0x0F == 0x0F).all()


def test_chain_entry_in_one_chunk_and_chained_calls(gpu_lib):
    """the default chunk size; and the stream cut into two calls, the second
    starting from the first's tip and counters"""
    s = LC.chain_stream()
    whole = check_chain(s)
    ledger, prow, known = LC.chain_expect(s)
    cut = 270
    table = L.Counters(s["table_ids"], s["known"])
    a = H.validate_chain_ledger_cbor(s["raws"][:cut], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                     counters=table, cfg=EC.VAL_CFG, epochs=s["epochs"])
    b = H.validate_chain_ledger_cbor(s["raws"][cut:], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                     counters=a[7], cfg=EC.VAL_CFG, epochs=s["epochs"], tip=a[3])
    np.testing.assert_array_equal(np.concatenate([a[5], b[5]]), ledger)
    np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), whole[2])
    assert b[7].as_dict() == known and b[3] == whole[3]


@pytest.mark.device_error
def test_chain_device_error_recomputes_on_the_host_path(gpu_lib):
    s = LC.chain_stream()
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1", OURO_CBOR_CHUNK="256"):
        check_chain(s)
        msg = gpu_lib.ouro_last_error().decode()
        assert "recomputed on the host path" in msg, msg
    views, _ = LC.main_views()
    rows = LC.main_rows()[:300]
    bits, prow = LC.main_expect()
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1"):
        got = L.ledger_checks(*LC.columns(rows)[:5], views, LC.G_MAIN)
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
    np.testing.assert_array_equal(got[0], bits[:300])
    np.testing.assert_array_equal(got[1], prow[:300])
