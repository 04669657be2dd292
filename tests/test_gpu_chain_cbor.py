"""The epoch-nonce schedule and the combined raw entry on the device:
ouro_tpraos_verify_batch_epochs (mkSeed's eta0 looked up per header inside the
header kernel) and ouro_chain_verify_cbor (each header classified while it is
gathered; one-era chunks on that era's path, mixed chunks through the Byron
slicer + ByronDSIGN kernel and the TPraos slicer + header kernel on one upload,
results scattered back), with its multi-device form.

The cases and their expected values are those of tests/test_epochs.py and
tests/test_chain_cbor.py (chain_cases.py: host slicers + the oracle, per-row
alphas built in Python), repeated by index to about 800 rows and cut into
256-header chunks over 3 slots.  conftest's _no_silent_host_recompute fails
any of these if the device path fell back to the host.
"""
import functools

import numpy as np
import pytest

import chain_cases as K
from test_epochs import check_epochs, seeded_batch

pytestmark = pytest.mark.gpu

MAGIC = -1
ROWS = 800


# ---- the schedule inside the header kernel -------------------------------------
@pytest.mark.parametrize("swapped", [False, True], ids=["proved", "swapped"])
def test_three_epochs_on_the_device(gpu_lib, swapped):
    from ouroboros_network_amd import tpraos as T

    raws, _slots, _ea, _la, want = K.epoch3(swapped)
    v = check_epochs(T.verify_headers, raws, K.sched3(), want)
    bad = (1, 2, 4, 5) if swapped else ()
    for i in range(len(raws)):
        if i in bad:
            assert v[i] & 0x0C == 0 and v[i] & 0x03 == 0x03
        else:
            assert v[i] == K.STRICT


@pytest.mark.parametrize("k", [2, 4096])
def test_search_ends_and_middle_on_the_device(gpu_lib, k):
    from ouroboros_network_amd import tpraos as T

    E, raws, _slots, want = K.sched_k_cases(k)
    v = check_epochs(T.verify_headers, raws, E, want)
    assert (v == K.STRICT).all()


@pytest.mark.parametrize("nonce", [b"\x5a" * 32, None], ids=["nonce", "neutral"])
def test_one_entry_is_the_single_nonce_call_on_the_device(gpu_lib, kats, nonce):
    from ouroboros_network_amd import tpraos as T

    slots = [0, 7, 2**33, 2**64 - 1, 12345, 999] * 50  # more than one workgroup
    raws = K.seeded_raw_at(kats, slots[:6], [nonce] * 6)
    b = seeded_batch([raws[i % 6] for i in range(len(slots))])
    E = T.EpochNonces(first_slot=[0], nonce=[nonce or b"\xaa" * 32],
                      neutral=None if nonce else [1])
    got = T.verify_headers(b, nonce=True, epochs=E)
    ref = T.verify_headers(
        b.with_(epoch_nonce=np.frombuffer(nonce, np.uint8) if nonce else None), nonce=True)
    for a, r in zip(got, ref):
        assert a.tobytes() == r.tobytes()
    assert (got[0] == K.STRICT).all()


# ---- the combined entry through the pipeline -----------------------------------
@functools.lru_cache(maxsize=None)
def _case_set(name):
    """(raws, eta_alpha, leader_alpha, epochs, want) of a case set"""
    if name == "fixtures":
        raws, ea, la, _kinds, want = K.fixtures15()
        return raws, ea, la, None, want
    if name == "corruptions":
        raws, ea, la, want = K.corruptions()
        return raws, ea, la, None, want
    raws, want = K.three_epoch_stream()
    return raws, None, None, K.sched3(), want


def _order(proto, order):
    """row indices of the case set, repeated to about ROWS rows in one of the
    four orders"""
    b = np.nonzero(proto == 0)[0]
    t = np.nonzero(proto == 1)[0]
    rep = lambda a, n: a[np.arange(n) % len(a)]  # noqa: E731
    if order == "byron_then_shelley":  # 400 + 400: the switch inside chunk 1
        return np.concatenate([rep(b, ROWS // 2), rep(t, ROWS // 2)])
    if order == "alternating":
        out = np.empty(ROWS, np.int64)
        out[0::2], out[1::2] = rep(b, ROWS // 2), rep(t, ROWS // 2)
        return out
    return rep(t if order == "pure_shelley" else b, ROWS)


def _run(name, order, devices=None):
    from ouroboros_network_amd import header as H

    raws, ea, la, epochs, want = _case_set(name)
    o = _order(want[0], order)
    rows = [raws[i] for i in o]
    got = H.verify_chain_cbor(rows, K.SPKP, MAGIC, epochs=epochs,
                              eta_alpha=None if ea is None else ea[o],
                              leader_alpha=None if la is None else la[o], nonce=True,
                              devices=devices)
    return rows, o, got, tuple(w[o] for w in want)


@pytest.mark.parametrize("order", ["byron_then_shelley", "alternating", "pure_shelley",
                                   "pure_byron"])
@pytest.mark.parametrize("name", ["fixtures", "corruptions", "three_epochs"])
def test_chain_cbor_orders(gpu_lib, small_chunks, name, order):
    from ouroboros_network_amd import byron as B
    from ouroboros_network_amd import header as H

    small_chunks(CHUNK=256, SLOTS=3)
    rows, o, got, want = _run(name, order)
    K.assert_chain_equal(got, want)
    stats = np.zeros(6)
    gpu_lib.ouro_debug_cbor_stats(stats.ctypes.data)
    assert stats[3] == -(-ROWS // 256) and stats[4] == 3  # whole chunks, never per-header launches
    _raws, ea, la, _epochs, _want = _case_set(name)
    # a pure stream equals the single-era entry byte for byte
    if order == "pure_byron":
        ok, st = B.verify_byron_cbor(rows, B.HEADER_MAGIC)
        assert got[1].tobytes() == st.tobytes()
        assert got[2].tobytes() == ok.astype(np.uint8).tobytes()
        assert not got[3].any() and not got[4].any() and not got[5].any()
    if order == "pure_shelley" and ea is not None:
        v, be, bl, st, en = H.verify_headers_cbor(rows, K.SPKP, eta_alpha=ea[o],
                                                  leader_alpha=la[o], nonce=True)
        for a, r in zip(got[1:], (st, v, be, bl, en)):
            assert a.tobytes() == r.tobytes()


@pytest.mark.parametrize("devices", [[0], [0, 0], "all"], ids=["d0", "d00", "all"])
@pytest.mark.parametrize("name", ["fixtures", "three_epochs"])
def test_chain_cbor_multi(gpu_lib, small_chunks, name, devices):
    small_chunks(CHUNK=256, SLOTS=3)
    _rows, _o, one, want = _run(name, "alternating")
    _rows, _o, got, _want = _run(name, "alternating", devices=devices)
    K.assert_chain_equal(got, want)
    for a, r in zip(got, one):
        assert a.tobytes() == r.tobytes()


@pytest.mark.device_error
def test_device_error_recomputes_on_the_host_path(gpu_lib, small_chunks):
    """OURO_TEST_DEVICE_ERROR (test build): every launch fails; the combined
    entry, its multi-device form and the epochs batch entry still return the
    oracle's verdicts, from the host path's own partition and lookup"""
    from ouroboros_network_amd import _native
    from ouroboros_network_amd import tpraos as T

    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1", OURO_CBOR_CHUNK="256"):
        for devices in (None, [0, 0]):
            for name in ("fixtures", "three_epochs"):
                _rows, _o, got, want = _run(name, "alternating", devices)
                K.assert_chain_equal(got, want)
                if devices is None:  # (a shard's message stays with its worker thread)
                    assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
        raws, _slots, _ea, _la, want = K.epoch3()
        check_epochs(T.verify_headers, raws, K.sched3(), want)
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
