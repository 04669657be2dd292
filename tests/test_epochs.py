"""The epoch-nonce schedule on the host path (CPU-only):
ouro_tpraos_verify_batch_epochs_host looks up mkSeed's eta0 per header by its
slot (csrc/tpraos.h hdr_mkseed, the routine the kernels run, compiled for the
CPU), so one call verifies headers of several epochs.

Expected values: the pinned host slicer + the oracle's header combiner with
explicit per-row alphas built in Python (chain_cases.py); the schedule never
reaches the oracle.  tests/test_gpu_chain_cbor.py runs the same cases on the
device.
"""
import ctypes

import numpy as np
import pytest

import chain_cases as K
from ouroboros_network_amd import _native
from ouroboros_network_amd import header as H
from ouroboros_network_amd import tpraos as T


def seeded_batch(raws):
    """the raw headers as a batch that carries slots (no nonce, no alphas)"""
    p = H.pack_cbor(raws, slots_per_kes_period=K.SPKP, seeds=True)
    assert (p.status == H.PACK_OK).all()
    return p.batch


def check_epochs(verify, raws, E, want):
    v, be, bl, en = verify(seeded_batch(raws), nonce=True, epochs=E)
    np.testing.assert_array_equal(v, want[0])
    np.testing.assert_array_equal(be, want[1])
    np.testing.assert_array_equal(bl, want[2])
    np.testing.assert_array_equal(en, want[3])
    return v


def test_three_epochs_boundary_slots():
    """slots 0, 999 | 1000, 1001, 4999 | 5000, 2^40, 2^64-1 under {neutral,
    0x33.., random}: every header strict-OK, outputs and nonces the oracle's"""
    raws, slots, _ea, _la, want = K.epoch3()
    assert list(slots) == K.SCHED3_SLOTS
    v = check_epochs(T.verify_headers_host, raws, K.sched3(), want)
    assert (v == K.STRICT).all()
    assert (want[1] != 0).any(axis=1).all()


def test_proofs_of_the_neighbouring_epoch_fail():
    """rows 999 <-> 1000 and 4999 <-> 5000 carry each other's proofs: both VRF
    bits clear there, OCERT and KES still set; the other rows strict-OK"""
    raws, _slots, _ea, _la, want = K.epoch3(swapped=True)
    v = check_epochs(T.verify_headers_host, raws, K.sched3(), want)
    for i in (1, 2, 4, 5):
        assert v[i] & 0x0C == 0 and v[i] & 0x03 == 0x03, (i, v[i])
    for i in (0, 3, 6, 7):
        assert v[i] == K.STRICT


@pytest.mark.parametrize("nonce", [b"\x5a" * 32, None], ids=["nonce", "neutral"])
def test_one_entry_is_the_single_nonce_call(kats, nonce):
    """k = 1: byte-identical verdicts, outputs and nonces to
    ouro_tpraos_verify_batch_host with that epoch_nonce"""
    slots = [0, 7, 2**33, 2**64 - 1, 12345, 999]
    raws = K.seeded_raw_at(kats, slots, [nonce] * len(slots))
    raws[2] = raws[2][:-1] + bytes([raws[2][-1] ^ 1])  # a KES failure travels too
    b = seeded_batch(raws)
    E = T.EpochNonces(first_slot=[0], nonce=[nonce or b"\xaa" * 32],
                      neutral=None if nonce else [1])
    got = T.verify_headers_host(b, nonce=True, epochs=E)
    ref = T.verify_headers_host(
        b.with_(epoch_nonce=np.frombuffer(nonce, np.uint8) if nonce else None), nonce=True)
    for a, r in zip(got, ref):
        assert a.tobytes() == r.tobytes()
    assert (got[0][[0, 1, 3, 4, 5]] == K.STRICT).all() and got[0][2] & 0x02 == 0


@pytest.mark.parametrize("k", [2, 4096])
def test_both_ends_and_the_middle_of_the_search(k):
    """first_slot = 0, 10, 20, ...: entries 0, 1, 2047, 2048, 4094, 4095 on
    their first and last slots"""
    E, raws, slots, want = K.sched_k_cases(k)
    assert len(raws) == (4 if k == 2 else 12)
    v = check_epochs(T.verify_headers_host, raws, E, want)
    assert (v == K.STRICT).all()


def _raw_call(b, e_struct, lib_fn):
    n = len(b)
    v = np.full(n, 0xEE, np.uint8)
    be = np.full((n, 64), 0xEE, np.uint8)
    bl = np.full((n, 64), 0xEE, np.uint8)
    en = np.full((n, 32), 0xEE, np.uint8)
    s = b.c_struct(en)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib_fn(ctypes.byref(s), ctypes.byref(e_struct) if e_struct is not None else None,
                ptr(v), ptr(be), ptr(bl))
    untouched = all((a == 0xEE).all() for a in (v, be, bl, en))
    return rc, untouched


def _estruct(first_slot, nonce, k=None):
    fs = np.array(first_slot, np.uint64)
    e = _native.EpochNonces()
    e.k = len(fs) if k is None else k
    e.first_slot = fs.ctypes.data
    e.nonce = None if nonce is None else nonce.ctypes.data
    e.neutral = None
    e._keep = (fs, nonce)
    return e


BAD_SCHEDULES = [
    ("k0", lambda nz: _estruct([0], nz, k=0), "k outside"),
    ("k4097", lambda nz: _estruct(list(range(4097)), nz), "k outside"),
    ("first1", lambda nz: _estruct([1, 5], nz), "first_slot[0]"),
    ("equal", lambda nz: _estruct([0, 5, 5], nz), "strictly increasing"),
    ("decreasing", lambda nz: _estruct([0, 9, 8], nz), "strictly increasing"),
    ("nullnonce", lambda nz: _estruct([0, 5], None), "null"),
]


@pytest.mark.parametrize("name,make,why", BAD_SCHEDULES, ids=[b[0] for b in BAD_SCHEDULES])
def test_bad_schedule_is_einval(name, make, why):
    lib = _native.load()
    raws, *_ = K.epoch3()
    b = seeded_batch(raws[:2])
    nz = np.zeros((4097, 32), np.uint8)
    rc, untouched = _raw_call(b, make(nz), lib.ouro_tpraos_verify_batch_epochs_host)
    assert rc == _native.OURO_EINVAL and untouched
    assert why in lib.ouro_last_error().decode()
    # the device entry checks its arguments before it looks for a device
    rc, untouched = _raw_call(b, make(nz), lib.ouro_tpraos_verify_batch_epochs)
    assert rc == _native.OURO_EINVAL and untouched


def test_bad_batch_is_einval():
    lib = _native.load()
    raws, *_ = K.epoch3()
    b = seeded_batch(raws[:2])
    nz = np.zeros((2, 32), np.uint8)
    good = _estruct([0, 5], nz)
    z = np.zeros((2, 32), np.uint8)
    for bad, why in ((b.with_(slot=None, eta_alpha=z, leader_alpha=z), "slot"),
                     (b.with_(epoch_nonce=np.zeros(32, np.uint8)), "epoch_nonce"),
                     (b.with_(eta_alpha=z, leader_alpha=z), "alpha")):
        for fn in (lib.ouro_tpraos_verify_batch_epochs_host, lib.ouro_tpraos_verify_batch_epochs):
            rc, untouched = _raw_call(bad, good, fn)
            assert rc == _native.OURO_EINVAL and untouched, why
            assert why in lib.ouro_last_error().decode()
    rc, untouched = _raw_call(b, None, lib.ouro_tpraos_verify_batch_epochs_host)
    assert rc == _native.OURO_EINVAL and untouched


def test_python_schedule_validates_the_same_rules():
    nz = np.zeros((3, 32), np.uint8)
    for fs in ([], [1, 2, 3], [0, 5, 5], [0, 9, 8], list(range(4097))):
        with pytest.raises(ValueError):
            T.EpochNonces(first_slot=fs, nonce=np.zeros((max(len(fs), 1), 32), np.uint8))
    with pytest.raises(ValueError):
        T.EpochNonces(first_slot=[0, 1, 2], nonce=None)
    with pytest.raises(ValueError):
        T.EpochNonces(first_slot=[0, 1, 2], nonce=nz[:2])
    with pytest.raises(ValueError):
        T.EpochNonces(first_slot=[0, 1, 2], nonce=nz, neutral=[1])
    E = K.sched3()
    assert [E.nonce_of(s) for s in K.SCHED3_SLOTS] == [K.sched3_nonce(s) for s in K.SCHED3_SLOTS]
