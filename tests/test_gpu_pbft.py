"""The Byron ledger-view checks on the device: k_pbft_checks and
k_byron_key_hash (csrc/kernels_pbft.hip) against the library's host path and
the plain-Python restatement (pbft.pbft_rule, hashlib), at sizes around a wave
and a block, with a long schedule, past the launch's grid cap, in the
device-pointer form on a caller's stream, and after an injected device
error."""
import ctypes

import numpy as np
import pytest

import pbft_cases as PC
from ouroboros_network_amd import _native
from ouroboros_network_amd import pbft as P
from ouroboros_network_amd._native import LV_NO_POOL

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257]
# csrc/launches.h kPbftBlocksMax (4096 blocks, the value of launch_ledger's cap) times
# csrc/launch.h kBlock (256 lanes): the lanes of the capped grid
GRID_CAP_ROWS = 4096 * 256


def _wave_rows(n):
    """n rows whose every 64 mix every outcome, slots ascending across the
    three entries so the fold passes and fails on both of its checks"""
    vk, slot, status = PC.tile(PC.mixed_wave(), n)
    slot = np.sort(slot, kind="stable")
    return vk, slot, status


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host_equals_rule(gpu_lib, n):
    v = PC.schedule(3, 3, 10, 3)
    vk, slot, status = _wave_rows(n)
    keys = [r.tobytes() for r in vk]
    st0 = P.PBftState([(0, PC.gen_id(1))] * 3)
    want = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), st0)
    host = P.pbft_checks(vk, slot, status, v, state=st0, host=True)
    got = P.pbft_checks(vk, slot, status, v, state=st0)
    for q in range(3):
        np.testing.assert_array_equal(got[q], want[q])
        np.testing.assert_array_equal(host[q], want[q])
    assert got[3] == want[3] == host[3]
    if n >= 64:  # one wave holds every outcome of the lookup
        w = want[0][:64]
        assert (w & P.PBFT_BOUNDARY).any() and (w == 0).any() and (w & 1).any()
        assert set(status[:64].tolist()) == {PC.OK, PC.EBB, PC.ESHELLEY, PC.ECBOR}
        assert ((want[0][:64] == 0) & (status[:64] == PC.OK)).any()
    # without a state: the lookup alone
    nb, nr, _ = P.pbft_checks(vk, slot, status, v)
    lb, lr, _, _ = P.pbft_rule(v, keys, slot.tolist(), status.tolist())
    np.testing.assert_array_equal(nb, lb)
    np.testing.assert_array_equal(nr, lr)


@pytest.mark.parametrize("n", SIZES)
def test_key_hash_batch(gpu_lib, n):
    x = np.random.default_rng(n).integers(0, 256, (n, 64), dtype=np.uint8)
    got = P.byron_key_hash(x)
    assert [r.tobytes() for r in got] == [P.key_hash(r.tobytes()) for r in x]
    np.testing.assert_array_equal(got, P.byron_key_hash(x, host=True))


def test_key_hash_one_row_past_the_grid_cap(gpu_lib):
    """The launch caps its grid and strides over the rest: one row more than
    the capped grid has lanes.  4,099 distinct keys (a prime, so a lane's two
    rows differ) hashed once by hashlib and tiled."""
    n = GRID_CAP_ROWS + 1
    base = np.random.default_rng(7).integers(0, 256, (4099, 64), dtype=np.uint8)
    ids = np.frombuffer(b"".join(P.key_hash(r.tobytes()) for r in base), np.uint8).reshape(-1, 28)
    reps = n // 4099 + 1
    x = np.ascontiguousarray(np.tile(base, (reps, 1))[:n])
    got = P.byron_key_hash(x)
    np.testing.assert_array_equal(got, np.tile(ids, (reps, 1))[:n])


def test_long_schedule(gpu_lib):
    """k = 4,096 entries of 7 rows: the entry search at its cap, each entry
    its own delegates (entry j knows keys j .. j + 6 of a pool of 4,102)."""
    k = 4096
    kk, ids = PC.keys(k + 6, seed=2)
    entries = [(10 * j, [(ids[j + i], PC.gen_id(i)) for i in range(7)]) for j in range(k)]
    v = P.PBftViews(entries, 20, 4)
    rng = np.random.default_rng(4)
    n = 1500
    slot = np.sort(rng.integers(0, 10 * k + 50, n)).astype(np.uint64)
    slot[:3] = (0, 9, 10)
    slot[-1] = (1 << 63) + 5
    slot = np.sort(slot)
    who = (slot // np.uint64(10)).clip(0, k - 1).astype(np.int64) + rng.integers(-2, 9, n)
    vk = np.ascontiguousarray(kk[who.clip(0, k + 5)])
    status = np.zeros(n, np.uint8)
    keys = [r.tobytes() for r in vk]
    want = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), P.PBftState())
    got = P.pbft_checks(vk, slot, status, v, state=P.PBftState())
    for q in range(3):
        np.testing.assert_array_equal(got[q], want[q])
    assert got[3] == want[3]
    known = (want[0] & P.PBFT_DELEGATE_KNOWN) != 0
    assert known.sum() >= 300 and (~known).sum() >= 300


def test_device_pointer_form(gpu_lib):
    import torch

    v = PC.schedule(3, 3, 10, 3)
    n = 700
    vk, slot, status = _wave_rows(n)
    lb, lr, _, _ = P.pbft_rule(v, [r.tobytes() for r in vk], slot.tolist(), status.tolist())
    dev = torch.device("cuda", 0)
    d_vk = torch.tensor(vk, device=dev)
    d_slot = torch.tensor(slot.view(np.int64), device=dev)
    d_status = torch.tensor(status, device=dev)
    bits = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    rows = torch.full((n,), 5, dtype=torch.int32, device=dev)
    cv = v.c_struct()
    h = ctypes.c_void_p()
    _native.check(gpu_lib.ouro_pbft_views_upload(ctypes.byref(cv), ctypes.byref(h)),
                  "ouro_pbft_views_upload")
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            args = [ctypes.c_void_p(side.cuda_stream), n, d_vk.data_ptr(), d_slot.data_ptr(),
                    d_status.data_ptr(), h, bits.data_ptr(), rows.data_ptr()]
            _native.check(gpu_lib.ouro_pbft_ledger_checks_device(*args),
                          "ouro_pbft_ledger_checks_device")
            ids = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
            _native.check(gpu_lib.ouro_byron_key_hash_batch_device(
                ctypes.c_void_p(side.cuda_stream), n, d_vk.data_ptr(), ids.data_ptr()),
                "ouro_byron_key_hash_batch_device")
        side.synchronize()
        np.testing.assert_array_equal(bits.cpu().numpy(), lb)
        np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint32), lr)
        np.testing.assert_array_equal(ids.cpu().numpy(), P.byron_key_hash(vk, host=True))
        # refused before anything is enqueued
        for at, val in ((2, d_vk.data_ptr() + 1), (3, d_slot.data_ptr() + 4), (5, None),
                        (7, None), (7, rows.data_ptr() + 2)):
            bad = list(args)
            bad[at] = val
            assert gpu_lib.ouro_pbft_ledger_checks_device(*bad) == _native.OURO_EINVAL
        assert gpu_lib.ouro_byron_key_hash_batch_device(None, n, d_vk.data_ptr() + 2,
                                                        ids.data_ptr()) == _native.OURO_EINVAL
    finally:
        gpu_lib.ouro_pbft_views_free(h)
    bad = P.PBftViews([(3, [])], 5, 2).c_struct()
    assert gpu_lib.ouro_pbft_views_upload(ctypes.byref(bad), ctypes.byref(h)) == \
        _native.OURO_EINVAL


@pytest.mark.device_error
def test_device_error_recomputes_on_the_host_path(gpu_lib):
    v = PC.schedule(3, 3, 10, 3)
    vk, slot, status = _wave_rows(300)
    keys = [r.tobytes() for r in vk]
    want = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), P.PBftState())
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1"):
        got = P.pbft_checks(vk, slot, status, v, state=P.PBftState())
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
        ids = P.byron_key_hash(vk)
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
    for q in range(3):
        np.testing.assert_array_equal(got[q], want[q])
    assert got[3] == want[3]
    assert [r.tobytes() for r in ids] == [P.key_hash(k) for k in keys]
    assert (want[1] != LV_NO_POOL).any()


# ---- the chain entry in 256-header chunks -----------------------------------------

def _chain(raws, pv, state, **kw):
    lv, g, spkp = PC.trivial_ledger()
    return P.validate_chain_pbft_cbor(raws, spkp, -1, lv, g, pv, state=state, cfg=PC.chain_cfg(),
                                      **kw)


def _same_base(a, b):
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3] and a[4] == b[4]
    assert a[5].tobytes() == b[5].tobytes() and a[6].tobytes() == b[6].tobytes()


def _check_chain3(got, want):
    for q in range(3):
        np.testing.assert_array_equal(got[8 + q], want[q])
    assert got[11] == want[3]
    assert (got[0][2] == 1).all()                       # every signature verifies, EBBs pass
    bits = want[0]
    # EBBs at the first row of the second and the third chunk
    assert (bits[[256, 512]] == (P.PBFT_BOUNDARY | P.PBFT_ALL_OK)).all()
    # the window (300) fills and starts trimming inside the second chunk
    assert len(want[3].signers) == 300
    # the breach: none in the first chunk, the first one in the second chunk,
    # before the window trims, so its count holds signatures of both chunks
    known = (bits & P.PBFT_DELEGATE_KNOWN) != 0
    over = np.nonzero(known & ((bits & P.PBFT_WINDOW_OK) == 0) & ((bits & P.PBFT_BOUNDARY) == 0))[0]
    assert len(over) > 20 and 256 < over[0] < 300 and want[2][over[0]] == 121
    assert bits[700] == 0 and got[0][2][700] == 1       # the undelegated signer: verdict 1, unknown


@pytest.mark.parametrize("slots", [1, 3])
def test_chain_entry_pure_byron_three_chunks(gpu_lib, small_chunks, slots):
    from ouroboros_network_amd import header as H

    raws = list(PC.chain3())
    pv = PC.chain_views(300, 120)
    want = PC.expect_pbft(raws, pv, PC.chain_cfg(), P.PBftState())
    small_chunks(CHUNK=256, SLOTS=slots)
    got = _chain(raws, pv, P.PBftState())
    _check_chain3(got, want)
    lv, g, spkp = PC.trivial_ledger()
    ref = H.validate_chain_ledger_cbor(raws, spkp, -1, lv, g, cfg=PC.chain_cfg())
    _same_base(ref, got)
    host = _chain(raws, pv, P.PBftState(), host=True)
    _same_base(host, got)
    for q in range(8, 11):
        np.testing.assert_array_equal(host[q], got[q])
    assert host[11] == got[11]


def test_chain_entry_mixed_chunk_with_every_schedule(gpu_lib, small_chunks):
    """Byron then Shelley in chunk 0, under ledger views, a genesis-delegation
    schedule and the golden delegation map together; everything but the PBFT
    outputs byte-identical to the overlay entry, and a NULL schedule too"""
    import envelope_cases as EC
    import ledger_cases as LC
    import overlay_cases as OC
    from ouroboros_network_amd import header as H
    from ouroboros_network_amd import ledger as L

    s = OC.chain_stream()
    nb = s["n_byron"]
    assert 0 < nb < 256 < len(s["raws"])
    pv = PC.golden_views(5, 2)
    st0 = P.PBftState([(0, bytes.fromhex(PC.golden()["header"]["genesis_id"]))])
    want = PC.expect_pbft(s["raws"], pv, EC.VAL_CFG, st0)
    assert (want[0][:nb] & P.PBFT_DELEGATE_KNOWN).any() and (want[0][:nb] & P.PBFT_BOUNDARY).any()
    assert not want[0][nb:].any()
    kw = dict(genesis=s["genesis"], cfg=EC.VAL_CFG, epochs=s["epochs"], nonce=True)
    call = lambda **k: H.validate_chain_ledger_cbor(  # noqa: E731
        s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
        counters=L.Counters(s["table_ids"], s["known"]), **kw, **k)
    small_chunks(CHUNK=256, SLOTS=3)
    ref = call()
    got = call(pbft=pv, pbft_state=st0)
    _same_base(ref, got)
    assert ref[7].as_dict() == got[7].as_dict()
    for q in range(3):
        np.testing.assert_array_equal(got[8 + q], want[q])
    assert got[11] == want[3]
    null = call(pbft=False)
    _same_base(ref, null)
    assert ref[7].as_dict() == null[7].as_dict()


@pytest.mark.device_error
def test_chain_device_error_restarts_the_fold(gpu_lib):
    raws = list(PC.chain3())
    pv = PC.chain_views(300, 120)
    st0 = P.PBftState([(0, PC.gen_id(1))] * 2)
    want = PC.expect_pbft(raws, pv, PC.chain_cfg(), st0)
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1", OURO_CBOR_CHUNK="256"):
        got = _chain(raws, pv, st0)
        assert "recomputed on the host path" in gpu_lib.ouro_last_error().decode()
    for q in range(3):
        np.testing.assert_array_equal(got[8 + q], want[q])
    assert got[11] == want[3]
