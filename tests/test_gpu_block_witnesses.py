"""Transaction witnesses on the device: the one-call entries on the case set,
block counts across every boundary of the scan, a witness wave that mixes
blocks, the device-resident form with exact and short capacities, the count
entry, the host-buffer form cut into groups, and the recompute after a device
error -- against the expectations of tests/witness_cases.py
(witness.parse_witnesses, hashlib, the oracle) and the host path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import block as B
from ouroboros_network_amd import witness as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE = 1024     # csrc/scan_excl.h kScanTile: one workgroup's tile of the scan


@pytest.fixture(scope="module")
def cs():
    return WC.case_set()


@pytest.fixture(scope="module")
def pool():
    """Blocks of 0 to 2 transactions with 0 to 2 witnesses each, one of them
    with a bad signature"""
    rng = np.random.default_rng(51)
    out = []
    for k, counts in enumerate([(), (0,), (1,), (2,), (1, 0), (2, 1), (0, 2)]):
        bodies = [WC.tx_body(20 + 5 * k + t, rng) for t in range(len(counts))]
        sets = [WC.cmap([(WC.uint(0), WC.arr(WC.vkey_wit(600 + 10 * k + 3 * t + q, WC.b2b(b))
                                             for q in range(c)))])
                for t, (b, c) in enumerate(zip(bodies, counts))]
        out.append(WC.make_block(bodies, sets, form=k % 4))
    bad = bytearray(out[5])
    sig = W.parse_witnesses(out[5]).witnesses[1].sig
    bad[out[5].index(sig) + 40] ^= 0x02
    out.append(bytes(bad))
    return out


def same_result(a, b, T, Wn):
    for f in ("status", "verdict", "n_bad", "tx_begin", "wit_begin"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), f)
    np.testing.assert_array_equal(a.tx_id[:T], b.tx_id[:T])
    for f in ("wit_tx", "wit_kind", "wit_ok", "wit_vk"):
        np.testing.assert_array_equal(getattr(a, f)[:Wn], getattr(b, f)[:Wn], f)


def test_one_call_entry_on_the_case_set(gpu_lib, cs):
    r = W.verify_block_witnesses(cs["triple"])
    WC.check_result(r, cs)
    h = W.verify_block_witnesses(cs["triple"], host=True)
    same_result(r, h, int(cs["tx_begin"][-1]), int(cs["wit_begin"][-1]))
    assert not ((r.verdict != 0) & (r.status != B.PACK_OK)).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 7,
                               2 * SCAN_TILE])
def test_block_counts_across_the_scan_boundaries(gpu_lib, pool, n):
    raws = [pool[(5 * i + i // 7) % len(pool)] for i in range(n)]
    want = WC.expected_arrays(raws)
    WC.check_result(W.verify_block_witnesses(raws), want)
    assert n < 8 or (want["n_bad"] > 0).any()


def test_one_block_of_65_witnesses_among_empty_blocks(gpu_lib, pool):
    """A witness wave then mixes blocks, and valid and invalid rows."""
    rng = np.random.default_rng(52)
    body = WC.tx_body(77, rng)
    wits = [WC.vkey_wit(700 + q, WC.b2b(body)) for q in range(65)]
    big = WC.make_block([body], [WC.cmap([(WC.uint(0), WC.arr(wits))])])
    p = W.parse_witnesses(big)
    r = bytearray(big)
    for q in (0, 31, 63, 64):
        r[big.index(p.witnesses[q].sig) + 3] ^= 0x80
    raws = [pool[0], pool[3], pool[0], bytes(r), pool[1], pool[5], pool[0]]
    want = WC.expected_arrays(raws)
    assert want["n_bad"].tolist() == [0, 0, 0, 4, 0, 0, 0]
    WC.check_result(W.verify_block_witnesses(raws), want)


def _device_call(gpu_lib, raws, tx_cap, wit_cap, extra_span=False):
    """ouro_block_witness_verify_cbor_device over blocks in device memory,
    spans padded apart; returns the outputs as numpy arrays"""
    import torch

    parts, off, ln, at = [], [], [], 0
    for k, r in enumerate(raws):
        pad = bytes(k % 7)
        parts += [pad, r]
        off.append(at + len(pad))
        ln.append(len(r))
        at += len(pad) + len(r)
    buf = b"".join(parts)
    if extra_span:
        off.append(len(buf) - 3)
        ln.append(10)
    n = len(off)
    dev = torch.device("cuda", 0)
    t8 = lambda shape, fill: torch.full(shape, fill, dtype=torch.uint8, device=dev)  # noqa: E731
    d_raw = torch.tensor(np.frombuffer(buf + bytes(-len(buf) % 4), np.uint8).copy(), device=dev)
    d_off = torch.tensor(np.array(off, np.int64), device=dev)
    d_len = torch.tensor(np.array(ln, np.int32), device=dev)
    o = dict(tx_begin=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
             wit_begin=torch.full((n + 1,), -1, dtype=torch.int64, device=dev),
             tx_id=t8((max(tx_cap, 1), 32), 5),
             wit_tx=torch.full((max(wit_cap, 1),), 9, dtype=torch.int32, device=dev),
             wit_kind=t8((max(wit_cap, 1),), 9), wit_ok=t8((max(wit_cap, 1),), 9),
             wit_vk=t8((max(wit_cap, 1), 32), 9), status=t8((n,), 9), verdict=t8((n,), 7),
             n_bad=torch.full((n,), 9, dtype=torch.int32, device=dev))
    out = W.WitnessOutC(tx_cap, wit_cap, *(o[f].data_ptr() for f in (
        "tx_begin", "wit_begin", "tx_id", "wit_tx", "wit_kind", "wit_ok", "wit_vk")))
    wb = int(gpu_lib.ouro_block_witness_work_bytes(n, tx_cap, wit_cap))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    args = [ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), len(buf), d_off.data_ptr(),
            d_len.data_ptr(), n, ctypes.byref(out), work.data_ptr(), wb, o["status"].data_ptr(),
            o["verdict"].data_ptr(), o["n_bad"].data_ptr()]
    _native.check(gpu_lib.ouro_block_witness_verify_cbor_device(*args),
                  "ouro_block_witness_verify_cbor_device")
    torch.cuda.synchronize()
    res = {f: v.cpu().numpy() for f, v in o.items()}
    for f in ("tx_begin", "wit_begin"):
        res[f] = res[f].astype(np.uint64)
    for f in ("wit_tx", "n_bad"):
        res[f] = res[f].astype(np.uint32)
    # a short work area, a misaligned buffer: errors, nothing launched
    short = list(args)
    short[8] = wb - 1
    assert gpu_lib.ouro_block_witness_verify_cbor_device(*short) == _native.OURO_EINVAL
    odd = list(args)
    odd[1] = d_raw.data_ptr() + 1
    assert gpu_lib.ouro_block_witness_verify_cbor_device(*odd) == _native.OURO_EINVAL
    return res


class _R:
    def __init__(self, d):
        self.__dict__.update(d)


def test_device_resident_form_exact_capacities(gpu_lib, cs):
    raws = cs["raws"]
    T, Wn = int(cs["tx_begin"][-1]), int(cs["wit_begin"][-1])
    res = _device_call(gpu_lib, raws, T, Wn, extra_span=True)
    n = len(raws)
    assert res["status"][n] == B.PACK_ESPAN and res["verdict"][n] == 0 and res["n_bad"][n] == 0
    assert res["tx_begin"][n + 1] == T and res["wit_begin"][n + 1] == Wn
    got = {f: (v[:n + 1] if f in ("tx_begin", "wit_begin") else v[:n] if f in (
        "status", "verdict", "n_bad") else v) for f, v in res.items()}
    WC.check_result(_R(got), cs)


@pytest.mark.parametrize("short", ["tx", "wit"])
def test_device_resident_form_one_row_short(gpu_lib, pool, short):
    """The last block gets ECAP and writes nothing (its rows stay zero), the
    blocks before it are untouched, the totals are still right."""
    raws = [pool[3], pool[0], pool[7], pool[4], pool[5]]
    want = WC.expected_arrays(raws)
    T, Wn = int(want["tx_begin"][-1]), int(want["wit_begin"][-1])
    tc, wc = T - (short == "tx"), Wn - (short == "wit")
    res = _device_call(gpu_lib, raws, tc, wc)
    np.testing.assert_array_equal(res["tx_begin"], want["tx_begin"])
    np.testing.assert_array_equal(res["wit_begin"], want["wit_begin"])
    assert res["status"][-1] == W.PACK_ECAP and res["verdict"][-1] == 0 and res["n_bad"][-1] == 0
    for f in ("status", "verdict", "n_bad"):
        np.testing.assert_array_equal(res[f][:-1], want[f][:-1], f)
    t0, w0 = int(want["tx_begin"][-2]), int(want["wit_begin"][-2])
    np.testing.assert_array_equal(res["tx_id"][:t0], want["tx_id"][:t0])
    assert not res["tx_id"][t0:tc].any()
    for f in ("wit_tx", "wit_kind", "wit_vk", "wit_ok"):
        np.testing.assert_array_equal(res[f][:w0], want[f][:w0], f)
        assert not res[f][w0:wc].any(), f


def test_device_count_entry(gpu_lib, cs):
    status, ntx, nwit = W.count_block_witnesses(cs["triple"])
    np.testing.assert_array_equal(status, cs["status"])
    np.testing.assert_array_equal(ntx, np.diff(cs["tx_begin"]))
    np.testing.assert_array_equal(nwit, np.diff(cs["wit_begin"]))


def test_host_buffer_form_in_three_groups(gpu_lib, pool):
    """The byte budget forced small (OURO_WITNESS_GROUP_BYTES): the batch
    spans three groups, the begins of the later groups continue the earlier
    ones, and a transaction's witnesses land next to a group boundary."""
    raws = [pool[5], pool[3], pool[7], pool[6], pool[0], pool[5], pool[4], pool[3], pool[1]]
    third = sum(len(r) for r in raws[:3])
    cuts, lo = [], 0
    while lo < len(raws):                   # the library's grouping: whole blocks under the budget
        hi, used = lo, 0
        while hi < len(raws) and (hi == lo or used + len(raws[hi]) <= third):
            used += len(raws[hi])
            hi += 1
        cuts.append(hi)
        lo = hi
    assert cuts == [3, 6, 9]
    want = WC.expected_arrays(raws)
    assert np.diff(want["wit_begin"])[[2, 3, 5, 6]].all()     # witnesses on both sides of each cut
    with _native.knob_env(OURO_WITNESS_GROUP_BYTES=str(third)):
        r = W.verify_block_witnesses(raws)
        WC.check_result(r, want)
        T, Wn = int(want["tx_begin"][-1]), int(want["wit_begin"][-1])
        short = W.verify_block_witnesses(raws, tx_cap=T, wit_cap=Wn - 1)
    # (the last block has no witness, but its rows begin past the capacity)
    assert short.status[-2:].tolist() == [W.PACK_ECAP] * 2 and short.status[-3] == B.PACK_OK
    np.testing.assert_array_equal(short.wit_begin, want["wit_begin"])
    w0 = int(want["wit_begin"][-3])
    np.testing.assert_array_equal(short.wit_ok[:w0], want["wit_ok"][:w0])


CHILD = r"""
import ctypes, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch
torch.cuda.init()
import witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import witness as W
lib = _native.load()
assert _native.test_hooks()
raws = [r for r, _ in WC.valid()[-5:]] + [r for r, _ in WC.invalid()[:3]] + [WC.malformed()[0][0]]
a, b0, b1 = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b0))
r = W.verify_block_witnesses(raws)          # the count call, then the verify call
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b1))
assert b1.value - b0.value == 2, (b0.value, b1.value)
assert b"recomputed on the host path" in lib.ouro_last_error()
WC.check_result(r, WC.expected_arrays(raws))
os.environ["OURO_ON_DEVICE_ERROR"] = "fail"
lib.ouro_debug_reload_knobs()
try:
    W.verify_block_witnesses(raws, tx_cap=100, wit_cap=400)
except _native.DeviceError:
    print("ok")
"""


def test_device_error_recomputes_on_the_host_path(gpu_lib):
    """A fresh child process on the test build with OURO_TEST_DEVICE_ERROR
    set: every launch reports a device error, both entries recompute on the
    host path and still give the rule's results; OURO_ON_DEVICE_ERROR=fail
    returns the error instead."""
    assert os.path.exists(_native.TEST_LIB_PATH), "build lib/libouro_verify_test.so (make)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("OURO_")}
    env["OURO_VERIFY_LIB"] = _native.TEST_LIB_PATH
    env["OURO_TEST_DEVICE_ERROR"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
