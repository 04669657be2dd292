"""Byron transaction witnesses on the device: all three device-side entries,
byte-identical to the rule of byron_witness.py and the oracle
(tests/byron_witness_cases.py) -- the whole case set, the magics, every flip and
truncation of the golden block, block counts across the scan's tile, a witness
wave that mixes blocks, one wave with every outcome, capacities exact and one
row short, the host-buffer form cut into groups, the count entry, and the
recompute after a device error."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import byron_block_cases as C
import byron_witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as BY
from ouroboros_network_amd import byron_witness as BW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE = 1024     # csrc/scan_excl.h kScanTile: one workgroup's tile of the scan
M = WC.GOLDEN_MAGIC


@pytest.fixture(scope="module")
def cs():
    return WC.case_set()


def test_one_call_entry_on_the_case_set(gpu_lib, cs):
    r = BW.verify_byron_block_witnesses(cs["triple"], M)
    WC.check_result(r, cs)
    assert not ((r.verdict != 0) & ~np.isin(r.status, (BW.PACK_OK, BW.PACK_EBB))).any()
    status, ntx, nwit = BW.count_byron_block_witnesses(cs["triple"], M)       # the device count entry
    for got, f in ((status, "status"), (ntx, "ntx"), (nwit, "nwit")):
        np.testing.assert_array_equal(got, cs[f], f)


def test_every_magic_and_each_headers_own(gpu_lib):
    raws = WC.magic_set()
    for magic in [BY.HEADER_MAGIC] + WC.MAGICS:
        want = WC.expected_arrays(raws, magic)
        WC.check_result(BW.verify_byron_block_witnesses(raws, magic), want)
        assert want["verdict"].any() and not want["verdict"].all()


def test_every_flip_and_truncation_of_the_golden_block(gpu_lib):
    for raws in (C.golden_flips(), C.golden_truncations()):
        WC.check_result(BW.verify_byron_block_witnesses(raws, M), WC.expected_arrays(raws, M))


@pytest.mark.parametrize("n", [1, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE])
def test_block_counts_across_the_scan_tile(gpu_lib, n):
    pool = WC.pool()
    raws = [pool[(7 * i + i // 9) % len(pool)] for i in range(n)]
    want = WC.expected_arrays(raws, M)
    WC.check_result(BW.verify_byron_block_witnesses(raws, M), want)
    assert n < 16 or ((want["n_bad"] > 0).any() and (want["status"] == BW.PACK_EBB).any())


def test_one_block_of_65_witnesses_among_empty_blocks(gpu_lib):
    """A witness wave then mixes blocks, and valid and invalid rows."""
    rng = np.random.default_rng(711)
    pool = WC.pool()
    tx = C.sized_array(77, rng)
    wits = [WC.enc_wit(k, *WC.sign(k, 100 + q, tx, M)) for q, k in enumerate(WC.kinds_of("alt", 65))]
    big = C.make_block([(tx, WC.vector(wits))], magic=M)
    p = BW.parse_byron_witnesses(big)
    r = bytearray(big)
    for q in (0, 31, 63, 64):
        r[big.index(p.witnesses[q].sig) + 3] ^= 0x80
    raws = [pool[0], pool[3], pool[0], bytes(r), pool[1], pool[5], pool[0]]
    want = WC.expected_arrays(raws, M)
    assert want["n_bad"].tolist() == [0, 0, 0, 4, 0, 0, 0]
    WC.check_result(BW.verify_byron_block_witnesses(raws, M), want)


def _device_call(gpu_lib, triple, magic, tx_cap, wit_cap, extra_span=False):
    """ouro_byron_block_witness_verify_cbor_device over the blocks of `triple`
    in device memory, as they lie in its buffer; the outputs as numpy arrays"""
    import torch

    buf, off, ln = triple
    buf = bytes(buf.tobytes())
    off, ln = [int(x) for x in off], [int(x) for x in ln]
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
             wit_vk=t8((max(wit_cap, 1), 64), 9), status=t8((n,), 9), verdict=t8((n,), 7),
             n_bad=torch.full((n,), 9, dtype=torch.int32, device=dev))
    out = BW.ByronWitnessOutC(tx_cap, wit_cap, *(o[f].data_ptr() for f in (
        "tx_begin", "wit_begin", "tx_id", "wit_tx", "wit_kind", "wit_ok", "wit_vk")))
    wb = int(gpu_lib.ouro_byron_block_witness_work_bytes(n, tx_cap, wit_cap))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    args = [ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), len(buf), d_off.data_ptr(),
            d_len.data_ptr(), n, magic, ctypes.byref(out), work.data_ptr(), wb,
            o["status"].data_ptr(), o["verdict"].data_ptr(), o["n_bad"].data_ptr()]
    _native.check(gpu_lib.ouro_byron_block_witness_verify_cbor_device(*args),
                  "ouro_byron_block_witness_verify_cbor_device")
    torch.cuda.synchronize()
    res = {f: v.cpu().numpy() for f, v in o.items()}
    for f in ("tx_begin", "wit_begin"):
        res[f] = res[f].astype(np.uint64)
    for f in ("wit_tx", "n_bad"):
        res[f] = res[f].astype(np.uint32)
    return res


class _R:
    def __init__(self, d):
        self.__dict__.update(d)


def _check_device(res, want, n):
    got = {f: (v[:n + 1] if f in ("tx_begin", "wit_begin") else v[:n] if f in (
        "status", "verdict", "n_bad") else v) for f, v in res.items()}
    WC.check_result(_R(got), want)


def test_device_resident_form_exact_capacities(gpu_lib, cs):
    """The case set's own buffer: every tx length at every alignment.  A span
    outside the buffer is OURO_PACK_ESPAN for that block alone."""
    T, Wn = int(cs["tx_begin"][-1]), int(cs["wit_begin"][-1])
    res = _device_call(gpu_lib, cs["triple"], M, T, Wn, extra_span=True)
    n = len(cs["raws"])
    assert res["status"][n] == BW.PACK_ESPAN and res["verdict"][n] == 0 and res["n_bad"][n] == 0
    assert res["tx_begin"][n + 1] == T and res["wit_begin"][n + 1] == Wn
    _check_device(res, cs, n)


def test_device_resident_form_each_headers_own_magic(gpu_lib):
    raws = WC.magic_set()
    want = WC.expected_arrays(raws, "header")
    res = _device_call(gpu_lib, C.layout(raws), -1, int(want["tx_begin"][-1]),
                       int(want["wit_begin"][-1]))
    _check_device(res, want, len(raws))


@pytest.mark.parametrize("short", ["tx", "wit"])
def test_device_resident_form_one_row_short(gpu_lib, short):
    """The last block gets ECAP and writes nothing (its rows are zero), the
    blocks before it are untouched, the totals are still right."""
    pool = WC.pool()
    raws = [pool[3], pool[0], pool[7], pool[8], pool[4], pool[5]]
    full = WC.expected_arrays(raws, M)
    tc = int(full["tx_begin"][-1]) - (short == "tx")
    wc = int(full["wit_begin"][-1]) - (short == "wit")
    want = WC.expected_arrays(raws, M, tc, wc)
    assert want["status"].tolist() == full["status"].tolist()[:-1] + [BW.PACK_ECAP]
    _check_device(_device_call(gpu_lib, C.layout(raws), M, tc, wc), want, len(raws))


def test_one_wave_mixing_every_outcome(gpu_lib, cs):
    """64 blocks in one wave of the count, emit and finish kernels: OK, EBB,
    ESHELLEY, ECBOR, ESHAPE, ESIZE, and ECAP for the blocks past the
    capacities."""
    pool = WC.pool()
    by = {k: cs["raws"][cs["kinds"].index(k)] for k in ("content_short", "type_1", "key_63",
                                                        "sig_bit")}
    cyc = [pool[5], pool[7], C.golden()["cardano_disk_Mary"], by["content_short"], pool[8],
           by["type_1"], by["key_63"], by["sig_bit"], pool[0]]
    raws = [cyc[i % len(cyc)] for i in range(64)]
    full = WC.expected_arrays(raws, M)
    tc, wc = int(full["tx_begin"][50]), int(full["wit_begin"][-1])
    want = WC.expected_arrays(raws, M, tc, wc)
    assert {int(s) for s in want["status"]} == {BW.PACK_OK, BW.PACK_EBB, BW.PACK_ESHELLEY,
                                                BW.PACK_ECBOR, BW.PACK_ESHAPE, BW.PACK_ESIZE,
                                                BW.PACK_ECAP}
    assert (want["status"] == BW.PACK_ECAP).sum() >= 5 and (want["n_bad"] > 0).sum() >= 8
    _check_device(_device_call(gpu_lib, C.layout(raws), M, tc, wc), want, 64)


def test_host_buffer_form_in_three_groups(gpu_lib):
    """The byte budget forced small (OURO_BYRON_WITNESS_GROUP_BYTES): the batch
    spans three groups, the begins of the later groups continue the earlier
    ones, and witnesses land on both sides of each cut."""
    pool = WC.pool()
    raws = [pool[5], pool[3], pool[8], pool[6], pool[7], pool[5], pool[4], pool[3], pool[1]]
    third = sum(len(r) for r in raws[:3])
    cuts, lo = [], 0
    while lo < len(raws):                   # the library's grouping: whole blocks under the budget
        hi, used = lo, 0
        while hi < len(raws) and (hi == lo or used + len(raws[hi]) <= third):
            used += len(raws[hi])
            hi += 1
        cuts.append(hi)
        lo = hi
    assert cuts == [3, 7, 9]                # (the EBB is small: the middle group holds four)
    want = WC.expected_arrays(raws, M)
    nw = np.diff(want["wit_begin"])
    assert nw[[2, 3, 6, 7]].all()           # witnesses on both sides of each cut
    with _native.knob_env(OURO_BYRON_WITNESS_GROUP_BYTES=str(third)):
        WC.check_result(BW.verify_byron_block_witnesses(raws, M), want)
        T, Wn = int(want["tx_begin"][-1]), int(want["wit_begin"][-1])
        short = BW.verify_byron_block_witnesses(raws, M, tx_cap=T, wit_cap=Wn - 1)
        status, ntx, nwit = BW.count_byron_block_witnesses(raws, M)
    # (the last block has no witness, but its rows begin past the capacity)
    WC.check_result(short, WC.expected_arrays(raws, M, T, Wn - 1))
    assert short.status[-2:].tolist() == [BW.PACK_ECAP] * 2 and short.status[-3] == BW.PACK_OK
    np.testing.assert_array_equal(status, want["status"])
    np.testing.assert_array_equal(nwit, want["nwit"])


CHILD = r"""
import ctypes, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch
torch.cuda.init()
import byron_witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron_witness as BW
lib = _native.load()
assert _native.test_hooks()
p = WC.pool()
raws = [p[5], p[7], p[8], p[3], p[0], WC.broken()[-1][1]]
a, b0, b1 = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b0))
r = BW.verify_byron_block_witnesses(raws, WC.GOLDEN_MAGIC)   # the count call, then the verify call
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b1))
assert b1.value - b0.value == 2, (b0.value, b1.value)
assert b"recomputed on the host path" in lib.ouro_last_error()
WC.check_result(r, WC.expected_arrays(raws, WC.GOLDEN_MAGIC))
os.environ["OURO_ON_DEVICE_ERROR"] = "fail"
lib.ouro_debug_reload_knobs()
try:
    BW.verify_byron_block_witnesses(raws, WC.GOLDEN_MAGIC, tx_cap=100, wit_cap=400)
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
