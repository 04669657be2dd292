"""Byron whole-block integrity on the device: the one-call entry and the count
entry on the case set and on every flip of the golden block, block counts
across every boundary of the scan, one wave that mixes every outcome, the
device-resident form with exact and short capacities, the host-buffer form cut
into groups, and the recompute after a device error -- against the
expectations of tests/byron_block_cases.py (byron_block.byron_block_rule,
hashlib, the oracle's ByronDSIGN verify) and the host path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import byron_block_cases as C
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron_block as BB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE = 1024     # csrc/scan_excl.h kScanTile: one workgroup's tile of the scan


@pytest.fixture(scope="module")
def cs():
    return C.case_set()


@pytest.fixture(scope="module")
def pool(cs):
    """the small blocks of the case set, every outcome among them"""
    return [r for k, r in zip(cs["kinds"], cs["raws"]) if len(r) < 2500] + \
        [C.golden()["cardano_n2n_Byron_regular"][:200]]


def check(got, want):
    v, st, root = got
    np.testing.assert_array_equal(st, want["status"])
    np.testing.assert_array_equal(v, want["verdict"])
    np.testing.assert_array_equal(root, want["tx_root"])


def test_one_call_entry_on_the_case_set(gpu_lib, cs):
    got = BB.verify_byron_block_integrity(cs["triple"], cs["magic"])
    check(got, cs)
    host = BB.verify_byron_block_integrity(cs["triple"], cs["magic"], host=True)
    for a, b in zip(got, host):
        np.testing.assert_array_equal(a, b)
    for kind, v in zip(cs["kinds"], got[0]):
        if kind in C.BROKEN:
            assert v == C.must_be(kind), kind


def test_count_entry_on_the_case_set(gpu_lib, cs):
    st, ntx, gather, msg, totals = BB.count_byron_blocks(cs["triple"], cs["magic"])
    np.testing.assert_array_equal(st, cs["status"])
    np.testing.assert_array_equal(ntx, cs["ntx"])
    np.testing.assert_array_equal(gather, cs["gather"])
    np.testing.assert_array_equal(msg, cs["msg"])
    assert totals.tolist() == [int(cs[f].sum()) for f in ("ntx", "gather", "msg")]


def test_every_flip_of_the_golden_block(gpu_lib):
    raws = C.golden_flips()
    magic = C.parts()["magic_value"]
    got = BB.verify_byron_block_integrity(raws, magic)
    check(got, C.expected_arrays(raws, magic))
    for a, b in zip(got, BB.verify_byron_block_integrity(raws, magic, host=True)):
        np.testing.assert_array_equal(a, b)


def test_each_headers_own_magic(gpu_lib, cs):
    raws = [r for k, r in zip(cs["kinds"], cs["raws"])
            if k in ("magic_field", "magic_signed", "golden_byron", "sig", "span")]
    check(BB.verify_byron_block_integrity(raws, "header"), C.expected_arrays(raws, "header"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_block_counts_across_the_scan_boundaries(gpu_lib, cs, pool, n):
    exp = {r: C.expect(r, cs["magic"]) for r in pool}
    raws = [pool[(5 * i + i // 7) % len(pool)] for i in range(n)]
    v, st, root = BB.verify_byron_block_integrity(raws, cs["magic"])
    assert st.tolist() == [exp[r][0] for r in raws]
    assert v.tolist() == [exp[r][1] for r in raws]
    assert root.tobytes() == b"".join(exp[r][2] for r in raws)


def _device_call(gpu_lib, raws, magic, caps, extra_span=False, triple=None):
    """ouro_byron_block_integrity_verify_cbor_device over blocks in device
    memory, spans padded apart (or laid out as `triple` has them); returns
    verdict, status and tx_root"""
    import torch

    if triple is not None:
        buf, off, ln = triple[0].tobytes(), [int(o) for o in triple[1]], [int(x) for x in triple[2]]
    else:
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
    d_raw = torch.tensor(np.frombuffer(buf + bytes(-len(buf) % 4), np.uint8).copy(), device=dev)
    d_off = torch.tensor(np.array(off, np.int64), device=dev)
    d_len = torch.tensor(np.array(ln, np.int32), device=dev)
    status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    verdict = torch.full((n,), 0x55, dtype=torch.uint8, device=dev)
    root = torch.full((n, 32), 5, dtype=torch.uint8, device=dev)
    wb = int(gpu_lib.ouro_byron_block_work_bytes(n, *caps))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    args = [ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), len(buf), d_off.data_ptr(),
            d_len.data_ptr(), n, magic, *caps, work.data_ptr(), wb, status.data_ptr(),
            verdict.data_ptr(), root.data_ptr()]
    _native.check(gpu_lib.ouro_byron_block_integrity_verify_cbor_device(*args),
                  "ouro_byron_block_integrity_verify_cbor_device")
    torch.cuda.synchronize()
    return verdict.cpu().numpy(), status.cpu().numpy(), root.cpu().numpy()


def _with_caps(raws, magic, caps):
    """the rule under capacities: the regular blocks whose rows end inside all
    three keep their results, the others are PACK_ECAP with nothing written"""
    want = C.expected_arrays(raws, magic)
    t = g = m = 0
    for i in range(len(raws)):
        if want["status"][i] == BB.PACK_OK:
            a, b, c = int(want["ntx"][i]), int(want["gather"][i]), int(want["msg"][i])
            if t + a > caps[0] or g + b > caps[1] or m + c > caps[2]:
                want["status"][i] = BB.PACK_ECAP
                want["verdict"][i] = 0
                want["tx_root"][i] = 0
            t, g, m = t + a, g + b, m + c
    return want, (t, g, m)


def test_device_resident_form_on_the_case_set(gpu_lib, cs):
    """The whole case set in the layout that puts every span length at every
    alignment (cs["aligns"]), exact capacities: the rule's results and the
    host path's, byte for byte."""
    want, caps = _with_caps(cs["raws"], cs["magic"], (1 << 40, 1 << 40, 1 << 40))
    assert caps == tuple(int(cs[f].sum()) for f in ("ntx", "gather", "msg"))
    got = _device_call(gpu_lib, cs["raws"], cs["magic"], caps, triple=cs["triple"])
    check(got, want)
    check(got, cs)
    for a, b in zip(got, BB.verify_byron_block_integrity(cs["triple"], cs["magic"], host=True)):
        np.testing.assert_array_equal(a, b)
    for kind, v in zip(cs["kinds"], got[0]):
        if kind in C.BROKEN:
            assert v == C.must_be(kind), kind


def test_device_resident_form_and_count_entry_on_every_flip(gpu_lib):
    raws = C.golden_flips()
    magic = C.parts()["magic_value"]
    want, caps = _with_caps(raws, magic, (1 << 40, 1 << 40, 1 << 40))
    got = _device_call(gpu_lib, raws, magic, caps)
    check(got, want)
    for a, b in zip(got, BB.verify_byron_block_integrity(raws, magic, host=True)):
        np.testing.assert_array_equal(a, b)
    st, ntx, gather, msg, totals = BB.count_byron_blocks(raws, magic)
    np.testing.assert_array_equal(st, want["status"])
    np.testing.assert_array_equal(ntx, want["ntx"])
    np.testing.assert_array_equal(gather, want["gather"])
    np.testing.assert_array_equal(msg, want["msg"])
    assert totals.tolist() == list(caps)
    for a, b in zip((st, ntx, gather, msg), BB.count_byron_blocks(raws, magic, host=True)):
        np.testing.assert_array_equal(a, b)


def test_one_wave_mixing_every_outcome(gpu_lib, cs, pool):
    """64 blocks on the device-resident form with exact capacities: valid
    blocks, every broken kind, EBBs, Shelley blocks, a truncated one, and a
    span outside the buffer"""
    kinds = {k: r for k, r in zip(cs["kinds"], cs["raws"]) if len(r) < 2500}
    raws = ([kinds[k] for k in C.BROKEN] + [kinds["count"], kinds["span"]] +
            list(C.golden().values()) + [pool[-1]])
    raws = (raws * 3)[:63]
    want, caps = _with_caps(raws, cs["magic"], (1 << 30, 1 << 30, 1 << 30))
    v, st, root = _device_call(gpu_lib, raws, cs["magic"], caps, extra_span=True)
    assert st[63] == BB.PACK_ESPAN and v[63] == 0 and not root[63].any()
    check((v[:63], st[:63], root[:63]), want)
    assert len(set(st.tolist())) >= 6 and len(set(v.tolist())) >= 8
    # each header's own magic, on the same form
    want, caps = _with_caps(raws, "header", (1 << 30, 1 << 30, 1 << 30))
    check(_device_call(gpu_lib, raws, -1, caps), want)


@pytest.mark.parametrize("short", [0, 1, 2])
def test_device_resident_form_one_short(gpu_lib, cs, short):
    """One transaction row, one gathered byte or one message byte short: the
    last regular block gets ECAP and writes nothing; the blocks before it and
    the EBB after it keep their results."""
    kinds = {k: r for k, r in zip(cs["kinds"], cs["raws"]) if len(r) < 2500}
    raws = [kinds["count"], kinds["tx_last"], C.golden()["cardano_disk_Byron_EBB"],
            kinds["wit_swapped"], C.golden()["cardano_n2n_Byron_regular"],
            C.golden()["cardano_n2n_Byron_EBB"]]
    _, full = _with_caps(raws, cs["magic"], (1 << 30, 1 << 30, 1 << 30))
    caps = tuple(c - (k == short) for k, c in enumerate(full))
    want, _ = _with_caps(raws, cs["magic"], caps)
    assert want["status"].tolist() == [0, 0, BB.PACK_EBB, 0, BB.PACK_ECAP, BB.PACK_EBB]
    check(_device_call(gpu_lib, raws, cs["magic"], caps), want)
    # ... and with room for the first block only
    c0 = _with_caps(raws[:1], cs["magic"], full)[1]
    want, _ = _with_caps(raws, cs["magic"], c0)
    assert want["status"].tolist() == [0, BB.PACK_ECAP, BB.PACK_EBB, BB.PACK_ECAP, BB.PACK_ECAP,
                                       BB.PACK_EBB]
    check(_device_call(gpu_lib, raws, cs["magic"], c0), want)


def test_device_entry_rejects_bad_work_and_alignment(gpu_lib, cs):
    """Every pointer is placed by hand inside one device allocation, at the
    alignment the entry documents and no better where it matters: raw at 4,
    off at 8, len at 4, tx_root at 16 (each an odd multiple), status and
    verdict at odd addresses."""
    import torch

    raw = C.golden()["cardano_disk_Byron_regular"]
    dev = torch.device("cuda", 0)
    area = torch.zeros(8192, dtype=torch.uint8, device=dev)
    base = (area.data_ptr() + 63) & ~63
    at = lambda k: base + k - area.data_ptr()  # noqa: E731
    p_raw, p_off, p_len = base + 4, base + 2048 + 8, base + 2048 + 64 + 4
    p_status, p_verdict, p_root = base + 2048 + 129, base + 2048 + 193, base + 2048 + 256 + 16
    padded = np.frombuffer(raw + bytes(-len(raw) % 4), np.uint8)
    area[at(4):at(4) + padded.size] = torch.tensor(padded.copy(), device=dev)
    area[at(2048 + 8):at(2048 + 16)] = torch.tensor(
        np.array([0], np.uint64).view(np.uint8).copy(), device=dev)
    area[at(2048 + 68):at(2048 + 72)] = torch.tensor(
        np.array([len(raw)], np.uint32).view(np.uint8).copy(), device=dev)
    wb = int(gpu_lib.ouro_byron_block_work_bytes(1, 1, 142, 337))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    args = [None, p_raw, len(raw), p_off, p_len, 1, -1, 1, 142, 337, work.data_ptr(), wb,
            p_status, p_verdict, p_root]
    fn = gpu_lib.ouro_byron_block_integrity_verify_cbor_device
    for k, delta in ((11, -1), (1, 1), (1, 2), (3, 4), (3, 1), (4, 2), (4, 1), (14, 8), (14, 1)):
        bad = list(args)
        bad[k] += delta
        assert fn(*bad) == _native.OURO_EINVAL, (k, delta)
    torch.cuda.synchronize()
    assert not area[at(2048 + 129):].any().item()          # nothing was launched
    assert fn(*args) == _native.OURO_OK
    torch.cuda.synchronize()
    got = area.cpu().numpy()
    assert got[at(2048 + 129)] == BB.PACK_OK and got[at(2048 + 193)] == BB.BYB_ALL_OK
    assert got[at(2048 + 272):at(2048 + 304)].tobytes() == C.expect(raw, "header")[2]


def test_host_buffer_form_in_groups(gpu_lib, cs, pool):
    """The byte budget forced small (OURO_BYRON_BLOCK_GROUP_BYTES): the batch
    spans many groups, a block larger than the budget is a group of its own."""
    big = [r for k, r in zip(cs["kinds"], cs["raws"]) if k == "count"][-1]     # 257 transactions
    raws = pool[:9] + [big] + pool[9:20]
    budget = sum(len(r) for r in raws[:3])
    assert len(big) > budget
    want = C.expected_arrays(raws, cs["magic"])
    with _native.knob_env(OURO_BYRON_BLOCK_GROUP_BYTES=str(budget)):
        check(BB.verify_byron_block_integrity(raws, cs["magic"]), want)
        st, ntx, gather, msg, totals = BB.count_byron_blocks(raws, cs["magic"])
    np.testing.assert_array_equal(st, want["status"])
    np.testing.assert_array_equal(ntx, want["ntx"])
    assert totals.tolist() == [int(want[f].sum()) for f in ("ntx", "gather", "msg")]


CHILD = r"""
import ctypes, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
torch.cuda.init()
import byron_block_cases as C
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron_block as BB
lib = _native.load()
assert _native.test_hooks()
cs = C.case_set()
raws = [r for k, r in zip(cs["kinds"], cs["raws"]) if k != "count"]
a, b0, b1 = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b0))
v, st, root = BB.verify_byron_block_integrity(raws, cs["magic"])
assert b"recomputed on the host path" in lib.ouro_last_error()
cnt = BB.count_byron_blocks(raws, cs["magic"])
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b1))
assert b1.value - b0.value == 2, (b0.value, b1.value)
want = C.expected_arrays(raws, cs["magic"])
assert (st == want["status"]).all() and (v == want["verdict"]).all()
assert (root == want["tx_root"]).all() and (cnt[1] == want["ntx"]).all()
os.environ["OURO_ON_DEVICE_ERROR"] = "fail"
lib.ouro_debug_reload_knobs()
try:
    BB.verify_byron_block_integrity(raws, cs["magic"])
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
