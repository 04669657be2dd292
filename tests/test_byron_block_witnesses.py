"""The host entries of the Byron transaction-witness feature
(ouro_byron_block_witness_verify_cbor_host, ..._count_cbor_host; CPU only)
against the rule of byron_witness.py, rows byte for byte
(tests/byron_witness_cases.py): the case set, the magics, every flip and every
truncation of the golden block, the capacities, every OURO_EINVAL."""
import ctypes

import numpy as np
import pytest

import byron_block_cases as C
import byron_witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as BY
from ouroboros_network_amd import byron_block as BB
from ouroboros_network_amd import byron_witness as BW

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def check_against_rule(raws, magic, triple=None):
    want = WC.expected_arrays(raws, magic)
    triple = triple or C.layout(raws)
    WC.check_result(BW.verify_byron_block_witnesses(triple, magic, host=True), want)
    status, ntx, nwit = BW.count_byron_block_witnesses(triple, magic, host=True)
    for got, f in ((status, "status"), (ntx, "ntx"), (nwit, "nwit")):
        np.testing.assert_array_equal(got, want[f], f)
    return want


def test_host_entries_on_the_case_set():
    cs = WC.case_set()
    want = check_against_rule(cs["raws"], cs["magic"], cs["triple"])
    for f in ("status", "verdict", "n_bad", "wit_ok"):
        np.testing.assert_array_equal(want[f], cs[f])
    assert (want["status"] == BW.PACK_OK).sum() > 40 and (want["n_bad"] > 0).sum() >= 8
    assert (want["wit_ok"] == 1).sum() > 1000


def test_every_magic_and_each_headers_own():
    raws = WC.magic_set()
    own = check_against_rule(raws, BY.HEADER_MAGIC)
    assert own["verdict"].tolist() == [1] * len(WC.MAGICS) + [0] and own["n_bad"][-1] == 5
    for k, m in enumerate(WC.MAGICS):
        want = check_against_rule(raws, m)
        assert want["verdict"][k] == 1 and want["verdict"].sum() == 1 + (m == WC.GOLDEN_MAGIC)


def test_statuses_outside_the_witness_vectors_are_the_block_walkers():
    """Every flip and every truncation of the golden block against the rule;
    where the rule's status does not come from inside a witness vector it is
    the one ouro_byron_block_count_cbor_host gives the same bytes."""
    m = WC.GOLDEN_MAGIC
    cs = WC.case_set()
    for raws in (C.golden_flips(), C.golden_truncations(), cs["raws"]):
        want = check_against_rule(raws, m)
        outer = BB.count_byron_blocks(raws, m, host=True)[0]
        inside = np.array([BW.byron_witness_error_in_vector(r) for r in raws])
        np.testing.assert_array_equal(outer[~inside], want["status"][~inside])
        assert np.isin(want["status"][inside], (BW.PACK_ESHAPE, BW.PACK_ESIZE, BW.PACK_ECBOR)).all()
        if raws is cs["raws"]:
            assert sorted(np.array(cs["kinds"])[inside]) == sorted(
                k for k, v in WC.BROKEN.items() if isinstance(v, int))
        elif len(raws[0]) == len(raws[-1]):         # the flips: some land in the witness vector
            assert inside.sum() >= 5 and (want["status"] == BW.PACK_OK).sum() > 500
        else:
            assert not inside.any() and (want["status"] == BW.PACK_ECBOR).all()


def _small():
    p = WC.pool()
    raws = [p[0], p[3], p[7], p[8], p[4], p[5]]
    return raws, WC.expected_arrays(raws, WC.GOLDEN_MAGIC)


@pytest.mark.parametrize("short", ["tx", "wit"])
def test_capacity_one_row_short(short):
    """The last block gets ECAP, the blocks before it are untouched (the host
    form leaves rows past the blocks that fit alone), the totals are right."""
    raws, full = _small()
    T, Wn = int(full["tx_begin"][-1]), int(full["wit_begin"][-1])
    tc, wc = T - (short == "tx"), Wn - (short == "wit")
    want = WC.expected_arrays(raws, WC.GOLDEN_MAGIC, tc, wc)
    assert want["status"].tolist() == full["status"].tolist()[:-1] + [BW.PACK_ECAP]
    r = BW.verify_byron_block_witnesses(raws, WC.GOLDEN_MAGIC, tx_cap=tc, wit_cap=wc, host=True)
    WC.check_result(r, want)


def test_exact_capacities_fit_and_zero_capacities_reject_every_block_with_rows():
    raws, want = _small()
    WC.check_result(BW.verify_byron_block_witnesses(raws, WC.GOLDEN_MAGIC, host=True), want)
    assert want["status"].tolist().count(BW.PACK_EBB) == 1 and want["n_bad"].sum() == 1
    r = BW.verify_byron_block_witnesses(raws, WC.GOLDEN_MAGIC, tx_cap=0, wit_cap=0, host=True)
    WC.check_result(r, WC.expected_arrays(raws, WC.GOLDEN_MAGIC, 0, 0))
    # (an empty block fits only while its rows begin inside the capacities)
    assert r.status.tolist() == [BW.PACK_OK, BW.PACK_ECAP, BW.PACK_EBB] + [BW.PACK_ECAP] * 3
    assert r.verdict.tolist() == [1, 0, 1, 0, 0, 0]


def test_more_blocks_than_one_task_of_the_host_path():
    p = WC.pool()
    raws = [p[(5 * i + i // 7) % len(p)] for i in range(300)]
    check_against_rule(raws, WC.GOLDEN_MAGIC)


def _call(name, **over):
    """One call with an argument replaced: the return code"""
    raws = [C.golden()["cardano_disk_Byron_regular"], C.golden()["cardano_disk_Byron_EBB"]]
    buf, off, ln = C.layout(raws)
    n = len(raws)
    lib = _native.load()
    st, ver = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    bad, a32, b32 = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    tb, wb = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    rows = {f: np.zeros(64 * 8, np.uint8) for f in ("tx_id", "wit_tx", "wit_kind", "wit_ok",
                                                    "wit_vk")}
    a = dict(raw=P(buf), raw_bytes=buf.size, off=P(off), len=P(ln), n=n, magic=-1, status=P(st),
             verdict=P(ver), n_bad=P(bad), ntx=P(a32), nwit=P(b32), tx_begin=P(tb), wit_begin=P(wb),
             tx_cap=4, wit_cap=8, out=True, work=ctypes.c_void_p(64), work_bytes=1 << 20,
             **{f: P(v) for f, v in rows.items()})
    a.update(over)
    if "count" in name:
        return getattr(lib, name)(a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"], a["magic"],
                                  a["status"], a["ntx"], a["nwit"])
    out = BW.ByronWitnessOutC(a["tx_cap"], a["wit_cap"], a["tx_begin"], a["wit_begin"], a["tx_id"],
                              a["wit_tx"], a["wit_kind"], a["wit_ok"], a["wit_vk"])
    o = ctypes.byref(out) if a["out"] else None
    if name.endswith("_device"):
        return getattr(lib, name)(None, a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"],
                                  a["magic"], o, a["work"], a["work_bytes"], a["status"],
                                  a["verdict"], a["n_bad"])
    return getattr(lib, name)(a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"], a["magic"], o,
                              a["status"], a["verdict"], a["n_bad"])


VERIFY = "ouro_byron_block_witness_verify_cbor"
COUNT = "ouro_byron_block_witness_count_cbor"


@pytest.mark.parametrize("suffix", ["_host", ""])
def test_every_einval(suffix):
    """before any work, so the device-side entries never reach a device here"""
    verify, count = VERIFY + suffix, COUNT + suffix
    if suffix:
        assert _call(verify) == _native.OURO_OK
        assert _call(verify, wit_vk=None) == _native.OURO_OK      # wit_vk may be NULL
        assert _call(count) == _native.OURO_OK
        assert _call(verify, magic=2**32 - 1) == _native.OURO_OK
    for arg in ("raw", "off", "len", "status", "verdict", "n_bad", "tx_begin", "wit_begin", "tx_id",
                "wit_tx", "wit_kind", "wit_ok"):
        assert _call(verify, **{arg: None}) == _native.OURO_EINVAL, arg
    assert _call(verify, out=False) == _native.OURO_EINVAL
    for arg in ("raw", "off", "len", "status", "ntx", "nwit"):
        assert _call(count, **{arg: None}) == _native.OURO_EINVAL, arg
    for name in (verify, count):
        assert _call(name, raw_bytes=100) == _native.OURO_EINVAL        # a span outside raw_bytes
        assert _call(name, off=P(np.array([2**63, 0], np.uint64))) == _native.OURO_EINVAL
        for magic in (-2, 2**32, -2**40):
            assert _call(name, magic=magic) == _native.OURO_EINVAL, magic
        assert b"protocol_magic" in _native.load().ouro_last_error()
        assert _call(name, n=0, raw=None, off=None) == _native.OURO_OK
    assert _call(verify, tx_cap=1 << 32) == _native.OURO_EINVAL          # above 2^32 - 1 rows
    assert _call(verify, wit_cap=1 << 32) == _native.OURO_EINVAL


# ouro_byron_block_witness_work_bytes(n, tx_cap, wit_cap) as the entry answered
# before the witness flow was shared between the eras: n at one tile of the
# scan, one past it and many; no rows, one row, and capacities at which every
# term counts
WORK_BYTES = {
    (1, 0, 0): 704,
    (1, 1, 1): 1024,
    (1, 100003, 250007): 33601792,
    (1024, 0, 0): 16896,
    (1024, 1, 1): 17216,
    (1024, 100003, 250007): 33617984,
    (1025, 0, 0): 17088,
    (1025, 1, 1): 17408,
    (1025, 100003, 250007): 33618176,
    (70000, 0, 0): 1121600,
    (70000, 1, 1): 1121920,
    (70000, 100003, 250007): 34722688,
}


def test_work_area_sizes_are_unchanged():
    wb = _native.load().ouro_byron_block_witness_work_bytes
    assert {a: int(wb(*a)) for a in WORK_BYTES} == WORK_BYTES


def test_device_entry_einval_before_any_work():
    name = VERIFY + "_device"
    wb = _native.load().ouro_byron_block_witness_work_bytes
    assert wb(10, 5, 7) < wb(11000, 5, 7) and wb(10, 5, 7) < wb(10, 500, 7) < wb(10, 500, 700)
    need = wb(2, 4, 8)
    for arg in ("raw", "off", "len", "work", "status", "verdict", "n_bad", "tx_begin", "wit_begin",
                "tx_id", "wit_tx", "wit_kind", "wit_ok"):
        assert _call(name, **{arg: None}) == _native.OURO_EINVAL, arg
    assert _call(name, out=False) == _native.OURO_EINVAL
    assert _call(name, magic=2**32) == _native.OURO_EINVAL and _call(name, magic=-2) == _native.OURO_EINVAL
    assert _call(name, work_bytes=need - 1) == _native.OURO_EINVAL
    assert b"work area" in _native.load().ouro_last_error()
    assert _call(name, tx_cap=1 << 32, work_bytes=1 << 62) == _native.OURO_EINVAL
    a = np.zeros(256, np.uint8)
    base = a.ctypes.data + (-a.ctypes.data % 16)
    for arg, k in (("raw", 1), ("off", 4), ("tx_begin", 4), ("wit_begin", 4), ("tx_id", 8),
                   ("wit_vk", 8), ("wit_tx", 2), ("n_bad", 2), ("len", 2)):
        assert _call(name, **{arg: ctypes.c_void_p(base + k)}) == _native.OURO_EINVAL, arg
    assert b"aligned" in _native.load().ouro_last_error()
    assert _call(name, n=0) == _native.OURO_OK
