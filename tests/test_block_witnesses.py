"""The host entries of the transaction-witness feature
(ouro_block_witness_verify_cbor_host, ouro_block_witness_count_cbor_host;
CPU-only) against the rule: witness.parse_witnesses for the status and the
rows, hashlib for the tx ids, the oracle's ed25519_verify for the verdicts
(tests/witness_cases.py)."""
import ctypes

import numpy as np
import pytest

import witness_cases as WC
from ouroboros_network_amd import _native
from ouroboros_network_amd import block as B
from ouroboros_network_amd import witness as W


def test_host_entry_matches_the_rule_on_the_whole_case_set():
    cs = WC.case_set()
    r = W.verify_block_witnesses(cs["triple"], host=True)
    WC.check_result(r, cs)
    assert (r.status == B.PACK_OK).sum() > 40 and (r.n_bad > 0).sum() >= 5


def test_count_entry_alone():
    cs = WC.case_set()
    status, ntx, nwit = W.count_block_witnesses(cs["triple"], host=True)
    assert status.tolist() == cs["status"].tolist()
    assert ntx.tolist() == np.diff(cs["tx_begin"]).tolist()
    assert nwit.tolist() == np.diff(cs["wit_begin"]).tolist()


def _small():
    raws = [r for r, _ in WC.valid()[-4:]] + [WC.malformed()[0][0]] + [WC.invalid()[0][0]]
    return raws, WC.expected_arrays(raws)


@pytest.mark.parametrize("short", ["tx", "wit"])
def test_capacity_one_row_short(short):
    """The last block gets ECAP, the blocks before it are untouched, the
    totals are still right."""
    raws, want = _small()
    T, Wn = int(want["tx_begin"][-1]), int(want["wit_begin"][-1])
    r = W.verify_block_witnesses(raws, tx_cap=T - (short == "tx"), wit_cap=Wn - (short == "wit"),
                                 host=True)
    assert r.tx_begin.tolist() == want["tx_begin"].tolist()
    assert r.wit_begin.tolist() == want["wit_begin"].tolist()
    assert r.status[-1] == W.PACK_ECAP and r.verdict[-1] == 0 and r.n_bad[-1] == 0
    for f in ("status", "verdict", "n_bad"):
        assert getattr(r, f)[:-1].tolist() == want[f][:-1].tolist()
    t0, w0 = int(want["tx_begin"][-2]), int(want["wit_begin"][-2])
    assert np.array_equal(r.tx_id[:t0], want["tx_id"][:t0])
    for f in ("wit_tx", "wit_kind", "wit_vk", "wit_ok"):
        assert np.array_equal(getattr(r, f)[:w0], want[f][:w0]), f


def test_exact_capacities_fit_and_zero_capacities_reject_every_block_with_rows():
    raws, want = _small()
    WC.check_result(W.verify_block_witnesses(raws, host=True), want)
    r = W.verify_block_witnesses(raws, tx_cap=0, wit_cap=0, host=True)
    for i in range(len(raws)):
        if want["status"][i] == B.PACK_OK:   # it fits iff its rows end at row 0
            rows = int(want["tx_begin"][i + 1]) + int(want["wit_begin"][i + 1])
            assert r.status[i] == (W.PACK_ECAP if rows else B.PACK_OK)
        else:
            assert r.status[i] == want["status"][i]


def _call(name, raws, **over):
    """One verify / count call with an argument replaced: the return code"""
    buf, off, ln = WC.layout(raws)
    n = len(raws)
    lib = _native.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    st, ver = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    bad, a32, b32 = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    tb, wb = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    rows = {f: np.zeros(64 * 200, np.uint8) for f in ("tx_id", "wit_tx", "wit_kind", "wit_ok",
                                                      "wit_vk")}
    a = dict(raw=p(buf), raw_bytes=buf.size, off=p(off), len=p(ln), n=n, status=p(st),
             verdict=p(ver), n_bad=p(bad), ntx=p(a32), nwit=p(b32), tx_begin=p(tb), wit_begin=p(wb),
             tx_cap=100, wit_cap=200, out=True, **{f: p(v) for f, v in rows.items()})
    a.update(over)
    if "count" in name:
        return getattr(lib, name)(a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"],
                                  a["status"], a["ntx"], a["nwit"])
    out = W.WitnessOutC(a["tx_cap"], a["wit_cap"], a["tx_begin"], a["wit_begin"], a["tx_id"],
                        a["wit_tx"], a["wit_kind"], a["wit_ok"], a["wit_vk"])
    return getattr(lib, name)(a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"],
                              ctypes.byref(out) if a["out"] else None, a["status"], a["verdict"],
                              a["n_bad"])


VERIFY = "ouro_block_witness_verify_cbor_host"
COUNT = "ouro_block_witness_count_cbor_host"


def test_every_einval():
    raws = [r for r, _ in WC.valid()[-2:]]
    assert _call(VERIFY, raws) == _native.OURO_OK
    assert _call(VERIFY, raws, wit_vk=None) == _native.OURO_OK      # wit_vk may be NULL
    assert _call(COUNT, raws) == _native.OURO_OK
    for arg in ("raw", "off", "len", "status", "verdict", "n_bad", "tx_begin", "wit_begin", "tx_id",
                "wit_tx", "wit_kind", "wit_ok"):
        assert _call(VERIFY, raws, **{arg: None}) == _native.OURO_EINVAL, arg
    assert _call(VERIFY, raws, out=False) == _native.OURO_EINVAL
    for arg in ("raw", "off", "len", "status", "ntx", "nwit"):
        assert _call(COUNT, raws, **{arg: None}) == _native.OURO_EINVAL, arg
    # a span outside raw_bytes, before any work
    total = sum(len(r) for r in raws)
    for name in (VERIFY, COUNT):
        assert _call(name, raws, raw_bytes=total - 1) == _native.OURO_EINVAL
        assert _call(name, raws, raw_bytes=total) == _native.OURO_OK
    # a capacity above 2^32 - 1 rows
    assert _call(VERIFY, raws, tx_cap=1 << 32) == _native.OURO_EINVAL
    # the work area of the device form grows with each of its arguments
    wb = _native.load().ouro_block_witness_work_bytes
    assert wb(10, 5, 7) < wb(11000, 5, 7) and wb(10, 5, 7) < wb(10, 500, 7) < wb(10, 500, 700)


# ouro_block_witness_work_bytes(n, tx_cap, wit_cap) as the entry answered before
# the witness flow was shared between the eras: n at one tile of the scan, one
# past it and many; no rows, one row, and capacities at which every term counts
WORK_BYTES = {
    (1, 0, 0): 640,
    (1, 1, 1): 960,
    (1, 100003, 250007): 25601536,
    (1024, 0, 0): 8704,
    (1024, 1, 1): 9024,
    (1024, 100003, 250007): 25609600,
    (1025, 0, 0): 8832,
    (1025, 1, 1): 9152,
    (1025, 100003, 250007): 25609728,
    (70000, 0, 0): 561600,
    (70000, 1, 1): 561920,
    (70000, 100003, 250007): 26162496,
}


def test_work_area_sizes_are_unchanged():
    wb = _native.load().ouro_block_witness_work_bytes
    assert {a: int(wb(*a)) for a in WORK_BYTES} == WORK_BYTES
