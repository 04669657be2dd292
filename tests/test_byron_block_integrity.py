"""Byron whole-block integrity on the host path (CPU): the _host and count
entries of include/ouro_verify.h against the rule of byron_block.py on the
case set, on every single-byte flip and every truncation of the reference's
golden Byron block; every OURO_EINVAL; and the Byron HEADER slicer's rows, which
the split of byron_pack_one must leave as they were."""
import ctypes

import numpy as np
import pytest

import byron_block_cases as C
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as BY
from ouroboros_network_amd import byron_block as BB

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def check_against_rule(raws, magic, triple=None):
    want = C.expected_arrays(raws, magic)
    triple = triple or C.layout(raws)
    v, st, root = BB.verify_byron_block_integrity(triple, magic, host=True)
    np.testing.assert_array_equal(st, want["status"])
    np.testing.assert_array_equal(v, want["verdict"])
    np.testing.assert_array_equal(root, want["tx_root"])
    s2, ntx, gather, msg, totals = BB.count_byron_blocks(triple, magic, host=True)
    np.testing.assert_array_equal(s2, want["status"])
    np.testing.assert_array_equal(ntx, want["ntx"])
    np.testing.assert_array_equal(gather, want["gather"])
    np.testing.assert_array_equal(msg, want["msg"])
    assert totals.tolist() == [int(want[f].sum()) for f in ("ntx", "gather", "msg")]
    return want


def test_host_entries_on_the_case_set():
    cs = C.case_set()
    want = check_against_rule(cs["raws"], cs["magic"], cs["triple"])
    for f in ("status", "verdict"):
        np.testing.assert_array_equal(want[f], cs[f])
    assert not ((want["verdict"] != 0) & ~np.isin(want["status"], (BB.PACK_OK, BB.PACK_EBB))).any()


def test_each_headers_own_magic():
    """HEADER_MAGIC (-1): the block signed under its own, other magic verifies;
    the one whose field was changed after signing does not."""
    cs = C.case_set()
    raws = [r for k, r in zip(cs["kinds"], cs["raws"]) if k in ("magic_field", "magic_signed",
                                                                "golden_byron", "sig")]
    want = check_against_rule(raws, BY.HEADER_MAGIC)
    assert sorted(want["verdict"].tolist()) == [126, 126, 127, 127, 127, 127, 127]


def test_every_flip_of_the_golden_block():
    raws = C.golden_flips()
    want = check_against_rule(raws, C.parts()["magic_value"])
    # a flip lands in the signed bytes, in the body, or breaks the slicing
    assert (want["status"] == BB.PACK_OK).sum() > 500 and (want["status"] != BB.PACK_OK).sum() > 20
    assert len({int(v) for v in want["verdict"]}) >= 6
    # (bytes nothing signs or hashes stay unnoticed: the SSC payload, the block's extra data,
    # the certificate's own signature and epoch, non-canonical heads the slicer reads alike)
    assert (want["verdict"] == BB.BYB_ALL_OK).sum() < len(raws) // 4


def test_every_truncation_of_the_golden_block():
    raws = C.golden_truncations()
    want = check_against_rule(raws, C.parts()["magic_value"])
    assert not want["verdict"].any() and (want["status"] == BB.PACK_ECBOR).all()


def test_chunks_of_the_host_path():
    """more blocks than one chunk of the host path (4,096)"""
    cs = C.case_set()
    pool = [r for k, r in zip(cs["kinds"], cs["raws"]) if k != "count" or len(r) < 3000]
    raws = [pool[(7 * i + i // 11) % len(pool)] for i in range(4096 + 37)]
    exp = {r: C.expect(r, cs["magic"]) for r in set(raws)}
    v, st, root = BB.verify_byron_block_integrity(raws, cs["magic"], host=True)
    assert st.tolist() == [exp[r][0] for r in raws]
    assert v.tolist() == [exp[r][1] for r in raws]
    assert root.tobytes() == b"".join(exp[r][2] for r in raws)


def _args(n=2, magic=-1, **kw):
    raws = [C.golden()["cardano_disk_Byron_regular"], C.golden()["cardano_disk_Byron_EBB"]]
    buf, off, ln = C.layout(raws)
    a = dict(raw=P(buf), raw_bytes=buf.size, off=P(off), len=P(ln), n=n, magic=magic,
             status=P(np.zeros(2, np.uint8)), verdict=P(np.zeros(2, np.uint8)),
             tx_root=P(np.zeros(64, np.uint8)), keep=(buf, off, ln))
    a.update(kw)
    return a


VERIFY = ("raw", "raw_bytes", "off", "len", "n", "magic", "status", "verdict", "tx_root")


@pytest.mark.parametrize("entry", ["ouro_byron_block_integrity_verify_cbor_host",
                                   "ouro_byron_block_integrity_verify_cbor"])
def test_verify_einval(entry):
    """before any work, so the device entry never reaches a device here"""
    fn = getattr(_native.load(), entry)

    def call(**kw):
        a = _args(**kw)                      # (alive until the call returns)
        return fn(*[a[k] for k in VERIFY])

    for name in ("raw", "off", "len", "status", "verdict"):
        assert call(**{name: None}) == _native.OURO_EINVAL, name
    assert call(raw_bytes=100) == _native.OURO_EINVAL          # a span outside raw_bytes
    off = np.array([2**63, 0], np.uint64)
    assert call(off=P(off)) == _native.OURO_EINVAL
    for magic in (-2, 2**32, -2**40):
        assert call(magic=magic) == _native.OURO_EINVAL, magic
    assert call(n=0, raw=None, off=None) == _native.OURO_OK
    if entry.endswith("_host"):
        assert call(tx_root=None) == _native.OURO_OK            # optional
        assert call(magic=2**32 - 1) == _native.OURO_OK
        assert b"protocol_magic" in (call(magic=-2), _native.load().ouro_last_error())[1]


@pytest.mark.parametrize("entry", ["ouro_byron_block_count_cbor_host",
                                   "ouro_byron_block_count_cbor"])
def test_count_einval(entry):
    fn = getattr(_native.load(), entry)
    cnt = [np.zeros(2, np.uint32) for _ in range(3)]
    tot = np.full(3, 9, np.uint64)

    def call(**kw):
        a = _args(**kw)
        extra = dict(ntx=P(cnt[0]), gather=P(cnt[1]), msg=P(cnt[2]), totals=P(tot))
        extra.update({k: v for k, v in kw.items() if k in extra})
        return fn(a["raw"], a["raw_bytes"], a["off"], a["len"], a["n"], a["magic"], a["status"],
                  extra["ntx"], extra["gather"], extra["msg"], extra["totals"])

    for name in ("raw", "off", "len", "status", "ntx", "gather", "msg", "totals"):
        assert call(**{name: None}) == _native.OURO_EINVAL, name
    assert call(raw_bytes=100) == _native.OURO_EINVAL
    assert call(magic=2**32) == _native.OURO_EINVAL and call(magic=-2) == _native.OURO_EINVAL
    assert call(n=0) == _native.OURO_OK and tot.tolist() == [0, 0, 0]


# ouro_byron_block_work_bytes(n, tx_cap, gather_cap, msg_cap) as the entry
# answered before its scan became scan_excl.h's: n at one tile of the scan, one
# past it and many; no rows, one of each, and capacities at which every term
# counts
WORK_BYTES = {
    (1, 0, 0, 0): 2176,
    (1, 1, 1, 1): 2496,
    (1, 100003, 250007, 3000017): 7652544,
    (1024, 0, 0, 0): 591680,
    (1024, 1, 1, 1): 592000,
    (1024, 100003, 250007, 3000017): 8242048,
    (1025, 0, 0, 0): 593024,
    (1025, 1, 1, 1): 593344,
    (1025, 100003, 250007, 3000017): 8243392,
    (70000, 0, 0, 0): 40392448,
    (70000, 1, 1, 1): 40392768,
    (70000, 100003, 250007, 3000017): 48042816,
}


def test_work_area_sizes_are_unchanged():
    wb = _native.load().ouro_byron_block_work_bytes
    assert {a: int(wb(*a)) for a in WORK_BYTES} == WORK_BYTES


def test_device_entry_einval_before_any_work():
    lib = _native.load()
    a = _args()
    wb = lib.ouro_byron_block_work_bytes(2, 1, 142, 337)
    assert wb > 0 and lib.ouro_byron_block_work_bytes(2, 100, 142, 337) > wb

    def call(**kw):
        b = dict(a, work=ctypes.c_void_p(64), work_bytes=wb, caps=(1, 142, 337))
        b.update(kw)
        return lib.ouro_byron_block_integrity_verify_cbor_device(
            None, b["raw"], b["raw_bytes"], b["off"], b["len"], b["n"], b["magic"], *b["caps"],
            b["work"], b["work_bytes"], b["status"], b["verdict"], b["tx_root"])

    for name in ("raw", "off", "len", "work", "status", "verdict"):
        assert call(**{name: None}) == _native.OURO_EINVAL, name
    assert call(magic=2**32) == _native.OURO_EINVAL
    assert call(work_bytes=wb - 1) == _native.OURO_EINVAL
    assert call(caps=(2**32, 142, 337), work_bytes=2**62) == _native.OURO_EINVAL
    assert call(raw=ctypes.c_void_p(a["raw"].value + 1)) == _native.OURO_EINVAL
    assert call(tx_root=ctypes.c_void_p(a["tx_root"].value + 8)) == _native.OURO_EINVAL
    assert call(n=0) == _native.OURO_OK


def test_header_slicer_rows_unchanged_on_the_golden_wire_forms(kats):
    """byron_pack_one after its split: the rows of the golden Byron header in
    its three wire forms are what byron.parse_byron_header states."""
    import envelope_cases as EC

    raw = bytes.fromhex(kats["byron"]["raw"])
    h = BY.parse_byron_header(raw)
    item = bytes.fromhex(EC.fixtures()["byron_regular_header"])
    forms = [EC.byron_wire(1, item, f) for f in (1, 2, 3)]
    assert raw in forms
    for magic in (kats["byron"]["magic"], BY.HEADER_MAGIC, 0, 2**32 - 1):
        pk = BY.pack_byron_cbor(forms, magic)
        assert pk.status.tolist() == [BY.PACK_OK] * 3
        for i in range(3):
            assert pk.message(i) == h.message(magic)
            assert pk.pk[i].tobytes() == h.delegate_xpub[:32] and pk.sig[i].tobytes() == h.sig
            assert pk.genesis_vk[i].tobytes() == h.issuer_xpub
            assert pk.delegate_vk[i].tobytes() == h.delegate_xpub
            assert int(pk.magic[i]) == h.magic
