"""Whole-block storage integrity on the host path (CPU-only):
ouro_block_integrity_verify_cbor_host and ouro_blake2b256_batch_host against
block.parse_block, hashlib and the oracle's kes_verify (tests/block_cases.py),
never against the library itself."""
import ctypes
import hashlib

import numpy as np
import pytest

import block_cases as BC
from ouroboros_network_amd import _native
from ouroboros_network_amd import block as B


@pytest.fixture(scope="module")
def cs():
    return BC.case_set()


@pytest.fixture(scope="module")
def host(cs):
    """the _host entry over the whole case set, once"""
    return B.verify_block_integrity_cbor(cs["triple"], BC.SPKP, host=True)


def _rows(cs, *kinds):
    return [i for i, k in enumerate(cs["kinds"]) if k in kinds]


def test_case_set_covers_the_issue(cs):
    """the set holds what it claims: every length at every alignment, the
    four encodings, and a few hundred blocks"""
    buf, off, ln = cs["triple"]
    seen = set()
    for i in _rows(cs, "synthetic"):
        pb = B.parse_block(cs["raws"][i])
        o, n = pb.segments[0]
        seen.add((n, (int(off[i]) + o) % 4))
    for n in BC.SEG_LENGTHS:
        for a in range(4):
            assert (n, a) in seen
    firsts = {bytes(cs["raws"][i][:1]) for i in _rows(cs, "synthetic")}
    assert firsts == {b"\x84", b"\xd8", b"\x82"}
    assert 300 <= len(cs["raws"]) <= 900


def test_golden_blocks(cs, host):
    verdict, status, body_hash = host
    rows = _rows(cs, "golden")
    assert len(rows) == 8
    for i in rows:
        pb = B.parse_block(cs["raws"][i])
        assert status[i] == B.PACK_OK
        assert verdict[i] & B.BLK_BODY_OK
        assert body_hash[i].tobytes() == pb.body_hash
        assert bool(verdict[i] & B.BLK_KES_OK) == bool(cs["verdict"][i] & B.BLK_KES_OK)
        assert cs["verdict"][i] == B.BLK_ALL_OK  # (what the oracle says: expected true)
    # the segment sizes the golden files pin
    sizes = {b["name"]: [n for _, n in B.parse_block(bytes.fromhex(b["raw"])).segments]
             for b in BC.golden() if not b["byron"]}
    assert sizes["shelley_disk"] == [450, 206, 27]
    assert sizes["cardano_disk_Allegra"] == [450, 206, 141]
    assert sizes["cardano_n2n_Mary"] == [543, 206, 141]


def test_byron_blocks(cs, host):
    verdict, status, body_hash = host
    rows = _rows(cs, "byron")
    assert len(rows) == 4
    for i in rows:
        assert status[i] == B.PACK_EBYRON and verdict[i] == 0
        assert not body_hash[i].any()


def test_synthetic_blocks(cs, host):
    verdict, status, body_hash = host
    rows = _rows(cs, "synthetic")
    assert len(rows) == 4 * len(BC.SEG_LENGTHS) + 1
    for i in rows:
        assert cs["status"][i] == B.PACK_OK and cs["verdict"][i] == B.BLK_ALL_OK
        assert status[i] == B.PACK_OK and verdict[i] == B.BLK_ALL_OK, i
        assert body_hash[i].tobytes() == cs["body_hash"][i].tobytes()


def test_single_byte_flips(cs, host):
    verdict, status, _ = host
    want = {"flip_seg": B.BLK_KES_OK, "flip_hash": 0, "flip_body": B.BLK_BODY_OK}
    n = 0
    for kind, v in want.items():
        for i in _rows(cs, kind):
            assert cs["status"][i] == B.PACK_OK and cs["verdict"][i] == v, (kind, i)
            assert status[i] == B.PACK_OK and verdict[i] == v, (kind, i)
            n += 1
    assert n == 5 * (8 + 4 * len(BC.SEG_LENGTHS) + 1)


def test_shape_and_truncation(cs, host):
    verdict, status, body_hash = host
    rows = _rows(cs, "shape")
    np.testing.assert_array_equal(status[rows], cs["status"][rows])
    np.testing.assert_array_equal(verdict[rows], cs["verdict"][rows])
    seen = set(int(s) for s in cs["status"][rows])
    assert {B.PACK_OK, B.PACK_ECBOR, B.PACK_ESHAPE, B.PACK_EBYRON} <= seen
    # nesting: cbor::skip's stack holds 64 open containers.  A segment of 63
    # arrays around an empty one opens 64 and fits; 64, 65 and 200 around it
    # open one too many
    deep = [i for i in rows if cs["raws"][i].endswith(b"\x81\x80")]
    assert [int(cs["status"][i]) for i in deep] == [B.PACK_OK, B.PACK_ECBOR, B.PACK_ECBOR,
                                                    B.PACK_ECBOR]


def test_everything_matches_the_expectations(cs, host):
    verdict, status, body_hash = host
    np.testing.assert_array_equal(status, cs["status"])
    np.testing.assert_array_equal(verdict, cs["verdict"])
    np.testing.assert_array_equal(body_hash, cs["body_hash"])
    # the status invariant
    assert not ((verdict != 0) & (status != B.PACK_OK)).any()
    assert not body_hash[status != B.PACK_OK].any()


def test_body_hash_may_be_null(cs, host):
    buf, off, ln = cs["triple"]
    n = 40
    st, v = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lib = _native.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.ouro_block_integrity_verify_cbor_host(p(buf), buf.size, p(off), p(ln), n, BC.SPKP,
                                                     p(st), p(v), None) == 0
    np.testing.assert_array_equal(v, host[0][:n])
    np.testing.assert_array_equal(st, host[1][:n])


@pytest.mark.parametrize("entry", ["ouro_block_integrity_verify_cbor_host",
                                   "ouro_block_integrity_verify_cbor"])
def test_bad_arguments_are_einval_before_any_work(cs, entry):
    buf, off, ln = cs["triple"]
    n = 4
    lib = _native.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = getattr(lib, entry)
    st, v = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
    bad = off[:n].copy()
    bad[2] = buf.size - 3
    assert fn(p(buf), buf.size, p(bad), p(ln), n, BC.SPKP, p(st), p(v), None) == _native.OURO_EINVAL
    assert fn(p(buf), buf.size, p(off), p(ln), n, 0, p(st), p(v), None) == _native.OURO_EINVAL
    assert fn(None, buf.size, p(off), p(ln), n, BC.SPKP, p(st), p(v), None) == _native.OURO_EINVAL
    assert fn(p(buf), buf.size, p(off), p(ln), n, BC.SPKP, None, p(v), None) == _native.OURO_EINVAL
    assert (st == 9).all() and (v == 9).all()
    assert fn(p(buf), buf.size, p(off), p(ln), 0, BC.SPKP, p(st), p(v), None) == 0


# ---- the generic batched hash ----
def test_blake2b_host_lengths_and_alignments():
    buf, off, ln = BC.hash_spans()
    got = B.blake2b256_batch((buf, off, ln), host=True)
    np.testing.assert_array_equal(got, BC.hash_expect(buf, off, ln))


@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_blake2b_host_counts(n):
    rng = np.random.default_rng(n)
    msgs = [rng.bytes(int(rng.integers(0, 700))) for _ in range(n)]
    got = B.blake2b256_batch(msgs, host=True)
    assert got.shape == (n, 32)
    for g, m in zip(got, msgs):
        assert g.tobytes() == hashlib.blake2b(m, digest_size=32).digest()


def test_blake2b_span_outside_the_buffer_is_einval():
    buf = np.zeros(100, np.uint8)
    out = np.full((2, 32), 7, np.uint8)
    lib = _native.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for off, ln in (([0, 90], [10, 11]), ([0, 101], [10, 0]), ([0, 2**63], [1, 1])):
        o, l_ = np.array(off, np.uint64), np.array(ln, np.uint32)
        for name in ("ouro_blake2b256_batch_host", "ouro_blake2b256_batch"):
            assert getattr(lib, name)(2, p(buf), buf.size, p(o), p(l_), p(out)) == \
                _native.OURO_EINVAL
    assert (out == 7).all()
    with pytest.raises(ValueError):
        B.blake2b256_batch((buf, [95], [6]), host=True)
