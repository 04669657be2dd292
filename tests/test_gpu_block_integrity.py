"""Whole-block storage integrity and the batched Blake2b-256 on the device:
the one-call entries, the length-class ordering across wave boundaries, the
pipeline cut into several chunks, the ordering switched off, the
device-resident forms -- against the expectations of tests/block_cases.py
(parse_block, hashlib, the oracle) and the host path."""
import ctypes
import hashlib

import numpy as np
import pytest

import block_cases as BC
from ouroboros_network_amd import _native
from ouroboros_network_amd import block as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cs():
    return BC.case_set()


@pytest.fixture(scope="module")
def mixed():
    """5 blocks with 70,000-byte bodies among 200 small ones: class counts that
    are no multiples of 64, so the permutation crosses wave boundaries; every
    13th block's body hash is wrong.  Returns (raws, expected verdicts, hashes)."""
    rng = np.random.default_rng(41)
    raws, verdict, hashes = [], [], []
    for i in range(205):
        big = i in (3, 50, 101, 102, 204)
        lens = (70000 if big else int(rng.integers(1, 400)), int(rng.integers(1, 200)),
                int(rng.integers(1, 600)) if i % 3 else 1)
        segs = [BC.segment(n, rng, as_map=bool(s % 2)) for s, n in enumerate(lens)]
        raw = BC.make_block(segs, form=i % 4, tag=2 + i % 3)
        if i % 13 == 5:
            o, n = B.parse_block(raw).segments[i % 3]
            raw = BC._flip_keeping_shape(raw, o, o + n)
        raws.append(raw)
    for raw in raws:
        st, v, h = BC.expect(raw)
        assert st == B.PACK_OK
        verdict.append(v)
        hashes.append(h)
    return raws, np.array(verdict, np.uint8), np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32)


def test_one_call_entry_on_the_case_set(gpu_lib, cs):
    verdict, status, body_hash = B.verify_block_integrity_cbor(cs["triple"], BC.SPKP)
    np.testing.assert_array_equal(status, cs["status"])
    np.testing.assert_array_equal(verdict, cs["verdict"])
    np.testing.assert_array_equal(body_hash, cs["body_hash"])
    hv, hs, hh = B.verify_block_integrity_cbor(cs["triple"], BC.SPKP, host=True)
    np.testing.assert_array_equal(verdict, hv)
    np.testing.assert_array_equal(status, hs)
    np.testing.assert_array_equal(body_hash, hh)
    assert not ((verdict != 0) & (status != B.PACK_OK)).any()


def test_length_classes_across_wave_boundaries(gpu_lib, mixed):
    raws, want_v, want_h = mixed
    verdict, status, body_hash = B.verify_block_integrity_cbor(raws, BC.SPKP)
    assert (status == B.PACK_OK).all()
    np.testing.assert_array_equal(verdict, want_v)
    np.testing.assert_array_equal(body_hash, want_h)
    assert (want_v == B.BLK_ALL_OK).sum() > 180 and (want_v == B.BLK_KES_OK).sum() >= 10


def test_several_chunks(gpu_lib, mixed, small_chunks):
    raws, want_v, want_h = mixed
    raws = raws * 4                       # 820 blocks: 4 chunks of 256
    small_chunks(CHUNK=256, SLOTS=2)
    verdict, status, body_hash = B.verify_block_integrity_cbor(raws, BC.SPKP)
    stats = (ctypes.c_double * 6)()
    assert gpu_lib.ouro_debug_cbor_stats(stats) == 0 and stats[3] >= 3
    assert (status == B.PACK_OK).all()
    np.testing.assert_array_equal(verdict, np.tile(want_v, 4))
    np.testing.assert_array_equal(body_hash, np.tile(want_h, (4, 1)))


def test_sort_knob_off_gives_identical_results(gpu_lib, mixed, cs):
    raws, want_v, want_h = mixed
    with _native.knob_env(OURO_BLOCK_SORT="0"):
        verdict, status, body_hash = B.verify_block_integrity_cbor(raws, BC.SPKP)
        cv, cst, ch = B.verify_block_integrity_cbor(cs["triple"], BC.SPKP)
    assert (status == B.PACK_OK).all()
    np.testing.assert_array_equal(verdict, want_v)
    np.testing.assert_array_equal(body_hash, want_h)
    np.testing.assert_array_equal(cv, cs["verdict"])
    np.testing.assert_array_equal(cst, cs["status"])
    np.testing.assert_array_equal(ch, cs["body_hash"])


def test_device_resident_form(gpu_lib, cs):
    """Blocks in device memory, spans padded apart, one span past the end
    (OURO_PACK_ESPAN, verdict 0): equal to the host-buffer form."""
    import torch

    raws = cs["raws"]
    parts, off, ln, at = [], [], [], 0
    for k, r in enumerate(raws):
        pad = bytes(k % 7)
        parts += [pad, r]
        off.append(at + len(pad))
        ln.append(len(r))
        at += len(pad) + len(r)
    buf = b"".join(parts)
    off.append(len(buf) - 3)
    ln.append(10)
    n = len(off)
    dev = torch.device("cuda", 0)
    d_raw = torch.tensor(np.frombuffer(buf, np.uint8).copy(), device=dev)
    d_off = torch.tensor(np.array(off, np.int64), device=dev)
    d_len = torch.tensor(np.array(ln, np.int32), device=dev)
    nb = int(gpu_lib.ouro_block_pack_bytes(n))
    arena = torch.zeros(nb, dtype=torch.uint8, device=dev)
    status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    verdict = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    body_hash = torch.full((n, 32), 5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    rc = gpu_lib.ouro_block_integrity_verify_cbor_device(
        ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), len(buf), d_off.data_ptr(),
        d_len.data_ptr(), n, BC.SPKP, arena.data_ptr(), nb, status.data_ptr(),
        verdict.data_ptr(), body_hash.data_ptr())
    _native.check(rc, "ouro_block_integrity_verify_cbor_device")
    torch.cuda.synchronize()
    hv, hs, hh = B.verify_block_integrity_cbor(raws, BC.SPKP)
    np.testing.assert_array_equal(verdict.cpu().numpy()[:-1], hv)
    np.testing.assert_array_equal(status.cpu().numpy()[:-1], hs)
    np.testing.assert_array_equal(body_hash.cpu().numpy()[:-1], hh)
    np.testing.assert_array_equal(hv, cs["verdict"])
    np.testing.assert_array_equal(hh, cs["body_hash"])
    assert status[-1].item() == B.PACK_ESPAN and verdict[-1].item() == 0
    assert not body_hash[-1].any().item()
    # a short arena, a misaligned buffer: errors, nothing launched
    assert gpu_lib.ouro_block_integrity_verify_cbor_device(
        None, d_raw.data_ptr(), len(buf), d_off.data_ptr(), d_len.data_ptr(), n, BC.SPKP,
        arena.data_ptr(), nb - 1, status.data_ptr(), verdict.data_ptr(), None) == _native.OURO_EINVAL
    assert gpu_lib.ouro_block_integrity_verify_cbor_device(
        None, d_raw.data_ptr() + 1, len(buf) - 1, d_off.data_ptr(), d_len.data_ptr(), n, BC.SPKP,
        arena.data_ptr(), nb, status.data_ptr(), verdict.data_ptr(), None) == _native.OURO_EINVAL


def test_blake2b_batch_lengths_and_alignments(gpu_lib):
    buf, off, ln = BC.hash_spans()
    want = BC.hash_expect(buf, off, ln)
    np.testing.assert_array_equal(B.blake2b256_batch((buf, off, ln)), want)
    with _native.knob_env(OURO_BLOCK_SORT="0"):
        np.testing.assert_array_equal(B.blake2b256_batch((buf, off, ln)), want)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_blake2b_batch_counts(gpu_lib, n):
    rng = np.random.default_rng(100 + n)
    msgs = [rng.bytes(int(rng.integers(0, 700))) for _ in range(n)]
    got = B.blake2b256_batch(msgs)
    for g, m in zip(got, msgs):
        assert g.tobytes() == hashlib.blake2b(m, digest_size=32).digest()


def test_blake2b_device_resident(gpu_lib):
    """ouro_blake2b256_batch_device: the CPU test's spans plus 257 random ones
    and one outside the buffer (a zero digest, nothing read)."""
    import torch

    buf, off, ln = BC.hash_spans()
    rng = np.random.default_rng(8)
    off = np.concatenate([off, rng.integers(0, 70000, 257).astype(np.uint64)])
    ln = np.concatenate([ln, rng.integers(0, 3000, 257).astype(np.uint32)])
    want = BC.hash_expect(buf, off, ln)
    off = np.concatenate([off, np.array([buf.size - 2], np.uint64)])
    ln = np.concatenate([ln, np.array([3], np.uint32)])
    n = int(off.size)
    dev = torch.device("cuda", 0)
    d_buf = torch.tensor(buf.copy(), device=dev)
    d_off = torch.tensor(off.astype(np.int64), device=dev)
    d_len = torch.tensor(ln.astype(np.int32), device=dev)
    out = torch.full((n, 32), 3, dtype=torch.uint8, device=dev)
    wb = int(gpu_lib.ouro_blake2b256_work_bytes(n))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    rc = gpu_lib.ouro_blake2b256_batch_device(
        ctypes.c_void_p(st.cuda_stream), n, d_buf.data_ptr(), buf.size, d_off.data_ptr(),
        d_len.data_ptr(), out.data_ptr(), work.data_ptr(), wb)
    _native.check(rc, "ouro_blake2b256_batch_device")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:-1], want)
    assert not got[-1].any()
    assert gpu_lib.ouro_blake2b256_batch_device(
        None, n, d_buf.data_ptr(), buf.size, d_off.data_ptr(), d_len.data_ptr(), out.data_ptr(),
        work.data_ptr(), wb - 1) == _native.OURO_EINVAL


@pytest.mark.parametrize("n", [65, 257])
def test_blake2b_device_resident_counts(gpu_lib, n):
    """ouro_blake2b256_batch_device at counts with a partial last workgroup in
    the scatter and the hash kernels, spans at every alignment."""
    import torch

    rng = np.random.default_rng(200 + n)
    buf = np.frombuffer(rng.bytes(40000), np.uint8)
    off = rng.integers(0, 30000, n).astype(np.uint64)
    ln = rng.integers(0, 2000, n).astype(np.uint32)
    ln[::9] = 0
    want = BC.hash_expect(buf, off, ln)
    dev = torch.device("cuda", 0)
    d_buf = torch.tensor(buf.copy(), device=dev)
    d_off = torch.tensor(off.astype(np.int64), device=dev)
    d_len = torch.tensor(ln.astype(np.int32), device=dev)
    out = torch.full((n, 32), 3, dtype=torch.uint8, device=dev)
    wb = int(gpu_lib.ouro_blake2b256_work_bytes(n))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    rc = gpu_lib.ouro_blake2b256_batch_device(
        ctypes.c_void_p(st.cuda_stream), n, d_buf.data_ptr(), buf.size, d_off.data_ptr(),
        d_len.data_ptr(), out.data_ptr(), work.data_ptr(), wb)
    _native.check(rc, "ouro_blake2b256_batch_device")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
