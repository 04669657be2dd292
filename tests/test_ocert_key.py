"""The key of the shared OCERT checks (csrc/tpraos.h ocert_key_hash /
ocert_key_equal, run by kernels.hip k_ocert_group), on the host build of the
kernels' routines: two headers may share one Ed25519 verification only if
their 144 bytes issuer_vk || hot_vk || ocert_counter || ocert_kes_period ||
ocert_sigma are all equal -- every bit of them counts and nothing else does.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ouroboros_network_amd.tpraos import HeaderBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")

# (member, bytes per row) of the key, in its byte order
KEY = [("issuer_vk", 32), ("hot_vk", 32), ("ocert_counter", 8), ("ocert_kes_period", 8),
       ("ocert_sigma", 64)]
OTHER = [("vrf_vk", 32), ("eta_proof", 80), ("leader_proof", 80), ("eta_alpha", 32),
         ("leader_alpha", 32), ("kes_t", 4), ("kes_sig", 448), ("body", 64), ("body_off", 8),
         ("body_len", 4)]
N = 4


@pytest.fixture(scope="module")
def dh():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ouroboros-network_amd"),
                        "lib/libouro_devhost_test.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(SO)
    lib.dh_ocert_key_hash.restype = ctypes.c_ulonglong
    lib.dh_ocert_key_hash.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.dh_ocert_key_equal.restype = ctypes.c_int
    lib.dh_ocert_key_equal.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]
    return lib


def _batch():
    """Four synthesised headers: rows 0 and 1 are twins in the key bytes and
    differ in every other member; rows 2 and 3 have keys of their own."""
    rng = np.random.default_rng(144)
    raw = {name: rng.integers(0, 256, (N, w), dtype=np.uint8) for name, w in KEY + OTHER}
    for name, _ in KEY:
        raw[name][1] = raw[name][0]
    raw["body_off"] = (np.arange(N, dtype=np.uint64) * 64).view(np.uint8).reshape(N, 8)
    raw["body_len"] = np.full(N, 64, np.uint32).view(np.uint8).reshape(N, 4)
    return raw


def _struct(raw):
    u64 = lambda k: raw[k].reshape(-1).view(np.uint64)  # noqa: E731
    u32 = lambda k: raw[k].reshape(-1).view(np.uint32)  # noqa: E731
    hb = HeaderBatch(issuer_vk=raw["issuer_vk"], vrf_vk=raw["vrf_vk"], eta_proof=raw["eta_proof"],
                     leader_proof=raw["leader_proof"], eta_alpha=raw["eta_alpha"],
                     leader_alpha=raw["leader_alpha"], hot_vk=raw["hot_vk"],
                     ocert_counter=u64("ocert_counter"), ocert_kes_period=u64("ocert_kes_period"),
                     ocert_sigma=raw["ocert_sigma"], kes_t=u32("kes_t"), kes_sig=raw["kes_sig"],
                     body=raw["body"].reshape(-1), body_off=u64("body_off"),
                     body_len=u32("body_len"))
    return hb, hb.c_struct()


def _equal(dh, raw, i, j):
    hb, s = _struct(raw)
    return bool(dh.dh_ocert_key_equal(ctypes.addressof(s), i, j))


def _hash(dh, raw, i):
    hb, s = _struct(raw)
    return dh.dh_ocert_key_hash(ctypes.addressof(s), i)


def test_a_header_equals_itself_and_its_twin(dh):
    raw = _batch()
    for i in range(N):
        assert _equal(dh, raw, i, i)
    assert _equal(dh, raw, 0, 1) and _equal(dh, raw, 1, 0)
    assert _hash(dh, raw, 0) == _hash(dh, raw, 1)
    for i, j in ((0, 2), (0, 3), (2, 3), (1, 2)):
        assert not _equal(dh, raw, i, j)
    assert len({_hash(dh, raw, i) for i in (0, 2, 3)}) == 3


def test_every_key_bit_counts(dh):
    """Each of the 144 x 8 key bits of header 1, flipped alone, makes it
    unequal to its twin, header 0 (and equal again when flipped back)."""
    raw = _batch()
    hb, s = _struct(raw)
    arrays = {"issuer_vk": hb.issuer_vk, "hot_vk": hb.hot_vk,
              "ocert_counter": hb.ocert_counter.view(np.uint8).reshape(N, 8),
              "ocert_kes_period": hb.ocert_kes_period.view(np.uint8).reshape(N, 8),
              "ocert_sigma": hb.ocert_sigma}
    h0 = dh.dh_ocert_key_hash(ctypes.addressof(s), 0)
    flipped = differing_hash = 0
    for name, w in KEY:
        a = arrays[name]  # the batch's own rows: the struct points at them
        for byte in range(w):
            for bit in range(8):
                a[1, byte] ^= 1 << bit
                assert not dh.dh_ocert_key_equal(ctypes.addressof(s), 0, 1), (name, byte, bit)
                assert not dh.dh_ocert_key_equal(ctypes.addressof(s), 1, 0), (name, byte, bit)
                differing_hash += dh.dh_ocert_key_hash(ctypes.addressof(s), 1) != h0
                a[1, byte] ^= 1 << bit
                flipped += 1
    assert flipped == 144 * 8
    assert dh.dh_ocert_key_equal(ctypes.addressof(s), 0, 1)
    assert dh.dh_ocert_key_hash(ctypes.addressof(s), 1) == h0
    # not a requirement of correctness, but a mix that ignored a word would
    # put every near-duplicate in one probe chain
    assert differing_hash == flipped


def test_no_other_member_counts(dh):
    """A bit flipped in any member outside the key leaves the twins equal and
    their hashes equal."""
    raw = _batch()
    rng = np.random.default_rng(145)
    want = _hash(dh, raw, 0)
    for name, w in OTHER:
        if name in ("body_off", "body_len"):
            continue  # HeaderBatch checks the spans; the twins' already differ
        for _ in range(8):
            byte, bit = int(rng.integers(0, w)), int(rng.integers(0, 8))
            raw[name][1, byte] ^= 1 << bit
            assert _equal(dh, raw, 0, 1), name
            assert _hash(dh, raw, 1) == want, name
    assert (raw["body_off"][0] != raw["body_off"][1]).any()
