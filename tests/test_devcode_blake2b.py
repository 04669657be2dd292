"""The streaming Blake2b-256 lane routine (csrc/blake2b_stream.h), compiled for
the host by hipcc, against hashlib (CPU-only), in the manner of
tests/test_devcode_host.py: the routine the kernels and the host path run,
and the device's dword block loads driven by a loader that checks the load
rule -- every dword read holds at least one byte of the span."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import block_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")
LENGTHS = [0, 2, 3, 4, 5] + BC.SEG_LENGTHS + [130, 131, 132, 383, 384, 385]


@pytest.fixture(scope="module")
def dh():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ouroboros-network_amd"),
                        "lib/libouro_devhost_test.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(SO)
    lib.dh_blake2b256_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.dh_blake2b256_dwords.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.dh_blake2b256_dwords.restype = ctypes.c_int
    lib.dh_blake2b256_96.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def data():
    # 64-byte aligned backing store, so that `align` below is the address's
    a = np.zeros(80000 + 64, np.uint8)
    start = (-a.ctypes.data) % 64
    a[:] = np.frombuffer(np.random.default_rng(1).bytes(a.size), np.uint8)
    return a, start


def b2b(m):
    return hashlib.blake2b(m, digest_size=32).digest()


def test_stream_against_hashlib(dh, data):
    a, start = data
    out = ctypes.create_string_buffer(32)
    for align in range(4):
        for n in LENGTHS:
            at = start + 8 + align
            dh.dh_blake2b256_stream(out, a.ctypes.data + at, n)
            assert out.raw == b2b(a[at:at + n].tobytes()), (align, n)


def test_device_dword_loads_against_hashlib_and_the_load_rule(dh, data):
    a, start = data
    out = ctypes.create_string_buffer(32)
    for align in range(4):
        for n in LENGTHS:
            at = start + 8 + align
            loads = dh.dh_blake2b256_dwords(out, a.ctypes.data + at, n)
            assert loads >= 0, f"a dword outside the span was read (align {align}, len {n})"
            assert out.raw == b2b(a[at:at + n].tobytes()), (align, n)
            # no more than the covering dwords, once per block they touch
            cover = (align + n + 3) // 4 if n else 0
            blocks = max(1, (n + 127) // 128)
            assert cover <= loads <= cover + blocks


def test_ninety_six_bytes_in_one_compression(dh):
    rng = np.random.default_rng(3)
    out = ctypes.create_string_buffer(32)
    for _ in range(20):
        m = rng.bytes(96)
        dh.dh_blake2b256_96(out, m)
        assert out.raw == b2b(m)
