"""The prover's scalar chain on the host build (csrc/prove.h var_mul, through
lib/libouro_devhost_test.so dh_var_mul) against exact-integer curve arithmetic
(lane_vectors.smul): [x]P for x = 2^254, 2^255 - 8, scalars with long runs of
zeros and of ones, and 200 random clamped scalars (reduced mod L first, as the
prover reduces its own, so the chain sees x mod L), and scalars below L with
long zero and one runs that reach the recoding as they are, on Elligator2
outputs and the base point.  No GPU.

The chain is var_mul's 64 four-bit windows; no fixed-scalar chain exists to
compare with it."""
import ctypes
import os

import numpy as np
import pytest

import edge_cases as E
import lane_vectors as LV
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")
B_ENC = bytes([0x58]) + bytes([0x66]) * 31


@pytest.fixture(scope="module")
def dh():
    lib = ctypes.CDLL(SO)
    lib.dh_var_mul.restype = ctypes.c_int
    lib.dh_var_mul.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


def clamp(b: bytes) -> int:
    return (int.from_bytes(b, "little") & ((1 << 255) - 8)) | (1 << 254)


def points():
    """The base point and eight Elligator2 outputs (prime-order: the map
    clears the cofactor), as (encoding, affine point)."""
    rng = np.random.default_rng(254)
    encs = [B_ENC] + [O.elligator2(bytes(r[:31]) + bytes([r[31] & 0x7F]))
                      for r in (rng.bytes(32) for _ in range(8))]
    out = []
    for e in encs:
        ok, _, small, x, y = LV.decode_want(e, False)
        assert ok and not small
        out.append((e, (x, y)))
    return out


def var_mul(dh, k: int, enc: bytes, reduce: bool) -> bytes:
    out = ctypes.create_string_buffer(32)
    assert dh.dh_var_mul(out, k.to_bytes(32, "little"), enc, 1 if reduce else 0) == 0
    return out.raw


def directed():
    ones = (1 << 254) | (((1 << 120) - 1) << 60)         # a run of 120 ones
    return [1 << 254, (1 << 255) - 8,
            (1 << 254) | 8,                              # 250 zeros below the top bit
            (1 << 254) | (1 << 131),                     # zero runs on both sides of one bit
            ones, (1 << 254) | ((1 << 200) - 8),         # 197 ones
            clamp(bytes([0x88]) * 32), clamp(bytes([0x77]) * 32), clamp(bytes([0xF0]) * 32)]


def test_clamped_scalars_against_exact_integers(dh):
    rng = np.random.default_rng(255)
    pts = points()
    xs = directed() + [clamp(rng.bytes(32)) for _ in range(200)]
    for j, x in enumerate(xs):
        assert x >> 254 == 1 and x % 8 == 0
        # every directed scalar on every point; the random ones on two points each
        for enc, pt in (pts if j < len(directed()) else (pts[0], pts[1 + j % 8])):
            assert var_mul(dh, x, enc, True) == E.enc_pt(LV.smul(x, pt)), (j, enc.hex())


def test_scalars_below_the_group_order_unreduced(dh):
    """What the prover passes for the nonce: any k < L, edge values included."""
    rng = np.random.default_rng(256)
    pts = points()
    ks = [0, 1, 2, 8, 15, 16, LV.L - 1, LV.L - 2, 1 << 252, (1 << 252) - 1, 1 << 128,
          (1 << 128) - 1]
    # long runs that reach the recoding as they are (no reduction comes first):
    # zeros between two bits, runs of ones (every digit 15 with its carry
    # chain), 0x8 and 0x7 digits (the recoding's sign boundary), alternating runs
    runs = [(1 << 251) | 1, (1 << 251) | (1 << 120), (1 << 252) | 8, (1 << 251) - 1,
            ((1 << 200) - 1) << 40, ((1 << 120) - 1) << 60, (1 << 252) - (1 << 130),
            int("8" * 62, 16), int("7" * 63, 16), int("f0" * 31, 16), int("0f" * 31, 16),
            int("f" * 20 + "0" * 20 + "f" * 20, 16), int("1" + "0" * 30 + "f" * 31, 16)]
    assert all(0 < k < LV.L for k in runs)
    ks += runs + [int.from_bytes(rng.bytes(40), "little") % LV.L for _ in range(40)]
    for j, k in enumerate(ks):
        # the directed values on two points (the base point among them), the rest on one
        for enc, pt in ([pts[0], pts[1 + j % 8]] if j < 12 + len(runs) else [pts[j % len(pts)]]):
            assert var_mul(dh, k, enc, False) == E.enc_pt(LV.smul(k, pt)), j


def test_a_point_that_does_not_decode_is_refused(dh):
    out = ctypes.create_string_buffer(32)
    assert dh.dh_var_mul(out, bytes(32), LV.NO_DECODE, 0) == -1
