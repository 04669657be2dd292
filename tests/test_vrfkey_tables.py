"""The per-key VRF tables on the host build of the kernels' routines
(csrc/verify.h vrfkey_base / vrfkey_fill / vrf_u_fixed_lane, tpraos.h
hdr_u_shared; exported by csrc/devhost_vrfkey.hip): U = [s]B - [c]Y from the
key's fixed-base table -- additions only -- is the point dsm_lane's doubling
chain gives, as an encoding, for random and directed c; the key flag is false
for small-order, non-canonical and undecodable keys, whose tables still build
within the limb bounds; and the workspace arithmetic of the launch
(csrc/vrfkey_ws.h) is consistent.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from lane_vectors import NON_CANONICAL, NO_DECODE, SMALL_ORDER
from lane_vectors import directed as _directed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")
L = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19


class Lib:
    def __init__(self):
        if not os.path.exists(SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "ouroboros-network_amd"),
                            "lib/libouro_devhost_test.so"], check=True, stdout=subprocess.DEVNULL)
        self.lib = lib = ctypes.CDLL(SO)
        lib.dh_bound_violations.restype = ctypes.c_ulonglong
        lib.dh_vrfkey_layout.restype = ctypes.c_size_t
        lib.dh_vrfkey_layout.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        w, nw, ne = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        tw, bw, r = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        lib.dh_vrfkey_params(*(ctypes.byref(x) for x in (w, nw, ne, tw, bw, r)))
        self.width, self.windows, self.entries = w.value, nw.value, ne.value
        self.tab_words, self.base_words, self.min_per_key = tw.value, bw.value, r.value

    def build(self, pk):
        tab = np.zeros(self.tab_words, np.int32)
        base = np.zeros(self.base_words, np.int32)
        flag = self.lib.dh_vrfkey_build(pk, tab.ctypes.data_as(ctypes.c_void_p),
                                        base.ctypes.data_as(ctypes.c_void_p))
        return flag, tab

    def u_table(self, tab, c, s):
        out = ctypes.create_string_buffer(32)
        self.lib.dh_vrfkey_u(out, tab.ctypes.data_as(ctypes.c_void_p), c.to_bytes(16, "little"),
                             s.to_bytes(32, "little"))
        return out.raw

    def u_inline(self, pk, c, s):
        out = ctypes.create_string_buffer(32)
        flag = self.lib.dh_vrfkey_u_inline(out, pk, c.to_bytes(16, "little"),
                                           s.to_bytes(32, "little"))
        return flag, out.raw


@pytest.fixture(scope="module")
def dh():
    return Lib()


def _valid_keys(dh, rng, count):
    keys = []
    while len(keys) < count:
        pk = rng.bytes(32)
        if dh.u_inline(pk, 1, 1)[0]:
            keys.append(pk)
    return keys


def test_table_shape(dh):
    assert 4 <= dh.width <= 8
    assert dh.windows == (128 + dh.width) // dh.width
    top = (1 << (128 - dh.width * (dh.windows - 1)))
    assert dh.entries == (dh.windows - 1) * (1 << (dh.width - 1)) + top
    assert dh.tab_words == 32 * dh.entries


def test_u_from_the_table_is_the_chain_s_u(dh):
    rng = np.random.default_rng(20261019)
    for pk in _valid_keys(dh, rng, 3):
        flag, tab = dh.build(pk)
        assert flag == 1
        cs = _directed(dh.width) + [int.from_bytes(rng.bytes(16), "little") for _ in range(12)]
        for c in cs:
            for s in (int.from_bytes(rng.bytes(32), "little") % L, 0, L - 1):
                want_flag, want = dh.u_inline(pk, c, s)
                assert want_flag == 1
                assert dh.u_table(tab, c, s) == want, (pk.hex(), hex(c), hex(s))
    assert dh.lib.dh_bound_violations() == 0


@pytest.mark.parametrize("k", range(len(SMALL_ORDER)))
def test_small_order_keys(dh, k):
    """Flag false; these are points of the curve, so the table is a table of
    multiples and U still equals the chain's."""
    pk = SMALL_ORDER[k]
    flag, tab = dh.build(pk)
    assert flag == 0
    c, s = 0x0123456789abcdef0fedcba987654321, L - 2
    want_flag, want = dh.u_inline(pk, c, s)
    assert want_flag == 0
    assert dh.u_table(tab, c, s) == want
    assert dh.lib.dh_bound_violations() == 0


@pytest.mark.parametrize("pk", [NON_CANONICAL, NO_DECODE], ids=["non_canonical", "no_decode"])
def test_keys_that_fail_the_checks(dh, pk):
    """Flag false, as the inline core's; the build and a chain over its table
    stay within the limb bounds and write every entry."""
    flag, tab = dh.build(pk)
    assert flag == 0 and dh.u_inline(pk, 5, 7)[0] == 0
    assert tab.reshape(-1, 32).any(axis=1).all()
    dh.u_table(tab, (1 << 128) - 1, L - 1)
    assert dh.lib.dh_bound_violations() == 0


def test_workspace_layout(dh):
    key_bytes = 4 * (dh.tab_words + dh.base_words)
    out = (ctypes.c_size_t * 7)()
    for n, budget in [(1, 1 << 30), (dh.min_per_key, 1 << 30), (1000, 1 << 30), (1 << 20, 512 << 20),
                      (2048, key_bytes - 1), (2048, 3 * key_bytes), ((1 << 30) + 1, 1 << 30)]:
        table_bytes = dh.lib.dh_vrfkey_layout(n, budget, out)
        kmax, cap, off_rep, off_uniq, off_kidx, off_flag, group_bytes = list(out)
        want = 0 if n > 1 << 30 else min(n // dh.min_per_key, budget // key_bytes)
        assert kmax == want and table_bytes == kmax * key_bytes <= budget
        if not kmax:
            continue
        assert cap >= 2 * n and cap & (cap - 1) == 0 and cap < 1 << 32
        assert off_rep == 80 + 4 * cap and off_uniq == off_rep + 4 * n
        assert off_kidx == off_uniq + 4 * n and off_flag == off_kidx + 4 * n
        assert off_flag + kmax <= group_bytes and group_bytes % 16 == 0
