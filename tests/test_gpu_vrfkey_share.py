"""One fixed-base table of -Y per distinct VRF key (kernels.hip k_vrfkey_group
/ k_vrfkey_base / k_vrfkey_fill, verify.h vrf_u_fixed_lane): header batches
whose headers repeat a pool's vrf_vk give, bit for bit, the verdicts and
outputs of the per-header doubling chains -- the oracle's -- for forged and
near-duplicate keys, at odd shapes, on both sides of every switch between the
shared and the inline U cores, and through the host-buffer path.

Headers come from bench.synth_headers: header i belongs to pool i % npools and
carries that pool's VRF key, so an untouched batch has npools distinct keys.
Each batch and its default-path results are computed once per module.
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def _params():
    """(R, bytes per key) as compiled: the headers per distinct key below which
    no tables are built (csrc/vrfkey_ws.h) and a key's table and base points,
    read from the host lane build.  (torch first: its HIP runtime has to be
    the one the process loads, see _native.load.)"""
    import torch  # noqa: F401

    lib = ctypes.CDLL(os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so"))
    w, nw, ne = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tw, bw, r = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    lib.dh_vrfkey_params(*(ctypes.byref(x) for x in (w, nw, ne, tw, bw, r)))
    return r.value, 4 * (tw.value + bw.value)


SMALL_ORDER = bytes([1] + [0] * 31)                       # the identity
NON_CANONICAL = bytes([0xff] * 31 + [0x7f])               # y = 2^255 - 1 >= p
NO_DECODE = bytes([2] + [0] * 31)                         # y = 2: (y^2 - 1)/(d y^2 + 1) is no square


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    return bench


def _dev():
    import torch

    return torch.device("cuda:0")


def _launch(t, n):
    """The device entry on batch t: (verdict, beta_eta, beta_leader, K, shared)."""
    import torch

    from ouroboros_network_amd import _native

    hdr = _bench().DeviceHeaders(t, n, _dev())
    st = torch.cuda.current_stream()
    hdr.launch(st)
    shared = ctypes.c_int(-1)
    k = _native.load().ouro_debug_last_vrfkey_groups(ctypes.c_void_p(st.cuda_stream),
                                                     ctypes.byref(shared))
    torch.cuda.synchronize()
    return (hdr.verdict.cpu().numpy(), hdr.beta_eta.cpu().numpy().reshape(n, 64),
            hdr.beta_leader.cpu().numpy().reshape(n, 64), k, shared.value)


def _host(t, n):
    return _bench().DeviceHeaders(t, n, _dev()).host_sample(n)


def _assert_oracle(t, n, got):
    wv, wbe, wbl = O.tpraos_verify_batch(_host(t, n), threads=THREADS)
    np.testing.assert_array_equal(got[0], wv)
    np.testing.assert_array_equal(got[1], wbe)
    np.testing.assert_array_equal(got[2], wbl)
    return wv


@functools.lru_cache(maxsize=None)
def _plain(n, npools):
    t, _ = _bench().synth_headers(n, npools, _dev())
    return t


@functools.lru_cache(maxsize=None)
def _default(n, npools):
    t = _plain(n, npools)
    return t, _launch(t, n)


def test_basic_shared_case():
    from ouroboros_network_amd import _native

    n, npools = 2048, 4
    t, got = _default(n, npools)
    assert (got[3], got[4]) == (npools, 1)
    assert (_assert_oracle(t, n, got) == 15).all()
    with _native.knob_env(OURO_VRFKEY_SHARE="0"):
        off = _launch(t, n)
    assert (off[3], off[4]) == (0, 0)
    for g, w in zip(off[:3], got[:3]):
        np.testing.assert_array_equal(g, w)


def test_node_configuration():
    """Seeds derived on the device, claimed outputs and the epoch nonce."""
    n, npools = 2048, 4
    t, _, pool = _bench().synth_headers(n, npools, _dev(), keep_pool=True)
    _bench().synth_node_config(t, n, npools, pool, bytes(range(7, 39)), _dev())
    got = _launch(t, n)
    assert (got[3], got[4]) == (npools, 1)
    assert (_assert_oracle(t, n, got) == 0x3f).all()


def test_forged_and_near_duplicate_keys():
    """40 seeded rows get one byte of vrf_vk incremented (the first 8 as 4
    pairs of one pool with the same byte: identical corrupted keys); three
    more rows each get a small-order key, ff..ff7f and a key that does not
    decode.  Every such header fails both VRFs with zeroed outputs."""
    import torch

    n, npools, per = 2048, 4, 40
    t, _ = _bench().synth_headers(n, npools, _dev())
    rng = np.random.default_rng(20261019)
    q = rng.permutation(n // npools)[: per + 9]
    pools = rng.integers(0, npools, per)
    cols = rng.integers(0, 32, per)
    for j in range(0, 8, 2):
        pools[j + 1], cols[j + 1] = pools[j], cols[j]
    rows = q[:per] * npools + pools
    view = t["vrf_vk"].view(n, 32)
    view[torch.from_numpy(rows).to(_dev()), torch.from_numpy(cols).to(_dev())] += 1
    special = q[per:] * npools
    for k, enc in enumerate((SMALL_ORDER, NON_CANONICAL, NO_DECODE)):
        for r in special[3 * k:3 * k + 3]:
            view[int(r)] = torch.frombuffer(bytearray(enc), dtype=torch.uint8).to(_dev())
    got = _launch(t, n)
    keys = view.cpu().numpy()
    distinct = len(np.unique(keys, axis=0))
    # the 4 forced pairs at least share a corrupted key (4 pools x 32 columns:
    # more rows collide by chance); every touched row is a forgery
    assert npools + 3 < distinct <= npools + 3 + per - 4
    assert (got[3], got[4]) == (distinct, 1)
    wv = _assert_oracle(t, n, got)
    bad = np.concatenate([rows, special])
    assert ((wv[bad] & 0x0c) == 0).all() and (np.delete(wv, bad) == 15).all()
    assert not got[1][bad].any() and not got[2][bad].any()


# n = 1: below R headers per key, no tables; 65 headers of one pool; 1,000 of
# 7: neither a multiple of the wave nor of the pool count
@pytest.mark.parametrize("n,npools,shared", [(1, 1, 0), (65, 1, 1), (1000, 7, 1)],
                         ids=["n1", "n65", "n1000"])
def test_shapes(n, npools, shared):
    t, got = _default(n, npools)
    assert got[4] == shared
    assert got[3] == (npools if n >= _params()[0] else 0)
    assert (_assert_oracle(t, n, got) == 15).all()


# kmax = n // R = 8 at n = 143: 8 keys share, 9 run the inline cores
@pytest.mark.parametrize("npools,shared", [(8, 1), (9, 0)], ids=["at_kmax", "above_kmax"])
def test_both_sides_of_the_ratio(npools, shared):
    R = _params()[0]
    n = 9 * R - 1
    assert n // R == 8
    t, got = _default(n, npools)
    assert (got[3], got[4]) == (npools, shared)
    assert (_assert_oracle(t, n, got) == 15).all()


def test_budget_below_one_key():
    """OURO_VRFKEY_TAB_MB=0: not one key's table fits, so nothing is grouped
    and the inline cores run; the results are the shared path's."""
    from ouroboros_network_amd import _native

    n, npools = 2048, 4
    t, want = _default(n, npools)
    with _native.knob_env(OURO_VRFKEY_TAB_MB="0"):
        got = _launch(t, n)
    assert (got[3], got[4]) == (0, 0)
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)


def test_budget_below_the_keys():
    """A 1 MB budget holds 11 keys of 90,752 bytes (width 6): that many pools
    share, one more does not."""
    from ouroboros_network_amd import _native

    R, key_bytes = _params()
    n, fit = 2048, (1 << 20) // key_bytes
    assert 1 <= fit < n // R - 1
    with _native.knob_env(OURO_VRFKEY_TAB_MB="1"):
        for npools, shared in ((fit, 1), (fit + 1, 0)):
            t = _plain(n, npools)
            got = _launch(t, n)
            assert (got[3], got[4]) == (npools, shared)
            assert (_assert_oracle(t, n, got) == 15).all()


def test_host_buffer_entry_in_chunks():
    """verify_headers from host memory in three chunks (grouping is per chunk)."""
    from ouroboros_network_amd import _native
    from ouroboros_network_amd.tpraos import verify_headers

    n, npools = 2048, 4
    t, want = _default(n, npools)
    with _native.knob_env(OURO_HOST_CHUNK="768"):
        hv, hbe, hbl = verify_headers(_host(t, n))
    np.testing.assert_array_equal(hv, want[0])
    np.testing.assert_array_equal(hbe, want[1])
    np.testing.assert_array_equal(hbl, want[2])


@pytest.mark.hooks
def test_probe_chains_and_the_probe_cap():
    """The test build's OURO_TEST_OCERT_HASH_BITS=2 leaves four adjacent start
    slots.  48 distinct keys then form one run of occupied slots shorter than
    the probe cap of 64: long probe chains, every key found, K = 48 and the
    tables shared.  128 keys make the run longer than the cap, so headers
    whose key lies beyond it give up and represent themselves (K above 128);
    which U cores then run follows from K against kmax = n // R.  The results
    are the oracle's in both."""
    from ouroboros_network_amd import _native

    with _native.knob_env(OURO_TEST_OCERT_HASH_BITS="2"):
        n, npools = 1536, 48
        t = _plain(n, npools)
        got = _launch(t, n)
        assert (got[3], got[4]) == (npools, 1)
        assert (_assert_oracle(t, n, got) == 15).all()
        n, npools = 4096, 128
        t = _plain(n, npools)
        got = _launch(t, n)
        assert npools < got[3] <= n
        assert got[4] == (1 if got[3] <= n // _params()[0] else 0)
        assert (_assert_oracle(t, n, got) == 15).all()


def test_probe_cap_on_the_test_build(gpu_lib):
    """Runs the hook test above in a child process on the test build."""
    from ouroboros_network_amd import _native

    assert os.path.exists(_native.TEST_LIB_PATH), "build lib/libouro_verify_test.so (make)"
    env = dict(os.environ)
    env["OURO_VERIFY_LIB"] = _native.TEST_LIB_PATH
    r = subprocess.run(
        [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
         "--timeout", "300", "--timeout-method", "thread", "-m", "gpu and hooks",
         os.path.abspath(__file__)],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ passed", ln)]
    assert summary and int(re.search(r"(\d+) passed", summary[-1]).group(1)) == 1, tail
    assert not re.search(r"\d+ skipped", summary[-1]), tail
