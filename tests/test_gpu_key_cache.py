"""The key directories a stream keeps from one header launch to the next
(csrc/key_cache.h, kernels.hip k_kc_begin ...; OURO_KEY_CACHE): a pool's VRF
key table is built, and its certificate verified, by the first launch that
carries them and found again by the later ones.  Every launch here is compared
with the oracle bit for bit, and the counts come from ouro_debug_key_cache:
(VRF keys resident, built by the last launch, times emptied; the same three
for certificates; the generation).

Headers come from bench.synth_headers: header i belongs to pool i % npools,
and a pool's keys depend on its number alone, so pools 0-3 of an 8-pool batch
are the pools of a 4-pool batch.  All launches run on the current stream; each
test starts from empty directories (a knob reload empties them).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, os.cpu_count() or 1)
ALL_STREAMS = ctypes.c_void_p(-1)

SMALL_ORDER = bytes([1] + [0] * 31)                       # the identity
NON_CANONICAL = bytes([0xff] * 31 + [0x7f])               # y = 2^255 - 1 >= p
NO_DECODE = bytes([2] + [0] * 31)                         # y = 2: no square root


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    return bench


def _dev():
    import torch

    return torch.device("cuda:0")


def _stats(stream=None):
    import torch

    from ouroboros_network_amd import _native

    out = (ctypes.c_uint64 * 8)()
    st = stream if stream is not None else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _native.load().ouro_debug_key_cache(st, out) == 0
    return list(out)


def _launch(t, n):
    """The device entry on batch t: (verdict, beta_eta, beta_leader, K, shared,
    certificates, the directories' counts)."""
    import torch

    from ouroboros_network_amd import _native

    hdr = _bench().DeviceHeaders(t, n, _dev())
    st = torch.cuda.current_stream()
    hdr.launch(st)
    lib = _native.load()
    shared = ctypes.c_int(-1)
    k = lib.ouro_debug_last_vrfkey_groups(ctypes.c_void_p(st.cuda_stream), ctypes.byref(shared))
    c = lib.ouro_debug_last_ocert_groups(ctypes.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    return (hdr.verdict.cpu().numpy(), hdr.beta_eta.cpu().numpy().reshape(n, 64),
            hdr.beta_leader.cpu().numpy().reshape(n, 64), k, shared.value, c, _stats())


@functools.lru_cache(maxsize=None)
def _plain(n, npools):
    t, _ = _bench().synth_headers(n, npools, _dev())
    return t


def _copy(t):
    return {k: v.clone() for k, v in t.items()}


_ORACLE = {}


def _oracle(t, n, key=None):
    """The oracle's (verdict, beta_eta, beta_leader) of batch t; computed once
    per named batch."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    hb = _bench().DeviceHeaders(t, n, _dev()).host_sample(n)
    want = O.tpraos_verify_batch(hb, threads=THREADS)
    if key is not None:
        _ORACLE[key] = want
    return want


def _assert_equal(got, want):
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)


@pytest.fixture(autouse=True)
def _empty_directories():
    from ouroboros_network_amd import _native

    _native.load()
    _native.reload_knobs()
    yield


def _twice(t, n, npools, key, all_bits):
    """Batch t launched twice, then once with OURO_KEY_CACHE=0."""
    from ouroboros_network_amd import _native

    want = _oracle(t, n, key)
    a = _launch(t, n)
    assert (a[3], a[4], a[5]) == (npools, 1, npools)
    assert a[6][:6] == [npools, npools, 0, npools, npools, 0]
    _assert_equal(a, want)
    assert (a[0] == all_bits).all()
    b = _launch(t, n)
    assert (b[3], b[4], b[5]) == (npools, 1, npools)       # this batch's distinct counts
    assert b[6][:6] == [npools, 0, 0, npools, 0, 0]         # nothing built, nothing verified
    assert b[6][6] == a[6][6] + 1
    _assert_equal(b, a)
    with _native.knob_env(OURO_KEY_CACHE="0"):
        for _ in range(2):
            c = _launch(t, n)
            assert (c[3], c[4], c[5]) == (npools, 1, npools)
            assert c[6][:6] == [npools, npools, 0, npools, npools, 0]   # all over again
            _assert_equal(c, a)


def test_same_batch_twice():
    n, npools = 2048, 4
    _twice(_plain(n, npools), n, npools, ("plain", n, npools), 15)


def test_node_configuration_twice():
    """Seeds derived on the device, claimed outputs and the epoch nonce."""
    n, npools = 2048, 4
    t, _, pool = _bench().synth_headers(n, npools, _dev(), keep_pool=True)
    _bench().synth_node_config(t, n, npools, pool, bytes(range(7, 39)), _dev())
    _twice(t, n, npools, None, 0x3f)


def test_old_and_new_pools():
    """Pools 0-3 already there, 4-7 new: exactly four keys built."""
    n = 2048
    t4, t8 = _plain(n, 4), _plain(n, 8)
    k4, k8 = (x["vrf_vk"].view(n, 32).cpu().numpy() for x in (t4, t8))
    assert (k4[:4] == k8[:4]).all() and len(np.unique(k8[:8], axis=0)) == 8   # the premise
    a = _launch(t4, n)
    _assert_equal(a, _oracle(t4, n, ("plain", n, 4)))
    b = _launch(t8, n)
    assert (b[3], b[4], b[5]) == (8, 1, 8)
    assert b[6][:6] == [8, 4, 0, 8, 4, 0]
    _assert_equal(b, _oracle(t8, n, ("plain", n, 8)))
    assert (b[0] == 15).all()
    c = _launch(t4, n)                                     # a batch's own count, not the directory's
    assert (c[3], c[5]) == (4, 4) and c[6][:6] == [8, 0, 0, 8, 0, 0]
    _assert_equal(c, a)


def test_batch_sizes_change_on_a_warm_stream():
    """1,100, 2,000, 600 and 2,000 headers of the same four pools, one after
    the other with nothing reloaded in between.  The per-call buffers grow at
    the second launch while the grouping table keeps its capacity (4,096
    entries for 1,100 and for 2,000 headers), shrink in use at the third and
    are back at the fourth; the key tables' layout grows once (kmax 68 ->
    125), which empties the VRF directory, and the certificates stay."""
    npools = 4
    built = []
    for n in (1100, 2000, 600, 2000):
        t = _plain(n, npools)
        got = _launch(t, n)
        assert (got[3], got[4], got[5]) == (npools, 1, npools)
        _assert_equal(got, _oracle(t, n, ("plain", n, npools)))
        assert (got[0] == 15).all()
        assert got[6][0] == got[6][3] == npools and got[6][2] == got[6][5] == 0
        built.append((got[6][1], got[6][4]))
    assert built == [(4, 4), (4, 0), (0, 0), (0, 0)]


def test_certificate_variants_of_a_cached_pool():
    """Two headers of pool 1 carry variants of its cached certificate: one
    sigma bit flipped, the counter changed.  Only they lose bit 0x01."""
    import torch

    n, npools = 2048, 4
    t0 = _plain(n, npools)
    _launch(t0, n)                                         # the four certificates cached
    t = _copy(t0)
    r_sig, r_ctr = 4 * 100 + 1, 4 * 300 + 1
    t["ocert_sigma"].view(n, 64)[r_sig, 17] ^= 0x04
    t["ocert_counter"].view(n, 8)[r_ctr, 0] += 1
    torch.cuda.synchronize()
    want = _oracle(t, n)
    expect = np.full(n, 15, np.uint8)
    expect[[r_sig, r_ctr]] = 14
    np.testing.assert_array_equal(want[0], expect)
    a = _launch(t, n)
    assert a[5] == npools + 2 and a[6][3:6] == [npools + 2, 2, 0]
    _assert_equal(a, want)
    b = _launch(t, n)                                      # the rejected variants cached too
    assert b[5] == npools + 2 and b[6][3:6] == [npools + 2, 0, 0]
    _assert_equal(b, want)


def test_bad_keys_cached():
    """Small-order, non-canonical and undecodable VRF keys (tests/edge_cases.py)
    get a directory slot like any key; their flag rejects them on every
    launch."""
    import torch

    import edge_cases as E

    encs = list(dict.fromkeys(E.small_order_encodings() + [NON_CANONICAL, NO_DECODE,
                                                           E.enc_int(E.non_square_y())]))
    n, npools = 2048, 4
    t = _copy(_plain(n, npools))
    view = t["vrf_vk"].view(n, 32)
    rows = []
    for k, enc in enumerate(encs):
        for r in (4 * (10 + 3 * k), 4 * (200 + 3 * k) + 2):    # each twice, in two pools' rows
            view[r] = torch.frombuffer(bytearray(enc), dtype=torch.uint8).to(_dev())
            rows.append(r)
    torch.cuda.synchronize()
    want = _oracle(t, n)
    assert ((want[0][rows] & 0x0c) == 0).all() and (np.delete(want[0], rows) == 15).all()
    distinct = npools + len(encs)
    a = _launch(t, n)
    assert (a[3], a[4]) == (distinct, 1) and a[6][:3] == [distinct, distinct, 0]
    _assert_equal(a, want)
    b = _launch(t, n)
    assert (b[3], b[4]) == (distinct, 1) and b[6][:3] == [distinct, 0, 0]
    _assert_equal(b, want)
    assert not b[1][rows].any() and not b[2][rows].any()


def test_directory_emptied_when_new_keys_do_not_fit():
    """The smallest budget the knob can express, 1 MB, holds 11 keys at width
    6.  Batches of 8 keys, then 8 other keys, then the first 8 again: each
    fits alone, none beside the one before, so every launch shares and every
    launch after the first empties the directory."""
    import torch

    from ouroboros_network_amd import _native

    lib = ctypes.CDLL(os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so"))
    w, nw, ne = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tw, bw, r = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    lib.dh_vrfkey_params(*(ctypes.byref(x) for x in (w, nw, ne, tw, bw, r)))
    fit = (1 << 20) // (4 * (tw.value + bw.value))
    n = 2048
    npools = fit - 3
    assert 2 <= npools <= fit < 2 * npools and fit <= n // r.value
    ta = _plain(n, npools)
    tb = _copy(ta)
    tb["vrf_vk"].view(n, 32)[:, 5] += 1                    # other keys (every header a forgery)
    torch.cuda.synchronize()
    wa, wb = _oracle(ta, n, ("plain", n, npools)), _oracle(tb, n)
    assert (wa[0] == 15).all() and ((wb[0] & 0x0c) == 0).all()
    with _native.knob_env(OURO_VRFKEY_TAB_MB="1"):
        for step, (t, want) in enumerate(((ta, wa), (tb, wb), (ta, wa), (ta, wa))):
            got = _launch(t, n)
            assert (got[3], got[4]) == (npools, 1)
            emptied = min(step, 2)
            assert got[6][:3] == [npools, npools if step < 3 else 0, emptied]
            _assert_equal(got, want)


@pytest.mark.parametrize("n,npools,shared", [(1, 1, 0), (65, 1, 1)], ids=["n1", "n65"])
def test_shapes(n, npools, shared):
    """One header: below the headers per key at which tables are built, so no
    VRF grouping; its certificate is cached.  65 headers of one pool."""
    t = _plain(n, npools)
    want = _oracle(t, n, ("plain", n, npools))
    for step in range(2):
        got = _launch(t, n)
        assert got[4] == shared and got[3] == (npools if shared else 0) and got[5] == npools
        built = npools if step == 0 else 0
        assert got[6][:6] == [npools if shared else 0, built if shared else 0, 0, npools, built, 0]
        _assert_equal(got, want)
        assert (got[0] == 15).all()


def test_host_buffer_entry_in_chunks():
    """verify_headers from host memory in chunks of 512 on the library's own
    streams: the chunks after a stream's first find every key there."""
    from ouroboros_network_amd import _native
    from ouroboros_network_amd.tpraos import verify_headers

    n, npools = 2048, 4
    t = _plain(n, npools)
    want = _oracle(t, n, ("plain", n, npools))
    hb = _bench().DeviceHeaders(t, n, _dev()).host_sample(n)
    with _native.knob_env(OURO_HOST_CHUNK="512"):
        got = verify_headers(hb)
        s = _stats(ALL_STREAMS)
    _assert_equal(got, want)
    streams = s[0] // npools
    assert 1 <= streams <= 2 and s[0] == s[3] == npools * streams   # each stream built once
    assert s[1] == s[4] == 0                              # every stream's last chunk built nothing
    assert s[2] == s[5] == 0 and s[6] >= 2
