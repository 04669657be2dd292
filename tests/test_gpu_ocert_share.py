"""One OCERT verification per distinct operational certificate (kernels.hip
k_ocert_group / k_ocert_unique*, kernels_lat.hip k_ocert_unique_wide): header
batches whose headers repeat a pool's certificate give, bit for bit, the
verdicts and outputs of a check per header -- the oracle's -- in every form of
the unique pass, for near-duplicate and forged records, with the sharing
switched off, and through the host-buffer path.

Headers come from bench.synth_headers: header i belongs to pool i % npools and
carries that pool's certificate, so an untouched batch has npools distinct
records.  Each batch and its default-path results are computed once per
module and shared by the tests that need them.
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

# (member, row width, verdict bits a one-byte change must clear): the table of
# tests/test_gpu_scale.py restricted to the certificate's members (the hot key
# is the certificate's message and the KES root)
FIELDS = [("issuer_vk", 32, 0x01), ("hot_vk", 32, 0x03), ("ocert_counter", 8, 0x01),
          ("ocert_kes_period", 8, 0x01), ("ocert_sigma", 64, 0x01)]


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    return bench


def _dev():
    import torch

    return torch.device("cuda:0")


def _launch(t, n):
    """The device entry on batch t: (verdict, beta_eta, beta_leader, groups)."""
    import torch

    from ouroboros_network_amd import _native

    hdr = _bench().DeviceHeaders(t, n, _dev())
    st = torch.cuda.current_stream()
    hdr.launch(st)
    groups = _native.load().ouro_debug_last_ocert_groups(ctypes.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    return (hdr.verdict.cpu().numpy(), hdr.beta_eta.cpu().numpy().reshape(n, 64),
            hdr.beta_leader.cpu().numpy().reshape(n, 64), groups)


def _host(t, n):
    return _bench().DeviceHeaders(t, n, _dev()).host_sample(n)


def _assert_oracle(t, n, got, sample=None):
    hb = _host(t, n)
    rows = np.arange(n) if sample is None else sample
    wv, wbe, wbl = O.tpraos_verify_batch(hb.rows(rows), threads=THREADS)
    np.testing.assert_array_equal(got[0][rows], wv)
    np.testing.assert_array_equal(got[1][rows], wbe)
    np.testing.assert_array_equal(got[2][rows], wbl)


def _keys(t, n):
    """The 144 key bytes of every header (host)."""
    return np.concatenate([t[name].view(n, w).cpu().numpy() for name, w, _ in FIELDS], axis=1)


@functools.lru_cache(maxsize=None)
def _plain(n, npools):
    t, _ = _bench().synth_headers(n, npools, _dev())
    return t


@functools.lru_cache(maxsize=None)
def _near_duplicates():
    """n = 2,048 over 4 pools; 40 seeded rows per certificate member get one
    byte incremented in that member alone (sigma untouched when the counter or
    the period changes).  The first 8 rows of each member form 4 pairs of one
    pool with the same byte changed -- identical corrupted records -- and the
    narrow members (8 columns x 4 pools) collide further by chance."""
    import torch

    n, npools, per = 2048, 4, 40
    t, _ = _bench().synth_headers(n, npools, _dev())
    rng = np.random.default_rng(20261019)
    q = rng.permutation(n // npools)[: per * len(FIELDS)]  # distinct rows whatever the pools
    expect = np.full(n, 15, np.uint8)
    touched = []
    for k, (name, w, bit) in enumerate(FIELDS):
        pools = rng.integers(0, npools, per)
        cols = rng.integers(0, w, per)
        for j in range(0, 8, 2):
            pools[j + 1], cols[j + 1] = pools[j], cols[j]
        rows = q[k * per:(k + 1) * per] * npools + pools
        view = t[name].view(n, w)
        view[torch.from_numpy(rows).to(_dev()), torch.from_numpy(cols).to(_dev())] += 1
        expect[rows] = 15 ^ bit
        touched.append(rows)
    return t, n, npools, expect, np.concatenate(touched)


@functools.lru_cache(maxsize=None)
def _default(case):
    """(t, n, results of the default path) of a named case."""
    if case == "near":
        t, n = _near_duplicates()[:2]
    else:
        n, npools = case
        t = _plain(n, npools)
    return t, n, _launch(t, n)


def test_many_duplicates():
    n, npools = 4096, 8
    t, _, got = _default((n, npools))
    assert got[3] == npools
    assert (got[0] == 15).all()
    _assert_oracle(t, n, got)


def test_near_duplicates():
    t, n, npools, expect, touched = _near_duplicates()
    got = _default("near")[2]
    np.testing.assert_array_equal(got[0], expect)
    keys = _keys(t, n)
    distinct = len(np.unique(keys[touched], axis=0))
    assert len(np.unique(keys, axis=0)) == npools + distinct
    # the 4 forced pairs per member at least; every touched row is a forgery
    assert 32 <= distinct <= len(touched) - 4 * len(FIELDS)
    assert got[3] == npools + distinct
    _assert_oracle(t, n, got)


def test_a_pool_with_one_forged_certificate():
    """Every header of pool 3 carries the same corrupted sigma: one record,
    one verification, all of its headers invalid; the other pools untouched."""
    import torch

    n, npools = 1024, 8
    t, _ = _bench().synth_headers(n, npools, _dev())
    rows = torch.arange(3, n, npools, device=_dev())
    t["ocert_sigma"].view(n, 64)[rows, 37] += 1
    got = _launch(t, n)
    expect = np.full(n, 15, np.uint8)
    expect[3::npools] = 14
    np.testing.assert_array_equal(got[0], expect)
    assert got[3] == npools
    _assert_oracle(t, n, got)


# n = 3,000 (no multiple of the 256-lane workgroup): 1,500 distinct records run
# the wave form (at most OURO_WIDE_SMALL_MAX = 2,048), 2,500 the lane form
# (above it, at most kOcertShareMax(3000) = 2,625), 3,000 the inline OCERT core
FORMS = [(3000, 1500), (3000, 2500), (3000, 3000), (1, 1), (65, 3)]


@pytest.mark.parametrize("n,npools", FORMS, ids=["wave", "lane", "inline", "n1", "n65"])
def test_unique_pass_forms(n, npools):
    t, _, got = _default((n, npools))
    assert (got[0] == 15).all()
    if (n, npools) != (3000, 3000):
        assert got[3] == npools
    _assert_oracle(t, n, got)


@pytest.mark.parametrize("case", ["near"] + FORMS, ids=lambda c: str(c).replace(" ", ""))
def test_switch_off(case):
    """OURO_OCERT_SHARE=0: no group or unique pass (groups == 0), and results
    byte-equal to the default's."""
    from ouroboros_network_amd import _native

    t, n, want = _default(case)
    with _native.knob_env(OURO_OCERT_SHARE="0"):
        got = _launch(t, n)
    assert got[3] == 0
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    assert want[3] > 0


def test_host_buffer_path():
    """20,000 headers over 16 pools from pageable host memory through
    verify_headers give the device entry's results (and the oracle's on a
    seeded sample); one header is forged so that a flag is not all ones."""
    from ouroboros_network_amd.tpraos import verify_headers

    n, npools = 20000, 16
    t, _ = _bench().synth_headers(n, npools, _dev())
    t["ocert_sigma"].view(n, 64)[12345, 3] += 1
    got = _launch(t, n)
    assert got[3] == npools + 1
    assert got[0][12345] == 14 and (np.delete(got[0], 12345) == 15).all()
    hv, hbe, hbl = verify_headers(_host(t, n))
    np.testing.assert_array_equal(hv, got[0])
    np.testing.assert_array_equal(hbe, got[1])
    np.testing.assert_array_equal(hbl, got[2])
    sample = np.sort(np.random.default_rng(9).choice(n, 512, replace=False))
    sample[0] = 12345
    _assert_oracle(t, n, got, np.sort(sample))


@pytest.mark.hooks
def test_probe_chains_and_the_probe_cap():
    """The test build's OURO_TEST_OCERT_HASH_BITS=2 leaves four start slots
    for 128 distinct records: one probe chain longer than the cap of 64, so
    some headers give up and represent themselves (groups above 128) -- the
    verdicts are still the oracle's."""
    from ouroboros_network_amd import _native

    n, npools = 1024, 128
    t = _plain(n, npools)
    with _native.knob_env(OURO_TEST_OCERT_HASH_BITS="2"):
        got = _launch(t, n)
    assert got[3] > npools
    assert got[3] <= n
    assert (got[0] == 15).all()
    _assert_oracle(t, n, got)
