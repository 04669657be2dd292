"""The forging-side kernels on the GPU (csrc/kernels_forge.hip k_vrf03_prove,
k_leader_schedule) through the C ABI: the device prover and the device
schedule against the host path and the oracle byte for byte, over the wave,
workgroup and grid-stride edges; the device verifier judging the device
prover; and the recompute on the host path after a device error, in a fresh
child process on the test build."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forge_cases as FC
from ouroboros_network_amd import PraosVRF, _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 63, 64, 65, 255, 256, 257, 1000]
N_SLOTS = [1, 64, 65, 257, 1500]
SETS = FC.param_sets(257)


@pytest.fixture(scope="module")
def prove_cases():
    """1,000 alphas (the eight lengths at all four alignments of the span) and
    the oracle's proofs of them under one shared key and under per-item keys,
    computed once; a batch of n is their first n."""
    n = max(NS)
    alphas, buf, off, ln = FC.prove_inputs(n)
    combos = {(int(ln[i]), int(off[i]) % 4) for i in range(n)}
    assert combos == {(l, a) for l in FC.ISSUE_LENS for a in range(4)}
    ks = FC.keys()
    sks = [ks[i % len(ks)][1] for i in range(n)]
    shared = FC.pool_key()
    want_shared = [FC.oracle_prove(shared, a) for a in alphas]
    want_each = [FC.oracle_prove(sk, a) for sk, a in zip(sks, alphas)]
    return dict(alphas=alphas, buf=buf, off=off, ln=ln, sks=sks, shared=shared,
                want_shared=want_shared, want_each=want_each)


def _rows(want, n):
    return (np.frombuffer(b"".join(w[0] for w in want[:n]), np.uint8).reshape(n, 80),
            np.frombuffer(b"".join(w[1] for w in want[:n]), np.uint8).reshape(n, 64))


@pytest.mark.parametrize("n", NS)
def test_device_prover_equals_host_and_oracle(gpu_lib, prove_cases, n):
    c = prove_cases
    # (the alpha buffer cut after the n-th span: the last span ends at its last byte)
    end = int(c["off"][n - 1]) + int(c["ln"][n - 1])
    buf = c["buf"][:end].copy()
    for keys, nkeys, want in (([c["shared"]], 1, c["want_shared"]),
                              (c["sks"][:n], n, c["want_each"])):
        rc, proof, beta = FC.prove_raw(n, keys, nkeys, buf, c["off"][:n], c["ln"][:n], host=False)
        assert rc == 0
        wp, wb = _rows(want, n)
        np.testing.assert_array_equal(proof, wp)
        np.testing.assert_array_equal(beta, wb)
        rc, hp, hb = FC.prove_raw(n, keys, nkeys, buf, c["off"][:n], c["ln"][:n], host=True)
        assert rc == 0
        np.testing.assert_array_equal(proof, hp)
        np.testing.assert_array_equal(beta, hb)
    rc, p0, b0 = FC.prove_raw(n, [c["shared"]], 1, buf, c["off"][:n], c["ln"][:n], host=False,
                              want_beta=False)
    assert rc == 0 and not b0.any()
    np.testing.assert_array_equal(p0, _rows(c["want_shared"], n)[0])


@pytest.fixture(scope="module")
def sk():
    return FC.pool_key()


@pytest.mark.parametrize("name", list(SETS))
def test_device_schedule_equals_host_and_restatement(gpu_lib, sk, name):
    ps, n = SETS[name], 257
    rc, cls, gen, beta = FC.sched_raw(sk, ps, n, host=False)
    assert rc == 0
    wcls, wgen, wbeta = FC.restate(sk, ps, n)
    np.testing.assert_array_equal(beta, wbeta)
    np.testing.assert_array_equal(cls, wcls)
    np.testing.assert_array_equal(gen, wgen)
    rc, hcls, hgen, hbeta = FC.sched_raw(sk, ps, n, host=True)
    assert rc == 0
    np.testing.assert_array_equal(cls, hcls)
    np.testing.assert_array_equal(gen, hgen)
    np.testing.assert_array_equal(beta, hbeta)
    if name == "half":
        assert 0 < (cls == 1).sum() < n
    if name == "overlay":
        assert (cls == 2).any() and (cls == 3).any() and (cls < 2).any()


@pytest.fixture(scope="module")
def long_schedule(sk):
    """The restatement of 1,500 slots, once per parameter set used below."""
    return {name: FC.restate(sk, FC.param_sets(1500)[name], 1500) for name in ("half", "overlay")}


@pytest.mark.parametrize("n", N_SLOTS)
@pytest.mark.parametrize("name", ["half", "overlay"])
def test_slot_counts_with_and_without_the_optional_outputs(gpu_lib, sk, long_schedule, name, n):
    ps = FC.param_sets(1500)[name]
    wcls, wgen, wbeta = (a[:n] for a in long_schedule[name])
    for want_gen, want_beta in ((True, True), (False, False), (True, False), (False, True)):
        rc, cls, gen, beta = FC.sched_raw(sk, ps, n, host=False, want_gen=want_gen,
                                          want_beta=want_beta)
        assert rc == 0
        np.testing.assert_array_equal(cls, wcls)
        if want_gen:
            np.testing.assert_array_equal(gen, wgen)
        else:
            assert (gen == 0xEEEEEEEE).all()
        if want_beta:
            np.testing.assert_array_equal(beta, wbeta)
        else:
            assert not beta.any()


def _winners(cls, first_slot):
    return [first_slot + int(i) for i in np.nonzero((cls == 1) | (cls == 2))[0]]


@pytest.mark.parametrize("name", ["half", "neutral", "overlay"])
def test_leader_vrfs_on_the_winners(gpu_lib, sk, name):
    ps = SETS[name]
    rc, cls, _, beta = FC.sched_raw(sk, ps, 257, host=False)
    assert rc == 0
    slots = _winners(cls, ps["first_slot"])
    assert len(slots) > 3
    assert FC.vrfs_raw(sk, ps["eta0"], [], host=False)[0] == 0            # m = 0
    for m in (1, len(slots)):
        got = FC.vrfs_raw(sk, ps["eta0"], slots[:m], host=False)
        FC.check_vrfs(sk, ps["eta0"], slots[:m], got)
        host = FC.vrfs_raw(sk, ps["eta0"], slots[:m], host=True)
        for a, b in zip(got[1:], host[1:]):
            np.testing.assert_array_equal(a, b)
    idx = [s - ps["first_slot"] for s in slots]
    np.testing.assert_array_equal(got[4], beta[idx])       # leader_output = the schedule's beta


def test_round_trip_through_the_device_verifier(gpu_lib, sk):
    """The winners' certified VRFs under the device verifier (ouro_vrf03_verify_
    batch on (pk, proof, mkSeed alpha)): every one verifies with the prover's
    output, and one with a flipped bit does not."""
    ps = SETS["half"]
    rc, cls, _, _ = FC.sched_raw(sk, ps, 257, host=False)
    slots = _winners(cls, ps["first_slot"])
    rc, ep, eo, lp, lo = FC.vrfs_raw(sk, ps["eta0"], slots, host=False)
    assert rc == 0
    m = len(slots)
    alphas = [FC.mk_alpha(s, ps["eta0"], False) for s in slots] + \
             [FC.mk_alpha(s, ps["eta0"], True) for s in slots]
    proofs = np.concatenate([ep, lp]).copy()
    proofs[0, 40] ^= 1
    ok, beta = PraosVRF.verify_batch([sk[32:]] * (2 * m), alphas, proofs)
    assert not ok[0] and ok[1:].all()
    np.testing.assert_array_equal(beta[1:], np.concatenate([eo, lo])[1:])


CHILD = r"""
import ctypes, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch
torch.cuda.init()
import numpy as np
import forge_cases as FC
from ouroboros_network_amd import _native
lib = _native.load()
assert _native.test_hooks()
sk = FC.pool_key()
ps = FC.param_sets(70)["overlay"]
alphas, buf, off, ln = FC.prove_inputs(70)
a, b0, b1 = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b0))
d = [FC.prove_raw(70, [sk], 1, buf, off, ln, host=False),
     FC.sched_raw(sk, ps, 70, host=False),
     FC.vrfs_raw(sk, ps["eta0"], [5, 6, 7], host=False)]
assert b"recomputed on the host path" in lib.ouro_last_error()
lib.ouro_debug_host_path(ctypes.byref(a), ctypes.byref(b1))
assert b1.value - b0.value == 3, (b0.value, b1.value)
h = [FC.prove_raw(70, [sk], 1, buf, off, ln, host=True),
     FC.sched_raw(sk, ps, 70, host=True),
     FC.vrfs_raw(sk, ps["eta0"], [5, 6, 7], host=True)]
for x, y in zip(d, h):
    assert x[0] == 0 and y[0] == 0
    for p, q in zip(x[1:], y[1:]):
        assert (p == q).all()
os.environ["OURO_ON_DEVICE_ERROR"] = "fail"
lib.ouro_debug_reload_knobs()
assert FC.sched_raw(sk, ps, 70, host=False)[0] == _native.OURO_EDEVICE
assert FC.prove_raw(70, [sk], 1, buf, off, ln, host=False)[0] == _native.OURO_EDEVICE
assert FC.vrfs_raw(sk, ps["eta0"], [5], host=False)[0] == _native.OURO_EDEVICE
print("ok")
"""


def test_device_error_recomputes_on_the_host_path(gpu_lib):
    """A fresh child process on the test build with OURO_TEST_DEVICE_ERROR
    set: every launch reports a device error, the three entries recompute on
    the host path and give the host entries' results; OURO_ON_DEVICE_ERROR=fail
    returns the error instead."""
    assert os.path.exists(_native.TEST_LIB_PATH), "build lib/libouro_verify_test.so (make)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("OURO_")}
    env["OURO_VERIFY_LIB"] = _native.TEST_LIB_PATH
    env["OURO_TEST_DEVICE_ERROR"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
