"""PraosVRF evalCertified on the library's host path (include/ouro_verify.h
ouro_vrf03_prove_batch_host, ouro_vrf03_prove; csrc/prove.h): pinned byte for
byte to the IETF draft-03 vectors, to the oracle's prover and to a prover built
from libsodium 1.0.18's primitives (test_host_sodium.SodiumVRF), over alphas
whose lengths cross the SHA-512 padding and block boundaries of the 34-byte
prefix; every proof verifies under the library's own verifier with the same
output; and every argument check answers OURO_EINVAL before anything runs.
No GPU."""
import ctypes

import numpy as np
import pytest

import forge_cases as FC
import oracle_ffi as O
from ouroboros_network_amd import PraosVRF, _native

EINVAL = _native.OURO_EINVAL


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def test_draft03_vectors(lib, kats):
    """Key, proof and output of the three vectors (alphas of 0, 1 and 2
    bytes), through the batch entry and the single-item one."""
    vs = kats["vrf_draft03"]
    assert sorted(len(v["alpha"]) // 2 for v in vs) == [0, 1, 2]
    for v in vs:
        sk64 = bytes.fromhex(v["sk"])[:32] + bytes.fromhex(v["pk"])
        pk, sk = PraosVRF.keypair_from_seed(sk64[:32])
        assert pk.hex() == v["pk"] and sk == sk64
        alpha = bytes.fromhex(v["alpha"])
        out, proof = PraosVRF.eval_certified(sk, alpha)
        assert proof.hex() == v["pi"] and out.hex() == v["beta"]
        pr, be = PraosVRF.prove_batch(sk, [alpha], host=True)
        assert bytes(pr[0]).hex() == v["pi"] and bytes(be[0]).hex() == v["beta"]


@pytest.fixture(scope="module")
def batch(lib):
    """200 seeded keys, each with an alpha of every one of the eight lengths
    (1,600 items, every length at every alignment), proved once on the host
    path with per-item keys."""
    nl = len(FC.ISSUE_LENS)
    ks = [k for k in FC.keys() for _ in range(nl)]      # item i: key i // 8, length i % 8
    n = len(ks)
    alphas, buf, off, ln = FC.prove_inputs(n)
    rc, proof, beta = FC.prove_raw(n, [sk for _, sk in ks], n, buf, off, ln, host=True)
    assert rc == 0
    return ks, alphas, (buf, off, ln), proof, beta


def test_equals_the_oracle_prover(batch):
    ks, alphas, _, proof, beta = batch
    assert len(set(ks)) == 200 and len(ks) == 1600
    assert [len(a) for a in alphas[:8]] == FC.ISSUE_LENS == [len(a) for a in alphas[-8:]]
    for i, ((_, sk), a) in enumerate(zip(ks, alphas)):
        want = FC.oracle_prove(sk, a)
        assert bytes(proof[i]) == want[0] and bytes(beta[i]) == want[1], i


def test_equals_the_libsodium_built_prover(batch):
    s = O.sodium()
    if s is None:
        pytest.skip("libsodium 1.0.18 not present")
    from test_host_sodium import SodiumVRF

    vrf = SodiumVRF(s)
    ks, alphas, _, proof, beta = batch
    for i, ((pk, sk), a) in enumerate(zip(ks, alphas)):
        spk, ssk = vrf.keypair(sk[:32])
        assert spk == pk
        pi = vrf.prove(ssk, spk, a)
        assert bytes(proof[i]) == pi and bytes(beta[i]) == vrf.beta(pi), i


def test_single_item_entry_equals_the_batch(lib, batch):
    ks, alphas, _, proof, _ = batch
    out = ctypes.create_string_buffer(80)
    for i in range(0, len(ks), 5):
        assert lib.ouro_vrf03_prove(out, ks[i][1], alphas[i], len(alphas[i])) == 0
        assert out.raw == bytes(proof[i]), i


def test_every_proof_verifies_with_the_same_output(batch):
    ks, alphas, _, proof, beta = batch
    ok, out = PraosVRF.verify_batch([pk for pk, _ in ks], alphas, proof, host=True)
    assert ok.all()
    np.testing.assert_array_equal(out, beta)
    for i in range(0, len(ks), 17):
        assert PraosVRF.verify_vrf(None, ks[i][0], alphas[i], (bytes(beta[i]), bytes(proof[i])),
                                   mode="strict")


def test_shared_key_equals_per_item_keys(batch):
    ks, _, (buf, off, ln), _, _ = batch
    n, sk = len(ks), ks[5][1]
    rc1, p1, b1 = FC.prove_raw(n, [sk], 1, buf, off, ln, host=True)
    rcn, pn, bn = FC.prove_raw(n, [sk] * n, n, buf, off, ln, host=True)
    assert rc1 == 0 and rcn == 0
    np.testing.assert_array_equal(p1, pn)
    np.testing.assert_array_equal(b1, bn)
    _, p0, _ = FC.prove_raw(n, [sk], 1, buf, off, ln, host=True, want_beta=False)
    np.testing.assert_array_equal(p0, p1)


def test_the_public_key_bytes_are_used_as_given(lib):
    """sk[32:64] goes into hash_to_curve as it stands (crypto_vrf_ietfdraft03_
    prove never recomputes the key): another key's bytes there change the
    proof, and the oracle's prover agrees on it."""
    (pk0, sk0), (pk1, _) = FC.keys()[:2]
    mixed = sk0[:32] + pk1
    out = ctypes.create_string_buffer(80)
    assert lib.ouro_vrf03_prove(out, mixed, b"abc", 3) == 0
    assert out.raw == O.vrf_prove(mixed, b"abc") != O.vrf_prove(sk0, b"abc")


@pytest.mark.parametrize("host", [True, False])
def test_argument_checks(lib, host):
    """OURO_EINVAL before anything runs (so the device entry too, with no
    device here); n == 0 is OURO_OK."""
    fn = lib.ouro_vrf03_prove_batch_host if host else lib.ouro_vrf03_prove_batch
    sk = np.frombuffer(FC.pool_key() * 3, np.uint8).copy()
    buf = np.arange(40, dtype=np.uint8)
    off = np.array([0, 8, 30], np.uint64)
    ln = np.array([8, 22, 10], np.uint32)
    proof = np.zeros((3, 80), np.uint8)
    args = [3, O.p(sk), 3, O.p(buf), buf.size, O.p(off), O.p(ln), O.p(proof), None]

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[k if isinstance(k, int) else int(k[1:])] = v
        return fn(*a)

    assert fn(0, None, 0, None, 0, None, None, None, None) == 0
    for idx in (1, 5, 6, 7):                       # sk, alpha_off, alpha_len, proof
        assert call(**{f"a{idx}": None}) == EINVAL, idx
    assert call(a3=None) == EINVAL                 # alpha NULL with alpha_bytes > 0
    assert call(a2=2) == EINVAL and call(a2=0) == EINVAL and call(a2=4) == EINVAL   # nkeys
    assert call(a4=39) == EINVAL                   # the last span ends one byte outside
    bad = off.copy()
    bad[1] = 2**64 - 4                             # off + len wraps
    assert call(a5=O.p(bad)) == EINVAL
    bad[1] = 41                                    # starts outside
    assert call(a5=O.p(bad)) == EINVAL
    assert b"alpha 1" in lib.ouro_last_error()
    assert not proof.any()                         # nothing ran
    out = ctypes.create_string_buffer(80)
    assert lib.ouro_vrf03_prove(None, FC.pool_key(), b"", 0) == EINVAL
    assert lib.ouro_vrf03_prove(out, None, b"", 0) == EINVAL
    assert lib.ouro_vrf03_prove(out, FC.pool_key(), None, 1) == EINVAL
    assert lib.ouro_vrf03_prove(out, FC.pool_key(), None, 0) == 0      # the empty alpha
    assert out.raw == O.vrf_prove(FC.pool_key(), b"")


def test_no_key_bytes_in_the_last_error(lib):
    sk = FC.pool_key()
    off = np.array([5], np.uint64)
    ln = np.array([5], np.uint32)
    rc, _, _ = FC.prove_raw(1, [sk], 1, np.zeros(4, np.uint8), off, ln, host=True)
    assert rc == EINVAL
    msg = lib.ouro_last_error()
    assert sk[:8].hex().encode() not in msg and sk[:4] not in msg
