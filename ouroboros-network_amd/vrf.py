"""PraosVRF (ECVRF-ED25519-SHA512-Elligator2, IETF draft-03) on gfx950 --
mirror of cardano-crypto-praos ``Cardano.Crypto.VRF.Praos``: the verify side,
and ``evalCertified`` (``eval_certified`` / ``prove_batch``; csrc/prove.h).  The
proving entries are for a machine that already holds the key: no constant-time
or side-channel claim is made (include/ouro_verify.h, "KEY HYGIENE").

Reference surface: ``verifyVRF :: ContextVRF v -> VerKeyVRF v -> a ->
(OutputVRF v, CertVRF v) -> Bool`` and ``verifyCertified``; the mock-protocol
usage is ouroboros-consensus-mock/src/Ouroboros/Consensus/Mock/Protocol/Praos.hs:341-354,
the real call is the OVERLAY rule via
ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:435.

Claimed-output semantics: ``verify_vrf`` in mode
``"ref2020"`` (default, as recalled for cardano-base@4251c0bb) checks the proof
only; ``"strict"`` additionally requires the claimed output to equal the
proof's output.  ``output_from_proof`` is ``crypto_vrf_ietfdraft03_proof_to_hash``.

The range of the proof's s: ``s_mode="reduce"`` (default,
the fork as recalled: s reduced mod L) or ``"strict"`` (s >= L rejected,
OURO_VRF_STRICT_S).  Which one cardano-crypto-praos uses is unpinned -- no
reference fixture has s >= L -- so both are offered.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._pack import as_rows, msgs_arg, ptr

SIZE_VERKEY = 32
SIZE_PROOF = 80
SIZE_OUTPUT = 64
SIZE_SIGNKEY = 64   # libsodium's layout: seed (32) || pk (32)
SIZE_SEED = 32


S_MODES = {"reduce": 0, "strict": _native.VRF_STRICT_S}


def _s_flags(s_mode: str) -> int:
    if s_mode not in S_MODES:
        raise ValueError(f"s_mode: one of {sorted(S_MODES)}")
    return S_MODES[s_mode]


class PraosVRF:
    @staticmethod
    def verify(vk: bytes, msg: bytes, proof: bytes, s_mode: str = "reduce"):
        """crypto_vrf_ietfdraft03_verify: the 64-byte output, or None."""
        if len(vk) != SIZE_VERKEY or len(proof) != SIZE_PROOF:
            return None
        if _s_flags(s_mode):
            ok, beta = PraosVRF.verify_batch([vk], [msg], [proof], s_mode=s_mode)
            return bytes(beta[0]) if ok[0] else None
        out = ctypes.create_string_buffer(SIZE_OUTPUT)
        rc = _native.load().ouro_vrf03_verify(out, vk, proof, msg, len(msg))
        if rc == _native.OURO_OK:
            return out.raw
        if rc == _native.OURO_INVALID:
            return None
        _native.check(rc, "ouro_vrf03_verify")
        return None

    @staticmethod
    def verify_vrf(ctx, vk: bytes, msg: bytes, certified, mode: str = "ref2020",
                   s_mode: str = "reduce") -> bool:
        """``verifyVRF () vk msg (output, proof)``."""
        output, proof = certified
        beta = PraosVRF.verify(vk, msg, proof, s_mode=s_mode)
        if beta is None:
            return False
        return True if mode == "ref2020" else bytes(output) == beta

    verify_certified = verify_vrf

    @staticmethod
    def output_from_proof(proof: bytes):
        """crypto_vrf_ietfdraft03_proof_to_hash: 64 bytes, or None if Gamma
        does not decode."""
        out = ctypes.create_string_buffer(SIZE_OUTPUT)
        rc = _native.load().ouro_vrf03_proof_to_hash(out, proof)
        if rc == _native.OURO_OK:
            return out.raw
        if rc == _native.OURO_INVALID:
            return None
        _native.check(rc, "ouro_vrf03_proof_to_hash")
        return None

    @staticmethod
    def verify_batch(vks, alphas, proofs, s_mode: str = "reduce", host: bool = False):
        """Returns (valid bool array, outputs (n, 64) uint8; zero rows where
        invalid).  host=True: the library's host path
        (ouro_vrf03_verify_batch_host) instead of the GPU."""
        flags = _s_flags(s_mode)
        vk = as_rows(vks, SIZE_VERKEY, "vk")
        pf = as_rows(proofs, SIZE_PROOF, "proof")
        buf, off, ln = msgs_arg(alphas)
        n = vk.shape[0]
        if pf.shape[0] != n or off.shape[0] != n:
            raise ValueError("vk, alpha and proof batches differ in length")
        ver = np.zeros(n, dtype=np.uint8)
        beta = np.zeros((n, SIZE_OUTPUT), dtype=np.uint8)
        if n:
            name = "ouro_vrf03_verify_batch_host" if host else "ouro_vrf03_verify_batch_flags"
            rc = getattr(_native.load(), name)(
                n, ptr(vk), ptr(pf), ptr(buf), ptr(off), ptr(ln), ptr(beta), ptr(ver), flags)
            _native.check(rc, name)
        return ver.astype(bool), beta

    @staticmethod
    def keypair_from_seed(seed: bytes):
        """crypto_vrf_ietfdraft03_keypair_from_seed: (pk, sk) with
        pk = [clamp(SHA-512(seed)[0:32])]B and sk = seed || pk."""
        if len(seed) != SIZE_SEED:
            raise ValueError("a VRF seed is 32 bytes")
        pk = ctypes.create_string_buffer(SIZE_VERKEY)
        sk = ctypes.create_string_buffer(SIZE_SIGNKEY)
        rc = _native.load().ouro_vrf03_keypair_from_seed(pk, sk, bytes(seed))
        _native.check(rc, "ouro_vrf03_keypair_from_seed")
        return pk.raw, sk.raw

    @staticmethod
    def eval_certified(sk: bytes, msg: bytes):
        """``evalCertified () msg sk``: (output64, proof80), one item on the
        library's host path (ouro_vrf03_prove, then proof_to_hash)."""
        if len(sk) != SIZE_SIGNKEY:
            raise ValueError("a VRF signing key is 64 bytes (seed || pk)")
        proof = ctypes.create_string_buffer(SIZE_PROOF)
        rc = _native.load().ouro_vrf03_prove(proof, bytes(sk), bytes(msg), len(msg))
        _native.check(rc, "ouro_vrf03_prove")
        out = PraosVRF.output_from_proof(proof.raw)
        if out is None:  # the prover encoded Gamma itself
            raise _native.DeviceError("ouro_vrf03_prove: the proof's Gamma does not decode")
        return out, proof.raw

    @staticmethod
    def prove_batch(sks, alphas, host: bool = False):
        """One certified VRF per alpha: (proofs (n, 80) uint8, outputs (n, 64)
        uint8).  ``sks``: one 64-byte key for every item (bytes, or one row) or
        one per item.  host=True: ouro_vrf03_prove_batch_host instead of the
        GPU."""
        if isinstance(sks, (bytes, bytearray)):
            sks = [bytes(sks)]
        sk = as_rows(sks, SIZE_SIGNKEY, "sk")
        buf, off, ln = msgs_arg(alphas)
        n = off.shape[0]
        if sk.shape[0] not in (1, n):
            raise ValueError("one signing key, or one per alpha")
        proof = np.zeros((n, SIZE_PROOF), dtype=np.uint8)
        beta = np.zeros((n, SIZE_OUTPUT), dtype=np.uint8)
        if n:
            name = "ouro_vrf03_prove_batch" + ("_host" if host else "")
            rc = getattr(_native.load(), name)(n, ptr(sk), sk.shape[0], ptr(buf), buf.size,
                                               ptr(off), ptr(ln), ptr(proof), ptr(beta))
            _native.check(rc, name)
        return proof, beta


verify_vrf = PraosVRF.verify_vrf
verify_certified = PraosVRF.verify_certified
output_from_proof = PraosVRF.output_from_proof
verify_batch = PraosVRF.verify_batch
eval_certified = PraosVRF.eval_certified
prove_batch = PraosVRF.prove_batch
keypair_from_seed = PraosVRF.keypair_from_seed
