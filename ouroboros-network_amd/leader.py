"""Leader threshold on the leader VRF output -- ledger-specs ``checkLeaderValue``.

Reference: ``meetsLeaderThreshold``
(ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:473-491)
calls ``SL.checkLeaderValue (VRF.certifiedOutput certNat) r (tpraosLeaderF
tpraosParams)`` with ``r`` the issuing pool's relative stake.  The reference
precomputes ``ActiveSlotCoeff``'s ``unActiveSlotLog = floor (10^34 ln (1 - f))``
once per network; this mirror takes that integer (``ActiveSlotCoeff`` below) so
the device never needs the reference's ``ln'``.

SURVEY.md §8(f) rank 3.  The batch runs on the GPU (``csrc/leader.h``); there is
no CPU fallback.  Parity is unpinned (the reference's packages are not in this
image): ``oracle/leader.py`` restates the same published algorithm
independently and the tests compare the two.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Sequence

import numpy as np

from . import _native
from ._pack import ptr

LEADER_NO = _native.LEADER_NO
LEADER_YES = _native.LEADER_YES
LEADER_BADARG = _native.LEADER_BADARG
SLOT_NOT_LEADER = _native.SLOT_NOT_LEADER
SLOT_LEADER = _native.SLOT_LEADER
SLOT_OVERLAY_ACTIVE = _native.SLOT_OVERLAY_ACTIVE
SLOT_OVERLAY_INACTIVE = _native.SLOT_OVERLAY_INACTIVE


@dataclass(frozen=True)
class ActiveSlotCoeff:
    """The reference's ``ActiveSlotCoeff``: ``unActiveSlotLog`` (a negative
    integer, floor(10^34 ln(1 - f))) and whether f is exactly 1."""

    un_active_slot_log: int
    is_one: bool = False

    def words(self):
        v = self.un_active_slot_log & ((1 << 128) - 1)
        lo = v & ((1 << 64) - 1)
        hi = v >> 64
        if hi >= 1 << 63:
            hi -= 1 << 64
        return hi, lo


def check_leader_values(beta_leader: np.ndarray, sigma: Sequence[Fraction],
                        f: ActiveSlotCoeff, host: bool = False) -> np.ndarray:
    """checkLeaderValue for every row of ``beta_leader`` (n x 64 u8) with the
    issuer's relative stake ``sigma[i]``; returns u8 LEADER_YES / LEADER_NO /
    LEADER_BADARG (sigma or f outside the supported domain).  host=True: the
    library's host path (ouro_leader_check_batch_host) instead of the GPU."""
    beta = np.ascontiguousarray(beta_leader, dtype=np.uint8).reshape(-1, 64)
    n = beta.shape[0]
    if len(sigma) != n:
        raise ValueError("one sigma per output")
    num = np.zeros(n, dtype=np.uint64)
    den = np.zeros(n, dtype=np.uint64)
    for i, s in enumerate(sigma):
        s = Fraction(s)
        if s.numerator < 0 or s.denominator >= 1 << 64 or s.numerator >= 1 << 64:
            raise ValueError("sigma must be a non-negative fraction of 64-bit integers")
        num[i], den[i] = s.numerator, s.denominator
    verdict = np.zeros(n, dtype=np.uint8)
    if n:
        hi, lo = f.words()
        name = "ouro_leader_check_batch" + ("_host" if host else "")
        rc = getattr(_native.load(), name)(n, ptr(beta), ptr(num), ptr(den), ctypes.c_int64(hi),
                                           ctypes.c_uint64(lo), 1 if f.is_one else 0,
                                           ptr(verdict))
        _native.check(rc, name)
    return verdict


def check_leader_value(beta: bytes, sigma: Fraction, f: ActiveSlotCoeff) -> bool:
    """The reference's single-item signature: Bool, True = eligible leader."""
    v = check_leader_values(np.frombuffer(bytes(beta), dtype=np.uint8).reshape(1, 64), [sigma], f)
    if v[0] == LEADER_BADARG:
        raise ValueError("sigma or active slot coefficient outside the supported domain")
    return bool(v[0] == LEADER_YES)


def _fraction64(x, what: str) -> Fraction:
    x = Fraction(x)
    if x.numerator < 0 or x.denominator >= 1 << 64 or x.numerator >= 1 << 64:
        raise ValueError(f"{what} must be a non-negative fraction of 64-bit integers")
    return x


def _nonce_arg(epoch_nonce: Optional[bytes]):
    if epoch_nonce is None:
        return None, None
    if len(epoch_nonce) != 32:
        raise ValueError("an epoch nonce is 32 bytes (None = NeutralNonce)")
    buf = np.frombuffer(bytes(epoch_nonce), dtype=np.uint8).copy()
    return buf, ptr(buf)


def leader_schedule(vrf_sk: bytes, epoch_nonce: Optional[bytes], first_slot: int, n_slots: int,
                    sigma: Fraction, f: ActiveSlotCoeff, d=Fraction(0),
                    asc_inv: Optional[int] = None, ngen: int = 0,
                    epoch_first_slot: Optional[int] = None, host: bool = False):
    """``checkIsLeader`` (Shelley/Protocol.hs:366-413) for slots ``first_slot ..
    first_slot + n_slots - 1`` of one epoch under the pool's VRF signing key
    (64 bytes, seed || pk) and relative stake ``sigma``.  Returns ``(cls,
    gen_index, beta_leader)``: the SLOT_* class of every slot (u8), the
    scheduled genesis key's index on an active overlay slot (u32, LV_NO_POOL
    elsewhere) and the leader VRF's output for every slot ((n, 64) u8).

    ``d`` is the decentralisation parameter; with ``d > 0`` the overlay
    schedule needs ``asc_inv`` (1 / f) and ``ngen`` (the epoch's genesis keys),
    and positions count from ``epoch_first_slot`` (default: ``first_slot``).
    host=True: ouro_tpraos_leader_schedule_host instead of the GPU."""
    if len(vrf_sk) != 64:
        raise ValueError("a VRF signing key is 64 bytes (seed || pk)")
    sigma = _fraction64(sigma, "sigma")
    d = _fraction64(d, "d")
    hi, lo = f.words()
    nonce_buf, nonce_ptr = _nonce_arg(epoch_nonce)
    p = _native.LeaderParamsC(
        epoch_nonce=nonce_ptr,
        epoch_first_slot=first_slot if epoch_first_slot is None else epoch_first_slot,
        sigma_num=sigma.numerator, sigma_den=sigma.denominator, act_log_hi=hi, act_log_lo=lo,
        f_is_one=1 if f.is_one else 0, d_num=d.numerator, d_den=d.denominator,
        asc_inv=0 if asc_inv is None else asc_inv, ngen=ngen)
    cls = np.zeros(n_slots, dtype=np.uint8)
    gen = np.full(n_slots, _native.LV_NO_POOL, dtype=np.uint32)
    beta = np.zeros((n_slots, 64), dtype=np.uint8)
    if n_slots:
        name = "ouro_tpraos_leader_schedule" + ("_host" if host else "")
        rc = getattr(_native.load(), name)(bytes(vrf_sk), ctypes.byref(p),
                                           ctypes.c_uint64(first_slot), n_slots, ptr(cls),
                                           ptr(gen), ptr(beta))
        _native.check(rc, name)
    return cls, gen, beta


def leader_vrfs(vrf_sk: bytes, epoch_nonce: Optional[bytes], slots, host: bool = False):
    """``TPraosIsLeader``'s two certified VRFs (rho and y of Protocol.hs:409-413)
    for the chosen ``slots``: ``(eta_proof (m, 80), eta_output (m, 64),
    leader_proof (m, 80), leader_output (m, 64))`` u8.  host=True:
    ouro_tpraos_leader_vrfs_host instead of the GPU."""
    if len(vrf_sk) != 64:
        raise ValueError("a VRF signing key is 64 bytes (seed || pk)")
    slot = np.ascontiguousarray(np.asarray(slots, dtype=np.uint64).reshape(-1))
    m = slot.shape[0]
    nonce_buf, nonce_ptr = _nonce_arg(epoch_nonce)
    ep = np.zeros((m, 80), dtype=np.uint8)
    eo = np.zeros((m, 64), dtype=np.uint8)
    lp = np.zeros((m, 80), dtype=np.uint8)
    lo = np.zeros((m, 64), dtype=np.uint8)
    if m:
        name = "ouro_tpraos_leader_vrfs" + ("_host" if host else "")
        rc = getattr(_native.load(), name)(bytes(vrf_sk), nonce_ptr, m, ptr(slot), ptr(ep),
                                           ptr(eo), ptr(lp), ptr(lo))
        _native.check(rc, name)
    return ep, eo, lp, lo
