// forge.h -- one item of the forging-side entries (include/ouro_verify.h
// ouro_tpraos_leader_schedule, ouro_vrf03_prove_batch, ouro_tpraos_leader_vrfs):
// checkIsLeader (ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/
// Protocol.hs:366-413) for one slot, and one certified VRF.  The one rule the
// kernels (kernels_forge.hip) and the host path (host_path.hip) both run, from
// routines the verifiers already have: mkSeed (blake2b.h mkseed_hash), the
// overlay classification (ledger_view.h), the leader threshold (leader.h) and
// the prover (prove.h).  No allocation; host and device.
#pragma once
#include "../../include/ouro_verify.h"
#include "blake2b.h"
#include "forge_args.h"
#include "leader.h"
#include "ledger_view.h"
#include "prove.h"

namespace ouro {

using ForgeSched = ::OuroForgeSched;  // forge_args.h

// mkSeed seedEta / seedL slot eta0 (eta0 null: NeutralNonce), as tpraos.h
// hdr_mkseed composes it for the verifiers
OURO_FI void forge_seed(uint32_t a[8], uint64_t slot, const uint32_t* eta0, bool leader) {
  mkseed_hash(a, slot, eta0);
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] ^= leader ? kSeedL[k] : kSeedEta[k];
}

// checkIsLeader for `slot`: the leader VRF's output (always evaluated: "We
// evaluate it as normal"), then the overlay classification when d > 0 and the
// slot is an overlay slot, else the threshold.  Returns the OURO_SLOT_* class;
// *gen_index = the scheduled genesis key's index on an active overlay slot,
// OURO_LV_NO_POOL otherwise.
OURO_HD inline uint8_t forge_schedule_item(const ForgeSched& s, uint64_t slot, uint32_t beta[16],
                                           uint32_t* gen_index, Slot lane, const int32_t* btab) {
  ProveRegTail alpha;
  forge_seed(alpha.w, slot, s.have_eta0 ? s.eta0 : nullptr, true);
  vrf03_gamma_lane(beta, s.x, s.pk, alpha, 32, lane, btab);
  *gen_index = OURO_LV_NO_POOL;
  uint64_t position;
  if (lv::overlay_position(slot - s.epoch_first_slot, s.d_num, s.d_den, &position)) {
    const uint32_t ix = lv::overlay_index(position, s.asc_inv, s.ngen);
    *gen_index = ix;
    return ix == OURO_LV_NO_POOL ? (uint8_t)OURO_SLOT_OVERLAY_INACTIVE
                                 : (uint8_t)OURO_SLOT_OVERLAY_ACTIVE;
  }
  if (s.f_is_one) return (uint8_t)OURO_SLOT_LEADER;
  uint8_t be[64];  // the output's bytes, as leader_check_lane reads them
#pragma unroll
  for (int k = 0; k < 64; k++) be[k] = (uint8_t)byte_of(beta, k);
  const int32_t r = leader_check_lane(be, s.sigma_num, s.sigma_den, s.act_log_lo, s.act_log_hi);
  return r == kLeaderYes ? (uint8_t)OURO_SLOT_LEADER : (uint8_t)OURO_SLOT_NOT_LEADER;
}

// One certified VRF: the 80-byte proof of `alpha` under sk = seed || pk, and
// its output when asked for (beta null: not computed).
template <class Tail>
OURO_HD inline void forge_prove_item(uint32_t pi[20], uint32_t* beta, const uint32_t sk[16],
                                     const Tail& alpha, uint32_t alen, Slot lane,
                                     const int32_t* btab) {
  ExpandedKey k;
  expand_vrf_sk(k, sk);
  vrf03_prove_lane(pi, k, alpha, alen, lane, btab, beta);
  prove_wipe(&k, sizeof k);
}

}  // namespace ouro
