// ledger_view.h -- the ledger-view header checks (include/ouro_verify.h
// OURO_LV_*): what SL.updateChainDepState (ouroboros-consensus-shelley/src/
// Ouroboros/Consensus/Shelley/Protocol.hs:433-442) checks with the epoch's
// LedgerView beside the signatures -- ledger-specs' OVERLAY rule (the pool
// lookup, the VRF key hash, checkLeaderValue under the pool's stake) and the
// period bounds of its OCERT rule -- for ONE sliced TPraos header row against
// a ledger-view schedule.  The one rule the kernel (kernels.hip
// k_ledger_checks), the host path and the host-compiled test build
// (devhost_test.hip dh_ledger_check) all run; ledger.py restates it in Python
// and tests/test_ledger_rule.py pins the two against each other.  No
// allocation; host and device.  With a genesis-delegation schedule the same
// routine evaluates the rule's other branch on overlay slots (lookupInOverlay
// Schedule, pbftVrfChecks).  The counter check is sequential and lives on
// the host (ledger_api.cpp ouro_ocert_counter_fold).
#pragma once
#include "../../include/ouro_verify.h"
#include "blake2b.h"
#include "common.h"
#include "leader.h"

namespace ouro {
namespace lv {

// The entry of `slot`: the last j with first_slot[j] <= slot (first_slot[0] is
// 0, so there always is one) -- the search of tpraos.h epoch_tab_find.
OURO_FI uint32_t entry_find(const uint64_t* first_slot, uint32_t k, uint64_t slot) {
  uint32_t lo = 0, hi = k;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ldg8(first_slot + mid) <= slot) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ledger-specs isOverlaySlot: ceil(s d) < ceil((s + 1) d) with d = num / den
// (num <= den, den > 0), in exact integers.  With a = s num and r = a mod den
// the next multiple of den at or above a is a + g, g = (den - r) mod den, and
// the ceiling steps iff a + num passes it: num > g.  a < 2^128.
// *position = ceil(s d) = q + (r != 0), from the same division (classifyOverlay
// Slot's position; <= s, so 64 bits hold it); 0 when num == 0.
OURO_HD inline bool overlay_position(uint64_t s, uint64_t num, uint64_t den, uint64_t* position) {
  *position = 0;
  if (num == 0) return false;
  const uint32_t s2[2] = {(uint32_t)s, (uint32_t)(s >> 32)};
  const uint32_t n2[2] = {(uint32_t)num, (uint32_t)(num >> 32)};
  const uint32_t d2[2] = {(uint32_t)den, (uint32_t)(den >> 32)};
  uint32_t a[4], q[4], rem[2];
  mw_mul<2, 2>(a, s2, n2);
  mw_divq<4, 2, 4>(q, rem, a, d2);  // floor(a / 2^128) = 0 < den
  const uint64_t r = (uint64_t)rem[0] | ((uint64_t)rem[1] << 32);
  const uint64_t g = r ? den - r : 0;
  *position = ((uint64_t)q[0] | ((uint64_t)q[1] << 32)) + (r != 0);
  return num > g;
}
OURO_HD inline bool is_overlay_slot(uint64_t s, uint64_t num, uint64_t den) {
  uint64_t position;
  return overlay_position(s, num, den, &position);
}

// ledger-specs classifyOverlaySlot on an overlay slot: active iff position mod
// asc_inv == 0, and then the scheduled genesis key is element (position div
// asc_inv) mod ngen of the entry's sorted keys.  Returns that index, or
// OURO_LV_NO_POOL on an inactive slot (and for ngen == 0, which the argument
// checks refuse wherever d > 0).  asc_inv >= 1.
OURO_HD inline uint32_t overlay_index(uint64_t position, uint64_t asc_inv, uint32_t ngen) {
  const uint64_t t = position / asc_inv;
  if (t * asc_inv != position || ngen == 0) return OURO_LV_NO_POOL;
  return (uint32_t)(t % ngen);
}

// The row of pool id `id` (7 words, each the big-endian value of 4 id bytes,
// so word order is unsigned byte order) among rows [b, e) of pool_id (28 bytes
// a row, sorted strictly ascending), or OURO_LV_NO_POOL.
OURO_HD inline uint32_t pool_find(const uint8_t* pool_id, uint32_t b, uint32_t e,
                                  const uint32_t id[7]) {
  uint32_t lo = b, hi = e;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint8_t* p = pool_id + 28 * (size_t)mid;
    int c = 0;  // sign of row - id
#pragma unroll
    for (int w = 0; w < 7; w++) {
      const uint32_t x = bswap32_b2((uint32_t)ldg1(p + 4 * w));
      if (c == 0 && x != id[w]) c = x < id[w] ? -1 : 1;
    }
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1;
    else hi = mid;
  }
  return OURO_LV_NO_POOL;
}

// c0 <= kp < c0 + max_evo with the sum not wrapping (a c0 above
// 2^64 - max_evo fails), kp = slot / spkp
OURO_FI bool kes_period_ok(uint64_t slot, uint64_t c0, uint64_t spkp, uint64_t max_evo) {
  const uint64_t kp = slot / spkp;
  const bool wraps = c0 > (uint64_t)0 - max_evo;  // (max_evo == 0: nothing passes below)
  return c0 <= kp && kp - c0 < max_evo && !wraps;
}

// The OURO_LV_* bits of one header row (COUNTER_OK excepted) and its view row.
// issuer_vk, vrf_vk: 32 bytes; leader_output: the header's claimed 64 bytes.
// kGen: with the genesis-delegation schedule gd (include/ouro_verify.h
// ouro_genesis_delegs; unread otherwise) an overlay row takes the delegate
// branch -- the row is indexed, not searched, and its registered hashes are
// the delegate's -- through the SAME two hash sites as a pool row; the row is
// then a genesis row.  Without it an overlay row stops at OURO_LV_OVERLAY.
template <bool kGen>
OURO_HD inline uint8_t ledger_check_lane(const ouro_ledger_views& v, const ouro_ledger_globals& g,
                                         const ouro_genesis_delegs& gd, const uint8_t* issuer_vk,
                                         const uint8_t* vrf_vk, uint64_t slot,
                                         const uint8_t* leader_output, uint64_t c0,
                                         uint32_t* pool_row) {
  uint32_t bits = 0, row = OURO_LV_NO_POOL;
  if (kes_period_ok(slot, c0, g.slots_per_kes_period, g.max_kes_evo)) bits |= OURO_LV_KES_PERIOD_OK;
  const uint32_t j = entry_find(v.first_slot, (uint32_t)v.k, slot);
  const uint64_t s = slot - ldg8(v.first_slot + j);
  uint64_t position;
  const bool overlay = overlay_position(s, ldg8(v.d_num + j), ldg8(v.d_den + j), &position);
  uint32_t grow = OURO_LV_NO_POOL;  // the scheduled delegate's row on an active overlay slot
  if (overlay) {
    bits |= OURO_LV_OVERLAY;
    if (kGen) {
      const uint32_t gb = (uint32_t)ldg1(gd.gen_begin + j);
      const uint32_t ix = overlay_index(position, gd.asc_inv, (uint32_t)ldg1(gd.gen_begin + j + 1) - gb);
      if (ix != OURO_LV_NO_POOL) {
        bits |= OURO_LV_OVERLAY_ACTIVE;
        grow = gb + ix;
      }
    }
  }
  const bool deleg = kGen && overlay;  // the delegate branch (then grow is a row)
  if (!overlay || (kGen && grow != OURO_LV_NO_POOL)) {
    uint32_t in[16], id[7];
#pragma unroll
    for (int w = 0; w < 16; w++) in[w] = w < 8 ? (uint32_t)ldg1(issuer_vk + 4 * w) : 0u;
    blake2b224_short(id, in, 32);
    if (deleg) {
      uint32_t diff = 0;
      const uint8_t* reg = gd.delegate_id + 28 * (size_t)grow;
#pragma unroll
      for (int w = 0; w < 7; w++) diff |= id[w] ^ (uint32_t)ldg1(reg + 4 * w);
      if (diff == 0) row = grow;
    } else {
#pragma unroll
      for (int w = 0; w < 7; w++) id[w] = bswap32_b2(id[w]);
      row = pool_find(v.pool_id, (uint32_t)ldg1(v.pool_begin + j),
                      (uint32_t)ldg1(v.pool_begin + j + 1), id);
    }
  }
  // (one site for the long, data-dependent leader routine: the lanes of a wave
  // that reach it run it together, whatever they did above; overlay lanes sit
  // it out -- there is no threshold on an overlay slot)
  if (row != OURO_LV_NO_POOL) {
    bits |= OURO_LV_POOL_KNOWN;
    uint32_t in[16], h[8];
#pragma unroll
    for (int w = 0; w < 16; w++) in[w] = w < 8 ? (uint32_t)ldg1(vrf_vk + 4 * w) : 0u;
    blake2b256_short(h, in, 32);
    uint32_t diff = 0;
    const uint8_t* reg = (deleg ? gd.delegate_vrf : v.vrf_hash) + 32 * (size_t)row;
#pragma unroll
    for (int w = 0; w < 8; w++) diff |= h[w] ^ (uint32_t)ldg1(reg + 4 * w);
    if (diff == 0) bits |= OURO_LV_VRF_KEY_OK;
    const int32_t r = deleg || g.f_is_one
                          ? kLeaderYes
                          : leader_check_lane(leader_output, ldg8(v.sigma_num + row),
                                              ldg8(v.sigma_den + row), g.act_log_lo, g.act_log_hi);
    if (r == kLeaderYes) bits |= OURO_LV_LEADER_OK;
    if (r == kLeaderBadArg) bits |= OURO_LV_BADARG;
  }
  *pool_row = row;
  return (uint8_t)bits;
}
// without a schedule
OURO_HD inline uint8_t ledger_check_lane(const ouro_ledger_views& v, const ouro_ledger_globals& g,
                                         const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                                         uint64_t slot, const uint8_t* leader_output, uint64_t c0,
                                         uint32_t* pool_row) {
  return ledger_check_lane<false>(v, g, ouro_genesis_delegs{}, issuer_vk, vrf_vk, slot,
                                  leader_output, c0, pool_row);
}

}  // namespace lv
}  // namespace ouro
