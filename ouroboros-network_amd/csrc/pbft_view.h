// pbft_view.h -- the Byron ledger-view checks (include/ouro_verify.h
// OURO_PBFT_*): what the reference's PBFT instance checks per header beside
// the block signature (ouroboros-consensus/src/Ouroboros/Consensus/Protocol/
// PBFT.hs:322-357) -- the parallel part, for ONE sliced Byron header row
// against a delegation schedule: hashVerKey of the delegate key (sha3.h
// byron_key_hash) and its lookup among the entry's delegates (Bimap.lookupR).
// The one rule the kernel (kernels_pbft.hip k_pbft_checks), the host path
// (pbft_api.cpp) and the host-compiled test build (devhost_test.hip) all run;
// pbft.py restates it in Python and tests/test_pbft_rule.py pins the two
// against each other.  No allocation; host and device.  The slot check and the
// signing window are sequential and live on the host (pbft_api.cpp
// ouro_pbft_window_fold).
#pragma once
#include "../../include/ouro_verify.h"
#include "common.h"
#include "ledger_view.h"
#include "sha3.h"

namespace ouro {
namespace pbft {

// The OURO_PBFT_* bits of one row (SLOT_OK and WINDOW_OK excepted: the fold's)
// and the absolute schedule row of its delegate.  status: the Byron slicer's
// (OURO_PACK_OK: a regular header, OURO_PACK_EBB: an epoch-boundary header,
// anything else: not a sliced Byron row).  delegate_vk: the 64 XPub bytes.
OURO_HD inline uint8_t pbft_check_lane(const ouro_pbft_views& v, const uint8_t* delegate_vk,
                                       uint64_t slot, uint32_t status, uint32_t* genesis_row) {
  *genesis_row = OURO_LV_NO_POOL;
  if (status == OURO_PACK_EBB) return (uint8_t)(OURO_PBFT_BOUNDARY | OURO_PBFT_ALL_OK);
  if (status != OURO_PACK_OK) return 0;
  const uint32_t j = lv::entry_find(v.first_slot, (uint32_t)v.k, slot);
  uint32_t id[7];
  byron_key_hash(id, delegate_vk);
#pragma unroll
  for (int w = 0; w < 7; w++) id[w] = bswap32_b2(id[w]);
  const uint32_t row = lv::pool_find(v.delegate_id, (uint32_t)ldg1(v.dlg_begin + j),
                                     (uint32_t)ldg1(v.dlg_begin + j + 1), id);
  *genesis_row = row;
  return row != OURO_LV_NO_POOL ? (uint8_t)OURO_PBFT_DELEGATE_KNOWN : (uint8_t)0;
}

// KH of one XPub as its 28 bytes (out: 4-byte aligned on the device)
OURO_HD inline void key_hash_lane(uint8_t* out, const uint8_t* xpub) {
  uint32_t id[7];
  byron_key_hash(id, xpub);
#pragma unroll
  for (int w = 0; w < 7; w++) stg1(out + 4 * w, (int32_t)id[w]);
}

}  // namespace pbft
}  // namespace ouro
