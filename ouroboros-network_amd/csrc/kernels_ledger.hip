// kernels_ledger.hip -- the ledger-view checks' kernel (ledger_view.h) and its
// launch (launches.h launch_ledger).
//
// A translation unit of its own: the kernel is a second user of leader.h's
// routines, and inside kernels.hip that alone changed how the inliner built
// k_leader_check (its private, inlined copies became shared out-of-line
// functions: 85 -> 135 VGPRs, 5 -> 3 waves per SIMD).  Here its copies live in
// namespace ouro_lv (as kernels_lat.hip's live in ouro_lat), so no symbol is
// shared with kernels.hip's and every kernel there is built exactly as before.
//
// Built twice (Makefile), for the same reason: with -DOURO_LV_GEN=1 the unit
// holds k_ledger_checks_overlay, the kernel of a call with a genesis-delegation
// schedule (ouro_genesis_delegs), its routines in namespace ouro_lvo.  As a
// second instantiation beside k_ledger_checks in ONE unit the two shared
// leader.h's routines out of line and both went from 105 to 135 VGPRs (4 -> 3
// waves per SIMD); apart, a call without a schedule runs the kernel it always
// ran.
#ifndef OURO_LV_GEN
#define OURO_LV_GEN 0
#endif
#if OURO_LV_GEN
#define ouro ouro_lvo
#else
#define ouro ouro_lv
#endif
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ouro_verify.h"
#include "launch.h"
#include "ledger_view.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;
using namespace ouro_rt;

// One header row per lane: ledger[i] = OURO_LV_* bits (COUNTER_OK excepted: the
// host's fold), pool_row[i] = the issuer's view row.  The rows are a slicer's
// arena columns (16-byte aligned); v's pointers are device pointers.
// The two searches and the two compressions are short; the leader routine is
// long and its trip count depends on the data, so it has ONE call site, after
// the lookup: the lanes of a wave that reach it run it together.
#if !OURO_LV_GEN
__global__ void __launch_bounds__(kBlock) k_ledger_checks(size_t n, const uint8_t* __restrict__ issuer_vk,
                                                          const uint8_t* __restrict__ vrf_vk,
                                                          const uint64_t* __restrict__ slot,
                                                          const uint8_t* __restrict__ leader_output,
                                                          const uint64_t* __restrict__ ocert_kes_period,
                                                          ouro_ledger_views v, ouro_ledger_globals g,
                                                          uint8_t* __restrict__ ledger,
                                                          uint32_t* __restrict__ pool_row) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t row;
    ledger[i] = lv::ledger_check_lane(v, g, issuer_vk + 32 * i, vrf_vk + 32 * i, slot[i],
                                      leader_output + 64 * i, ocert_kes_period[i], &row);
    pool_row[i] = row;
  }
}

namespace ouro_rt {
int launch_ledger(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                  const uint64_t* slot, const uint8_t* leader_output,
                  const uint64_t* ocert_kes_period, const ouro_ledger_views& v,
                  const ouro_ledger_globals& g, uint8_t* ledger, uint32_t* pool_row) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  hipLaunchKernelGGL(k_ledger_checks, dim3(blocks), dim3(kBlock), 0, st, n, issuer_vk, vrf_vk, slot,
                     leader_output, ocert_kes_period, v, g, ledger, pool_row);
  return launch_check();
}
}  // namespace ouro_rt
#else
// The same with the schedule gd, whose pointers are device pointers into the
// views' block: an overlay row takes the delegate branch (ledger_view.h), and
// sits the leader routine out.
__global__ void __launch_bounds__(kBlock)
    k_ledger_checks_overlay(size_t n, const uint8_t* __restrict__ issuer_vk,
                            const uint8_t* __restrict__ vrf_vk, const uint64_t* __restrict__ slot,
                            const uint8_t* __restrict__ leader_output,
                            const uint64_t* __restrict__ ocert_kes_period, ouro_ledger_views v,
                            ouro_ledger_globals g, ouro_genesis_delegs gd,
                            uint8_t* __restrict__ ledger, uint32_t* __restrict__ pool_row) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t row;
    ledger[i] = lv::ledger_check_lane<true>(v, g, gd, issuer_vk + 32 * i, vrf_vk + 32 * i, slot[i],
                                            leader_output + 64 * i, ocert_kes_period[i], &row);
    pool_row[i] = row;
  }
}

namespace ouro_rt {
int launch_ledger_overlay(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                          const uint64_t* slot, const uint8_t* leader_output,
                          const uint64_t* ocert_kes_period, const ouro_ledger_views& v,
                          const ouro_ledger_globals& g, const ouro_genesis_delegs& gd,
                          uint8_t* ledger, uint32_t* pool_row) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  hipLaunchKernelGGL(k_ledger_checks_overlay, dim3(blocks), dim3(kBlock), 0, st, n, issuer_vk,
                     vrf_vk, slot, leader_output, ocert_kes_period, v, g, gd, ledger, pool_row);
  return launch_check();
}
}  // namespace ouro_rt
#endif
