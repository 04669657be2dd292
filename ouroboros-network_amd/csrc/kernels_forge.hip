// kernels_forge.hip -- the forging-side kernels (forge.h, prove.h) and their
// launches (launches.h launch_leader_schedule, launch_vrf_prove).
//
// A translation unit of its own, as kernels_ledger.hip and kernels_witness.hip
// are: its copies of verify.h's lane routines live in namespace ouro_forge, so
// no symbol is shared with kernels.hip's and every kernel there is built
// exactly as before.  The launches take plain pointers and one plain struct.
//
// Both kernels borrow k_ed25519_verify's launch shape, per-lane scratch slots
// and B table (runtime.h plan(kEd)), as k_witness_verify does.  A lane's slot
// holds the secret scalar and its recoding while a multiplication runs; every
// lane clears them before it ends (prove.h prove_wipe_lane).
#define ouro ouro_forge
#include <hip/hip_runtime.h>

#include "../../include/ouro_verify.h"
#include "forge.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;
using namespace ouro_rt;

// checkIsLeader, one lane per slot first_slot + i (forge.h forge_schedule_item).
// beta / gen_index: optional.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_leader_schedule(
    ForgeSched s, uint64_t first_slot, size_t n, uint8_t* __restrict__ cls,
    uint32_t* __restrict__ gen_index, uint8_t* __restrict__ beta, int32_t* scratch,
    const int32_t* __restrict__ btab) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  for (size_t i = tid; i < n; i += nth) {
    uint32_t b[16], gi;
    const uint8_t c = forge_schedule_item(s, first_slot + i, b, &gi, lane, btab);
    cls[i] = c;
    if (gen_index) stg1(gen_index + i, (int32_t)gi);
    if (beta) store_words(beta + 64 * i, b, 4);
  }
  prove_wipe_lane(lane);
}

// The full prover, one lane per item.  sk: nkeys x 64 (nkeys 1: shared).
// alpha of item i: the span (alpha + off[i], len[i]) when slot is null, else
// mkSeed(seedEta for even i / seedL for odd i, slot[i / 2], eta0) -- the two
// certified VRFs of a forged header, interleaved.  beta: optional.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_vrf03_prove(
    size_t n, const uint8_t* __restrict__ sk, uint32_t shared_key,
    const uint8_t* __restrict__ alpha, const uint64_t* __restrict__ alpha_off,
    const uint32_t* __restrict__ alpha_len, const uint64_t* __restrict__ slot,
    const uint8_t* __restrict__ eta0, uint8_t* __restrict__ proof, uint8_t* __restrict__ beta,
    int32_t* scratch, const int32_t* __restrict__ btab) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  for (size_t i = tid; i < n; i += nth) {
    uint32_t k[16], pi[20], b[16];
    load_words(k, sk + (shared_key ? 0 : 64 * i), 4);
    if (slot) {
      uint32_t e0[8];
      if (eta0) load_words(e0, eta0, 2);
      ProveRegTail a;
      forge_seed(a.w, ldg8(slot + (i >> 1)), eta0 ? e0 : nullptr, (i & 1) != 0);
      forge_prove_item(pi, beta ? b : nullptr, k, a, 32, lane, btab);
    } else {
      forge_prove_item(pi, beta ? b : nullptr, k, ShaGlobalTail{alpha + ldg8(alpha_off + i)},
                       (uint32_t)ldg1(alpha_len + i), lane, btab);
    }
    store_words(proof + 80 * i, pi, 5);
    if (beta) store_words(beta + 64 * i, b, 4);
  }
  prove_wipe_lane(lane);
}

namespace ouro_rt {

int launch_leader_schedule(hipStream_t st, const OuroForgeSched& s, uint64_t first_slot, size_t n,
                           uint8_t* cls, uint32_t* gen_index, uint8_t* beta) {
  if (n == 0) return OURO_OK;
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, n, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_leader_schedule, dim3(grid), dim3(kBlock), 0, st, s, first_slot, n, cls,
                     gen_index, beta, scr, ds->btab);
  return launch_check();
}

int launch_vrf_prove(hipStream_t st, size_t n, const uint8_t* sk, bool shared_key,
                     const uint8_t* alpha, const uint64_t* off, const uint32_t* len,
                     const uint64_t* slot, const uint8_t* eta0, uint8_t* proof, uint8_t* beta) {
  if (n == 0) return OURO_OK;
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, n, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_vrf03_prove, dim3(grid), dim3(kBlock), 0, st, n, sk, shared_key ? 1u : 0u,
                     alpha, off, len, slot, eta0, proof, beta, scr, ds->btab);
  return launch_check();
}

}  // namespace ouro_rt
