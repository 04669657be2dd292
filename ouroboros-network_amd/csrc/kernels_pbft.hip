// kernels_pbft.hip -- the Byron ledger-view checks' kernels (pbft_view.h,
// sha3.h) and their launches (launches.h launch_pbft, launch_byron_key_hash).
//
// A translation unit of its own, its lane routines in namespace ouro_pbft, for
// the reason kernels_ledger.hip gives: a second user of blake2b.h's and
// ledger_view.h's routines inside another kernel unit changes how the inliner
// builds that unit's kernels.  Here no symbol is shared with kernels.hip,
// kernels_lat.hip or kernels_ledger.hip and every kernel there is built
// exactly as before.
#define ouro ouro_pbft
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ouro_verify.h"
#include "envelope.h"
#include "launch.h"
#include "pbft_view.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;
using namespace ouro_rt;

// One Byron header row per lane: pbft[i] = OURO_PBFT_* bits (SLOT_OK and
// WINDOW_OK excepted: the host's fold), genesis_row[i] = the delegate's
// schedule row.  delegate_vk is the Byron slicer's arena column (64 bytes a
// row, 16-byte aligned); v's pointers are device pointers.  One Keccak-f
// permutation, one Blake2b compression and a binary search per regular row; the
// 25 state words are indexed by literals only, so nothing goes to scratch.
__global__ void __launch_bounds__(kBlock) k_pbft_checks(size_t n, const uint8_t* __restrict__ delegate_vk,
                                                        const uint64_t* __restrict__ slot,
                                                        const uint8_t* __restrict__ status,
                                                        ouro_pbft_views v,
                                                        uint8_t* __restrict__ pbft,
                                                        uint32_t* __restrict__ genesis_row) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t row;
    pbft[i] = pbft::pbft_check_lane(v, delegate_vk + 64 * i, slot[i], status[i], &row);
    genesis_row[i] = row;
  }
}

// The same inside the raw-CBOR pipeline: row j of the chunk's Byron arena takes
// its slot from the envelope record of the same header (record idx[j] of the
// chunk in the caller's order; idx null: record j) and hands it on for the
// host's fold.  A row the envelope slicer did not slice has status != OK too.
__global__ void __launch_bounds__(kBlock)
    k_pbft_checks_chain(size_t n, const uint8_t* __restrict__ delegate_vk,
                        const uint8_t* __restrict__ status, const env::Rec* __restrict__ rec,
                        const uint32_t* __restrict__ idx, ouro_pbft_views v,
                        uint8_t* __restrict__ pbft, uint32_t* __restrict__ genesis_row,
                        uint64_t* __restrict__ slot_out) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const size_t r = idx ? idx[i] : i;
    const uint64_t slot = rec[r].slot;
    uint32_t row;
    pbft[i] = pbft::pbft_check_lane(v, delegate_vk + 64 * i, slot, status[i], &row);
    genesis_row[i] = row;
    slot_out[i] = slot;
  }
}

// KH of n XPubs: one key per lane (xpub n x 64, out n x 28, both 4-byte aligned)
__global__ void __launch_bounds__(kBlock) k_byron_key_hash(size_t n, const uint8_t* __restrict__ xpub,
                                                           uint8_t* __restrict__ out) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) pbft::key_hash_lane(out + 28 * i, xpub + 64 * i);
}

namespace ouro_rt {
int launch_pbft(hipStream_t st, size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                const uint8_t* status, const ouro_pbft_views& v, uint8_t* pbft,
                uint32_t* genesis_row) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, kPbftBlocksMax);
  hipLaunchKernelGGL(k_pbft_checks, dim3(blocks), dim3(kBlock), 0, st, n, delegate_vk, slot, status,
                     v, pbft, genesis_row);
  return launch_check();
}
int launch_pbft_chain(hipStream_t st, size_t n, const uint8_t* delegate_vk, const uint8_t* status,
                      const void* rec, const uint32_t* idx, const ouro_pbft_views& v,
                      uint8_t* pbft, uint32_t* genesis_row, uint64_t* slot_out) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, kPbftBlocksMax);
  hipLaunchKernelGGL(k_pbft_checks_chain, dim3(blocks), dim3(kBlock), 0, st, n, delegate_vk, status,
                     static_cast<const env::Rec*>(rec), idx, v, pbft, genesis_row, slot_out);
  return launch_check();
}
int launch_byron_key_hash(hipStream_t st, size_t n, const uint8_t* xpub, uint8_t* out) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, kPbftBlocksMax);
  hipLaunchKernelGGL(k_byron_key_hash, dim3(blocks), dim3(kBlock), 0, st, n, xpub, out);
  return launch_check();
}
}  // namespace ouro_rt
