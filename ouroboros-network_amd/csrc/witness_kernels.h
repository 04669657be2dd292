// witness_kernels.h -- the transaction-witness kernels that do not depend on
// the era, written once: count, clear and finish as templates on a small era
// trait, the tail kernel as it is, and their launches (kernels_witness.hip and
// kernels_byron_witness.hip instantiate them).  Device code of the unit that
// includes it, inside that unit's renamed namespace, as scan_excl.h is, so the
// kernels' names stay distinct per era.  The emit and verify kernels stay in
// the units: they carry what the eras do differently.
//
// The trait:
//   kKeyBytes   a witness key row's width
//   kAllOk      the verdict of a block whose witnesses all verify
//   kEbbOk      whether a block of status OURO_PACK_EBB has that verdict too
//   count_one   the walker's count pass (cbor_witness.h, cbor_byron_witness.h)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ouro_verify.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"
#include "scan_excl.h"

namespace ouro {
namespace wit {

// the kind of a witness row nothing was emitted to (k_witness_clear); the
// verify kernels write zeros for it
constexpr uint8_t kUnwritten = 0xff;

inline unsigned lane_grid(size_t n) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, 4096));
}

// one lane per block: the count pass; zeros where the block does not slice
// (Byron: unless it is a regular block that slices)
template <class Era>
__global__ void __launch_bounds__(kBlock) k_witness_count(
    const uint8_t* __restrict__ raw, size_t raw_bytes, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, size_t n, uint8_t* __restrict__ status,
    uint32_t* __restrict__ ntx, uint32_t* __restrict__ nwit) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = ldg8(off + i);
    const uint32_t l0 = (uint32_t)ldg1(len + i);
    uint32_t a = 0, b = 0;
    const uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                           ? (uint8_t)OURO_PACK_ESPAN
                           : Era::count_one(raw, o0, l0, &a, &b);
    status[i] = st;
    stg1(ntx + i, (int32_t)a);
    stg1(nwit + i, (int32_t)b);
  }
}

// Every row up to the capacities to "not written": a tx span outside the raw
// buffer (k_blake2b256 then writes a zero digest), a witness row of kind
// kUnwritten with a zero key, so that the rows of a block that did not fit,
// and those past the totals, read as zero.
template <class Era>
__global__ void __launch_bounds__(kBlock) k_witness_clear(
    size_t tx_cap, size_t wit_cap, uint64_t* __restrict__ tx_off, uint32_t* __restrict__ tx_len,
    uint32_t* __restrict__ wit_tx, uint8_t* __restrict__ kind, uint8_t* __restrict__ vk) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < tx_cap; i += nth) {
    stg8(tx_off + i, ~0ull);
    stg1(tx_len + i, 0);
  }
  for (size_t i = tid; i < wit_cap; i += nth) {
    stg1(wit_tx + i, 0);
    kind[i] = kUnwritten;
    cbor::zero_bytes(vk + Era::kKeyBytes * i, Era::kKeyBytes);
  }
}

// the rows from the row count (rows[1], the scan) to the capacity: zeros (a
// kernel of its own, so that the verify kernel's loop is k_ed25519_verify's)
__global__ void __launch_bounds__(kBlock) k_witness_tail(const uint64_t* __restrict__ rows,
                                                         size_t wit_cap, uint8_t* __restrict__ kind,
                                                         uint8_t* __restrict__ wit_ok) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)ldg8(rows + 1) + tid; i < wit_cap; i += nth) {
    kind[i] = 0;
    wit_ok[i] = 0;
  }
}

// one lane per block: n_bad[i] = its witness rows with wit_ok == 0; verdict[i]
// = kAllOk iff the block sliced, fit and n_bad == 0, or is an EBB where kEbbOk
template <class Era>
__global__ void __launch_bounds__(kBlock) k_witness_finish(
    size_t n, const uint8_t* __restrict__ status, const uint64_t* __restrict__ wit_begin,
    const uint8_t* __restrict__ wit_ok, uint64_t wit_cap, uint8_t* __restrict__ verdict,
    uint32_t* __restrict__ n_bad) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t bad = 0;
    uint8_t v = Era::kEbbOk && status[i] == OURO_PACK_EBB ? (uint8_t)Era::kAllOk : (uint8_t)0;
    if (status[i] == OURO_PACK_OK) {
      const uint64_t lo = ldg8(wit_begin + i), e = ldg8(wit_begin + i + 1);
      const uint64_t hi = e < wit_cap ? e : wit_cap;
      for (uint64_t r = lo; r < hi; r++) bad += ldg_u8(wit_ok + r) ? 0u : 1u;
      v = bad == 0 ? (uint8_t)Era::kAllOk : (uint8_t)0;
    }
    stg1(n_bad + i, (int32_t)bad);
    verdict[i] = v;
  }
}

// ---- their launches on `st`, each checking itself (launches.h WitnessDev) ----
template <class Era>
int launch_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                 const uint32_t* len, size_t n, uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_witness_count<Era>, dim3(lane_grid(n)), dim3(kBlock), 0, st, raw, raw_bytes,
                     off, len, n, status, ntx, nwit);
  return ouro_rt::launch_check();
}
inline int launch_scan(hipStream_t st, size_t n, const ouro_rt::WitnessDev& d) {
  if (n == 0) return OURO_OK;
  const scan::Args<ouro_rt::kWitnessVals> a{
      {d.ntx, d.nwit}, {d.tx_begin, d.wit_begin}, {(uint64_t)d.tx_cap, (uint64_t)d.wit_cap}};
  scan::launch<ouro_rt::kWitnessVals>(st, n, a, d.sums, d.rows);
  return ouro_rt::launch_check();
}
// (the emit launch's first step; the unit's own emit kernel follows it)
template <class Era>
void launch_clear(hipStream_t st, const ouro_rt::WitnessDev& d) {
  hipLaunchKernelGGL(k_witness_clear<Era>, dim3(lane_grid(std::max(d.tx_cap, d.wit_cap))),
                     dim3(kBlock), 0, st, d.tx_cap, d.wit_cap, d.tx_off, d.tx_len, d.wit_tx, d.kind,
                     d.vk);
}
// (the verify launch's last step)
inline void launch_tail(hipStream_t st, const ouro_rt::WitnessDev& d) {
  hipLaunchKernelGGL(k_witness_tail, dim3(lane_grid(d.wit_cap)), dim3(kBlock), 0, st, d.rows,
                     d.wit_cap, d.kind, d.wit_ok);
}
template <class Era>
int launch_finish(hipStream_t st, size_t n, const uint8_t* status, const ouro_rt::WitnessDev& d,
                  uint8_t* verdict, uint32_t* n_bad) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_witness_finish<Era>, dim3(lane_grid(n)), dim3(kBlock), 0, st, n, status,
                     d.wit_begin, d.wit_ok, (uint64_t)d.wit_cap, verdict, n_bad);
  return ouro_rt::launch_check();
}

}  // namespace wit
}  // namespace ouro
