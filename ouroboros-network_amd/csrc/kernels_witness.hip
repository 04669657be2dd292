// kernels_witness.hip -- the transaction-witness kernels (cbor_witness.h) and
// their launches (launches.h launch_witness_*).
//
// A translation unit of its own, as kernels_ledger.hip is: k_witness_verify is
// another user of verify.h's lane routines, and its copies live in namespace
// ouro_wit, so no symbol is shared with kernels.hip's and every kernel there is
// built exactly as before.  The launches take plain pointers only, one struct of
// them (launches.h WitnessDev): no type of the renamed namespace crosses to the
// host units.
//
// The sequence (witness_flow.h count_scan, rows): count (one lane per block),
// the two-value exclusive scan (scan_excl.h), clear, emit (one lane per block,
// at the rows the scan gave it: no atomics), the tx ids (kernels.hip's
// launch_blake2b over the emitted spans), verify (one lane per witness row,
// the row count read from device memory), the tail and finish (one lane per
// block).  Count, clear, tail and finish are witness_kernels.h's, shared with
// kernels_byron_witness.hip; emit and verify are this era's own.
#define ouro ouro_wit
#include <hip/hip_runtime.h>

#include "../../include/ouro_verify.h"
#include "cbor_witness.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"
#include "witness_kernels.h"

using namespace ouro;
using namespace ouro_rt;

// the era trait of witness_kernels.h
struct ShelleyWit {
  static constexpr int kKeyBytes = 32;
  static constexpr uint8_t kAllOk = OURO_WIT_ALL_OK;
  static constexpr bool kEbbOk = false;
  static __device__ __forceinline__ uint8_t count_one(const uint8_t* raw, uint64_t base,
                                                      uint32_t len, uint32_t* ntx, uint32_t* nwit) {
    return cbor::witness_count_one(raw, base, len, ntx, nwit);
  }
};

// one lane per block: the emit pass of a sliced block whose rows fit, at the
// rows the scan gave it; one that does not fit: OURO_PACK_ECAP, nothing written
__global__ void __launch_bounds__(kBlock) k_witness_emit(const uint8_t* __restrict__ raw,
                                                         const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ len, size_t n,
                                                         const uint32_t* __restrict__ ntx,
                                                         const uint32_t* __restrict__ nwit,
                                                         const uint64_t* __restrict__ tx_begin,
                                                         const uint64_t* __restrict__ wit_begin,
                                                         uint64_t tx_cap, uint64_t wit_cap,
                                                         cbor::WitRows rows,
                                                         uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    if (status[i] != OURO_PACK_OK) continue;  // (its span was checked by the count pass)
    const uint64_t t0 = ldg8(tx_begin + i), w0 = ldg8(wit_begin + i);
    const uint32_t a = (uint32_t)ldg1(ntx + i), b = (uint32_t)ldg1(nwit + i);
    if (t0 > tx_cap || tx_cap - t0 < a || w0 > wit_cap || wit_cap - w0 < b) {
      status[i] = (uint8_t)OURO_PACK_ECAP;
      continue;
    }
    cbor::witness_emit_one(raw, ldg8(off + i), (uint32_t)ldg1(len + i), rows, t0, w0, a, b);
  }
}

// One lane per witness row around ed25519_verify_lane (byron = false), with
// k_ed25519_verify's scratch slots and B table.  The grid is sized from the
// capacity; the row count comes from device memory (rows[1], the scan).
// The message is the row's transaction id (tx_id row wit_tx - tx_base).  A row nothing was emitted to
// (wit::kUnwritten) gets zeros.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_witness_verify(
    const uint64_t* __restrict__ rows, const uint8_t* __restrict__ vk,
    const uint8_t* __restrict__ sig, const uint32_t* __restrict__ wit_tx,
    const uint8_t* __restrict__ tx_id, uint64_t tx_cap, uint64_t tx_base,
    uint8_t* __restrict__ kind, uint8_t* __restrict__ wit_ok, int32_t* scratch,
    const int32_t* __restrict__ btab) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  const size_t n = (size_t)ldg8(rows + 1);
  for (size_t i = tid; i < n; i += nth) {
    // wit_tx is the global row; tx_id holds this call's rows, the first tx_base
    const uint64_t t = (uint64_t)(uint32_t)ldg1(wit_tx + i) - tx_base;
    if (kind[i] == wit::kUnwritten || t >= tx_cap) {  // (t < tx_cap always for an emitted row)
      kind[i] = 0;
      wit_ok[i] = 0;
      continue;
    }
    uint32_t s[16], p[8];
    load_words(s, sig + 64 * i, 4);
    load_words(p, vk + 32 * i, 2);
    const bool ok = ed25519_verify_lane(s, p, ShaGlobalTail{tx_id + 32 * t}, 32, lane, btab,
                                        false);
    wit_ok[i] = ok ? 1 : 0;
  }
}

namespace ouro_rt {

int launch_witness_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                         const uint32_t* len, size_t n, uint8_t* status, uint32_t* ntx,
                         uint32_t* nwit) {
  return wit::launch_count<ShelleyWit>(st, raw, raw_bytes, off, len, n, status, ntx, nwit);
}

int launch_witness_scan(hipStream_t st, size_t n, const WitnessDev& d) {
  return wit::launch_scan(st, n, d);
}

int launch_witness_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off, const uint32_t* len,
                        size_t n, int64_t, const WitnessDev& d, uint8_t* status) {
  if (n == 0) return OURO_OK;
  wit::launch_clear<ShelleyWit>(st, d);
  const cbor::WitRows rows{d.tx_off, d.tx_len, d.vk, d.sig, d.wit_tx, d.kind, d.tx_base};
  hipLaunchKernelGGL(k_witness_emit, dim3(wit::lane_grid(n)), dim3(kBlock), 0, st, raw, off, len, n,
                     d.ntx, d.nwit, d.tx_begin, d.wit_begin, (uint64_t)d.tx_cap,
                     (uint64_t)d.wit_cap, rows, status);
  return launch_check();
}

int launch_witness_verify(hipStream_t st, size_t n, const WitnessDev& d) {
  if (d.wit_cap == 0 || n == 0) return OURO_OK;
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, d.wit_cap, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_witness_verify, dim3(grid), dim3(kBlock), 0, st, d.rows, d.vk, d.sig,
                     d.wit_tx, d.tx_id, (uint64_t)d.tx_cap, d.tx_base, d.kind, d.wit_ok, scr,
                     ds->btab);
  wit::launch_tail(st, d);
  return launch_check();
}

int launch_witness_finish(hipStream_t st, size_t n, const uint8_t* status, const WitnessDev& d,
                          uint8_t* verdict, uint32_t* n_bad) {
  return wit::launch_finish<ShelleyWit>(st, n, status, d, verdict, n_bad);
}

}  // namespace ouro_rt
