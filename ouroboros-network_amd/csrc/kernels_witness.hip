// kernels_witness.hip -- the transaction-witness kernels (cbor_witness.h) and
// their launches (launches.h launch_witness_*).
//
// A translation unit of its own, as kernels_ledger.hip is: k_witness_verify is
// another user of verify.h's lane routines, and its copies live in namespace
// ouro_wit, so no symbol is shared with kernels.hip's and every kernel there is
// built exactly as before.  The launches take plain pointers only (no type of
// the renamed namespace crosses to the host units).
//
// The sequence (witness_api.cpp wit_launch): count (one lane per block), a
// two-level exclusive scan of both count arrays, clear, emit (one lane per
// block, at the rows the scan gave it: no atomics), the tx ids (kernels.hip's
// launch_blake2b over the emitted spans), verify (one lane per witness row,
// the row count read from device memory) and finish (one lane per block).
#define ouro ouro_wit
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ouro_verify.h"
#include "cbor_witness.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;
using namespace ouro_rt;

// one lane per block: the count pass; zeros where the block does not slice
__global__ void __launch_bounds__(kBlock) k_witness_count(const uint8_t* __restrict__ raw,
                                                          size_t raw_bytes,
                                                          const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ len, size_t n,
                                                          uint8_t* __restrict__ status,
                                                          uint32_t* __restrict__ ntx,
                                                          uint32_t* __restrict__ nwit) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = ldg8(off + i);
    const uint32_t l0 = (uint32_t)ldg1(len + i);
    uint32_t a = 0, b = 0;
    const uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                           ? (uint8_t)OURO_PACK_ESPAN
                           : cbor::witness_count_one(raw, o0, l0, &a, &b);
    status[i] = st;
    stg1(ntx + i, (int32_t)a);
    stg1(nwit + i, (int32_t)b);
  }
}

// ---- the exclusive scan of ntx and nwit, in two levels ----
// A tile is kScanTile consecutive blocks: kScanPer per thread of one
// workgroup.  Level 1 (k_witness_tile_sums) reduces every tile, level 2
// (k_witness_scan_sums, ONE workgroup) scans the tile sums in place and writes
// the totals, and k_witness_scan_apply scans inside each tile on top of its
// tile's prefix.  2^20 blocks are 1024 tiles: four sums per thread of level 2.
constexpr int kScanPer = 4;
constexpr int kScanTile = kBlock * kScanPer;

// the exclusive prefix of one (a, b) pair per thread over the workgroup's
// kBlock threads, and the workgroup's totals (every thread calls it)
__device__ __forceinline__ void wg_excl_scan(uint64_t* a, uint64_t* b, uint64_t* ta, uint64_t* tb) {
  __shared__ uint64_t sa[kBlock], sb[kBlock];
  const int t = threadIdx.x;
  sa[t] = *a;
  sb[t] = *b;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {  // Hillis-Steele, inclusive
    const uint64_t xa = t >= d ? sa[t - d] : 0, xb = t >= d ? sb[t - d] : 0;
    __syncthreads();
    sa[t] += xa;
    sb[t] += xb;
    __syncthreads();
  }
  *ta = sa[kBlock - 1];
  *tb = sb[kBlock - 1];
  const uint64_t ia = sa[t] - *a, ib = sb[t] - *b;
  __syncthreads();  // (the arrays are reused by the caller's next tile)
  *a = ia;
  *b = ib;
}

// sums[2 k], sums[2 k + 1] = the sums of ntx and nwit over tile k
__global__ void __launch_bounds__(kBlock) k_witness_tile_sums(size_t n,
                                                              const uint32_t* __restrict__ ntx,
                                                              const uint32_t* __restrict__ nwit,
                                                              uint64_t* __restrict__ sums) {
  const size_t tiles = (n + kScanTile - 1) / kScanTile;
  for (size_t k = blockIdx.x; k < tiles; k += gridDim.x) {  // (whole workgroups: the barriers)
    uint64_t a = 0, b = 0, ta, tb;
    for (int q = 0; q < kScanPer; q++) {
      const size_t i = k * kScanTile + (size_t)threadIdx.x * kScanPer + q;
      if (i < n) {
        a += (uint32_t)ldg1(ntx + i);
        b += (uint32_t)ldg1(nwit + i);
      }
    }
    wg_excl_scan(&a, &b, &ta, &tb);
    if (threadIdx.x == 0) {
      stg8(sums + 2 * k, ta);
      stg8(sums + 2 * k + 1, tb);
    }
  }
}

// one workgroup: the tile sums to their exclusive prefixes, in place (each
// thread a run of consecutive tiles); the totals to tx_begin[n], wit_begin[n]
// and rows[0..1] = min(total, capacity): the rows the later kernels read
__global__ void __launch_bounds__(kBlock) k_witness_scan_sums(size_t n, uint64_t* __restrict__ sums,
                                                              uint64_t* __restrict__ tx_begin,
                                                              uint64_t* __restrict__ wit_begin,
                                                              uint64_t tx_cap, uint64_t wit_cap,
                                                              uint64_t* __restrict__ rows) {
  const size_t tiles = (n + kScanTile - 1) / kScanTile;
  const size_t per = (tiles + kBlock - 1) / kBlock;
  const size_t lo = (size_t)threadIdx.x * per < tiles ? (size_t)threadIdx.x * per : tiles;
  const size_t hi = lo + per < tiles ? lo + per : tiles;
  uint64_t a = 0, b = 0, ta, tb;
  for (size_t k = lo; k < hi; k++) {
    a += ldg8(sums + 2 * k);
    b += ldg8(sums + 2 * k + 1);
  }
  wg_excl_scan(&a, &b, &ta, &tb);
  for (size_t k = lo; k < hi; k++) {
    const uint64_t xa = ldg8(sums + 2 * k), xb = ldg8(sums + 2 * k + 1);
    stg8(sums + 2 * k, a);
    stg8(sums + 2 * k + 1, b);
    a += xa;
    b += xb;
  }
  if (threadIdx.x == 0) {
    stg8(tx_begin + n, ta);
    stg8(wit_begin + n, tb);
    stg8(rows, ta < tx_cap ? ta : tx_cap);
    stg8(rows + 1, tb < wit_cap ? tb : wit_cap);
  }
}

// tx_begin[i], wit_begin[i] for i < n: the tile's prefix + the scan inside it
__global__ void __launch_bounds__(kBlock) k_witness_scan_apply(size_t n,
                                                               const uint32_t* __restrict__ ntx,
                                                               const uint32_t* __restrict__ nwit,
                                                               const uint64_t* __restrict__ sums,
                                                               uint64_t* __restrict__ tx_begin,
                                                               uint64_t* __restrict__ wit_begin) {
  const size_t tiles = (n + kScanTile - 1) / kScanTile;
  for (size_t k = blockIdx.x; k < tiles; k += gridDim.x) {
    const size_t i0 = k * kScanTile + (size_t)threadIdx.x * kScanPer;
    uint32_t va[kScanPer], vb[kScanPer];
    uint64_t a = 0, b = 0, ta, tb;
    for (int q = 0; q < kScanPer; q++) {
      va[q] = i0 + q < n ? (uint32_t)ldg1(ntx + i0 + q) : 0u;
      vb[q] = i0 + q < n ? (uint32_t)ldg1(nwit + i0 + q) : 0u;
      a += va[q];
      b += vb[q];
    }
    wg_excl_scan(&a, &b, &ta, &tb);
    a += ldg8(sums + 2 * k);
    b += ldg8(sums + 2 * k + 1);
    for (int q = 0; q < kScanPer; q++) {
      if (i0 + q < n) {
        stg8(tx_begin + i0 + q, a);
        stg8(wit_begin + i0 + q, b);
      }
      a += va[q];
      b += vb[q];
    }
  }
}

// Every row up to the capacities to "not written": a tx span outside the raw
// buffer (k_blake2b256 then writes a zero digest), a witness row of kind
// kWitUnwritten (k_witness_verify then writes zeros) with a zero key, so that the rows of a
// block that did not fit, and those past the totals, read as zero.
constexpr uint8_t kWitUnwritten = 0xff;
__global__ void __launch_bounds__(kBlock) k_witness_clear(size_t tx_cap, size_t wit_cap,
                                                          uint64_t* __restrict__ tx_off,
                                                          uint32_t* __restrict__ tx_len,
                                                          uint32_t* __restrict__ wit_tx,
                                                          uint8_t* __restrict__ kind,
                                                          uint8_t* __restrict__ vk) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < tx_cap; i += nth) {
    stg8(tx_off + i, ~0ull);
    stg1(tx_len + i, 0);
  }
  for (size_t i = tid; i < wit_cap; i += nth) {
    stg1(wit_tx + i, 0);
    kind[i] = kWitUnwritten;
    cbor::zero_bytes(vk + 32 * i, 32);
  }
}

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
// capacity; the row count comes from device memory (rows[1], k_witness_scan_sums).
// The message is the row's transaction id (tx_id row wit_tx - tx_base).  A row nothing was emitted to
// (kWitUnwritten) gets zeros.
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
    if (kind[i] == kWitUnwritten || t >= tx_cap) {  // (t < tx_cap always for an emitted row)
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
// the rows from the row count to the capacity: zeros (a kernel of its own, so
// that the verify kernel's loop is k_ed25519_verify's)
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
// = OURO_WIT_ALL_OK iff the block sliced, fit and n_bad == 0
__global__ void __launch_bounds__(kBlock) k_witness_finish(size_t n, const uint8_t* __restrict__ status,
                                                           const uint64_t* __restrict__ wit_begin,
                                                           const uint8_t* __restrict__ wit_ok,
                                                           uint64_t wit_cap,
                                                           uint8_t* __restrict__ verdict,
                                                           uint32_t* __restrict__ n_bad) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t bad = 0;
    uint8_t v = 0;
    if (status[i] == OURO_PACK_OK) {
      const uint64_t lo = ldg8(wit_begin + i), e = ldg8(wit_begin + i + 1);
      const uint64_t hi = e < wit_cap ? e : wit_cap;
      for (uint64_t r = lo; r < hi; r++) bad += ldg_u8(wit_ok + r) ? 0u : 1u;
      v = bad == 0 ? (uint8_t)OURO_WIT_ALL_OK : (uint8_t)0;
    }
    stg1(n_bad + i, (int32_t)bad);
    verdict[i] = v;
  }
}

static unsigned lane_grid(size_t n) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, 4096));
}

namespace ouro_rt {

size_t witness_scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }

int launch_witness_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                         const uint32_t* len, size_t n, uint8_t* status, uint32_t* ntx,
                         uint32_t* nwit) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_witness_count, dim3(lane_grid(n)), dim3(kBlock), 0, st, raw, raw_bytes, off,
                     len, n, status, ntx, nwit);
  return launch_check();
}

int launch_witness_scan(hipStream_t st, size_t n, const uint32_t* ntx, const uint32_t* nwit,
                        uint64_t* sums, uint64_t* tx_begin, uint64_t* wit_begin, size_t tx_cap,
                        size_t wit_cap, uint64_t* rows) {
  if (n == 0) return OURO_OK;
  const unsigned tiles = (unsigned)std::min<size_t>(witness_scan_tiles(n), 4096);
  hipLaunchKernelGGL(k_witness_tile_sums, dim3(tiles), dim3(kBlock), 0, st, n, ntx, nwit, sums);
  hipLaunchKernelGGL(k_witness_scan_sums, dim3(1), dim3(kBlock), 0, st, n, sums, tx_begin,
                     wit_begin, (uint64_t)tx_cap, (uint64_t)wit_cap, rows);
  hipLaunchKernelGGL(k_witness_scan_apply, dim3(tiles), dim3(kBlock), 0, st, n, ntx, nwit, sums,
                     tx_begin, wit_begin);
  return launch_check();
}

int launch_witness_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off, const uint32_t* len,
                        size_t n, const uint32_t* ntx, const uint32_t* nwit,
                        const uint64_t* tx_begin, const uint64_t* wit_begin, size_t tx_cap,
                        size_t wit_cap, uint64_t tx_base, uint64_t* tx_off, uint32_t* tx_len,
                        uint8_t* vk, uint8_t* sig, uint32_t* wit_tx, uint8_t* kind,
                        uint8_t* status) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_witness_clear, dim3(lane_grid(std::max(tx_cap, wit_cap))), dim3(kBlock), 0,
                     st, tx_cap, wit_cap, tx_off, tx_len, wit_tx, kind, vk);
  const cbor::WitRows rows{tx_off, tx_len, vk, sig, wit_tx, kind, tx_base};
  hipLaunchKernelGGL(k_witness_emit, dim3(lane_grid(n)), dim3(kBlock), 0, st, raw, off, len, n, ntx,
                     nwit, tx_begin, wit_begin, (uint64_t)tx_cap, (uint64_t)wit_cap, rows, status);
  return launch_check();
}

int launch_witness_verify(hipStream_t st, size_t wit_cap, const uint64_t* rows, const uint8_t* vk,
                          const uint8_t* sig, const uint32_t* wit_tx, const uint8_t* tx_id,
                          size_t tx_cap, uint64_t tx_base, uint8_t* kind, uint8_t* wit_ok) {
  if (wit_cap == 0) return OURO_OK;
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, wit_cap, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_witness_verify, dim3(grid), dim3(kBlock), 0, st, rows, vk, sig, wit_tx,
                     tx_id, (uint64_t)tx_cap, tx_base, kind, wit_ok, scr, ds->btab);
  hipLaunchKernelGGL(k_witness_tail, dim3(lane_grid(wit_cap)), dim3(kBlock), 0, st, rows, wit_cap,
                     kind, wit_ok);
  return launch_check();
}

int launch_witness_finish(hipStream_t st, size_t n, const uint8_t* status,
                          const uint64_t* wit_begin, const uint8_t* wit_ok, size_t wit_cap,
                          uint8_t* verdict, uint32_t* n_bad) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_witness_finish, dim3(lane_grid(n)), dim3(kBlock), 0, st, n, status,
                     wit_begin, wit_ok, (uint64_t)wit_cap, verdict, n_bad);
  return launch_check();
}

}  // namespace ouro_rt
