// scan_excl.h -- the two-level exclusive scan of kVals count arrays over n
// items, written once as a template: kernels_witness.hip and
// kernels_byron_witness.hip instantiate it with two values,
// kernels_byron_block.hip with three.  Device code of the unit that includes
// it, inside that unit's renamed namespace; needs launch.h's kBlock.  The host
// units size its work from launches.h (kScanTile, scan_tiles, scan_rows_words).
//
// A tile is kScanTile consecutive items: kScanPer per thread of one workgroup.
// Level 1 (k_scan_tile_sums) reduces every tile, level 2 (k_scan_sums, ONE
// workgroup) scans the tile sums in place and writes the totals, and
// k_scan_apply scans inside each tile on top of its tile's prefix.  2^20 items
// are 1024 tiles: four sums per thread of level 2.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"
#include "launches.h"

namespace ouro {
namespace scan {

constexpr int kScanPer = 4;
constexpr int kScanTile = kBlock * kScanPer;
static_assert(kScanTile == ouro_rt::kScanTile, "launches.h sizes the tile sums by its own kScanTile");

// cnt[q]: n counts; begin[q]: n + 1 (begin[q][n] = the total); cap[q]: the
// capacity rows[q] = min(total, cap[q]) is cut at, rows[kVals + q] = the total
template <int kVals>
struct Args {
  const uint32_t* cnt[kVals];
  uint64_t* begin[kVals];
  uint64_t cap[kVals];
};

// the exclusive prefix of one kVals-tuple per thread over the workgroup's
// kBlock threads, and the workgroup's totals (every thread calls it)
template <int kVals>
__device__ __forceinline__ void wg_excl_scan(uint64_t v[kVals], uint64_t tot[kVals]) {
  __shared__ uint64_t s[kVals][kBlock];
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kVals; q++) s[q][t] = v[q];
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {  // Hillis-Steele, inclusive
    uint64_t x[kVals];
#pragma unroll
    for (int q = 0; q < kVals; q++) x[q] = t >= d ? s[q][t - d] : 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kVals; q++) s[q][t] += x[q];
    __syncthreads();
  }
  uint64_t ex[kVals];
#pragma unroll
  for (int q = 0; q < kVals; q++) {
    tot[q] = s[q][kBlock - 1];
    ex[q] = s[q][t] - v[q];
  }
  __syncthreads();  // (the arrays are reused by the caller's next tile)
#pragma unroll
  for (int q = 0; q < kVals; q++) v[q] = ex[q];
}

// sums[kVals k + q] = the sum of cnt[q] over tile k
template <int kVals>
__global__ void __launch_bounds__(kBlock) k_scan_tile_sums(size_t n, Args<kVals> a,
                                                           uint64_t* __restrict__ sums) {
  const size_t nt = (n + kScanTile - 1) / kScanTile;
  for (size_t k = blockIdx.x; k < nt; k += gridDim.x) {  // (whole workgroups: the barriers)
    uint64_t v[kVals], tot[kVals];
#pragma unroll
    for (int q = 0; q < kVals; q++) v[q] = 0;
    for (int p = 0; p < kScanPer; p++) {
      const size_t i = k * kScanTile + (size_t)threadIdx.x * kScanPer + p;
      if (i < n) {
#pragma unroll
        for (int q = 0; q < kVals; q++) v[q] += (uint32_t)ldg1(a.cnt[q] + i);
      }
    }
    wg_excl_scan<kVals>(v, tot);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < kVals; q++) stg8(sums + kVals * k + q, tot[q]);
    }
  }
}

// one workgroup: the tile sums to their exclusive prefixes, in place (each
// thread a run of consecutive tiles); the totals to begin[q][n] and to rows
template <int kVals>
__global__ void __launch_bounds__(kBlock) k_scan_sums(size_t n, Args<kVals> a,
                                                      uint64_t* __restrict__ sums,
                                                      uint64_t* __restrict__ rows) {
  const size_t nt = (n + kScanTile - 1) / kScanTile;
  const size_t per = (nt + kBlock - 1) / kBlock;
  const size_t lo = (size_t)threadIdx.x * per < nt ? (size_t)threadIdx.x * per : nt;
  const size_t hi = lo + per < nt ? lo + per : nt;
  uint64_t v[kVals], tot[kVals];
#pragma unroll
  for (int q = 0; q < kVals; q++) v[q] = 0;
  for (size_t k = lo; k < hi; k++) {
#pragma unroll
    for (int q = 0; q < kVals; q++) v[q] += ldg8(sums + kVals * k + q);
  }
  wg_excl_scan<kVals>(v, tot);
  for (size_t k = lo; k < hi; k++) {
#pragma unroll
    for (int q = 0; q < kVals; q++) {
      const uint64_t x = ldg8(sums + kVals * k + q);
      stg8(sums + kVals * k + q, v[q]);
      v[q] += x;
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kVals; q++) {
      stg8(a.begin[q] + n, tot[q]);
      stg8(rows + q, tot[q] < a.cap[q] ? tot[q] : a.cap[q]);
      stg8(rows + kVals + q, tot[q]);
    }
  }
}

// begin[q][i] for i < n: the tile's prefix + the scan inside it
template <int kVals>
__global__ void __launch_bounds__(kBlock) k_scan_apply(size_t n, Args<kVals> a,
                                                       const uint64_t* __restrict__ sums) {
  const size_t nt = (n + kScanTile - 1) / kScanTile;
  for (size_t k = blockIdx.x; k < nt; k += gridDim.x) {
    const size_t i0 = k * kScanTile + (size_t)threadIdx.x * kScanPer;
    uint32_t c[kVals][kScanPer];
    uint64_t v[kVals], tot[kVals];
#pragma unroll
    for (int q = 0; q < kVals; q++) {
      v[q] = 0;
#pragma unroll
      for (int p = 0; p < kScanPer; p++) {
        c[q][p] = i0 + p < n ? (uint32_t)ldg1(a.cnt[q] + i0 + p) : 0u;
        v[q] += c[q][p];
      }
    }
    wg_excl_scan<kVals>(v, tot);
#pragma unroll
    for (int q = 0; q < kVals; q++) {
      v[q] += ldg8(sums + kVals * k + q);
#pragma unroll
      for (int p = 0; p < kScanPer; p++) {
        if (i0 + p < n) stg8(a.begin[q] + i0 + p, v[q]);
        v[q] += c[q][p];
      }
    }
  }
}

// the three launches on `st` (n > 0); sums: kVals * scan_tiles(n) words, rows:
// scan_rows_words(kVals)
template <int kVals>
inline void launch(hipStream_t st, size_t n, const Args<kVals>& a, uint64_t* sums, uint64_t* rows) {
  const unsigned nt = (unsigned)std::min<size_t>(ouro_rt::scan_tiles(n), 4096);
  hipLaunchKernelGGL(k_scan_tile_sums<kVals>, dim3(nt), dim3(kBlock), 0, st, n, a, sums);
  hipLaunchKernelGGL(k_scan_sums<kVals>, dim3(1), dim3(kBlock), 0, st, n, a, sums, rows);
  hipLaunchKernelGGL(k_scan_apply<kVals>, dim3(nt), dim3(kBlock), 0, st, n, a, sums);
}

}  // namespace scan
}  // namespace ouro
