// kernels_byron_witness.hip -- the Byron transaction-witness kernels
// (cbor_byron_witness.h) and their launches (launches.h launch_byron_witness_*).
//
// A translation unit of its own, as kernels_witness.hip and
// kernels_byron_block.hip are: k_byron_witness_verify is another user of
// verify.h's lane routines, and its copies (and those of the slicers) live in
// namespace ouro_byw, so no symbol is shared with the other units' and every
// kernel there is built exactly as before.  The launches take plain pointers
// only, one struct of them (launches.h WitnessDev): no type of the renamed
// namespace crosses to the host units.
//
// The sequence (witness_flow.h count_scan, rows): count (one lane per block),
// the two-value exclusive scan (scan_excl.h), clear, emit (one lane per block,
// at the rows the scan gave it: no atomics), the tx ids (kernels.hip's
// launch_blake2b over the emitted spans), verify (one lane per witness row, the
// row count read from device memory, the signed message built in the lane),
// the tail and finish (one lane per block).  Count, clear, tail and finish are
// witness_kernels.h's, shared with kernels_witness.hip; emit and verify are
// this era's own.
#define ouro ouro_byw
#include <hip/hip_runtime.h>

#include "../../include/ouro_verify.h"
#include "cbor_byron_witness.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"
#include "witness_kernels.h"

using namespace ouro;
using namespace ouro_rt;

// the era trait of witness_kernels.h
struct ByronWit {
  static constexpr int kKeyBytes = 64;
  static constexpr uint8_t kAllOk = OURO_BYW_ALL_OK;
  static constexpr bool kEbbOk = true;
  static __device__ __forceinline__ uint8_t count_one(const uint8_t* raw, uint64_t base,
                                                      uint32_t len, uint32_t* ntx, uint32_t* nwit) {
    return cbor::byron_witness_count_one(raw, base, len, ntx, nwit);
  }
};

// one lane per block: the emit pass of a sliced block whose rows fit, at the
// rows the scan gave it, and the magic its messages use (the configured one,
// or the header's own field); one that does not fit: OURO_PACK_ECAP, nothing
// written
__global__ void __launch_bounds__(kBlock) k_byron_witness_emit(
    const uint8_t* __restrict__ raw, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, size_t n, int64_t magic_cfg,
    const uint32_t* __restrict__ ntx, const uint32_t* __restrict__ nwit,
    const uint64_t* __restrict__ tx_begin, const uint64_t* __restrict__ wit_begin, uint64_t tx_cap,
    uint64_t wit_cap, cbor::BywRows rows, uint64_t* __restrict__ magic,
    uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint64_t m = 0;
    if (status[i] == OURO_PACK_OK) {  // (its span was checked by the count pass)
      const uint64_t t0 = ldg8(tx_begin + i), w0 = ldg8(wit_begin + i);
      const uint32_t a = (uint32_t)ldg1(ntx + i), b = (uint32_t)ldg1(nwit + i);
      if (t0 > tx_cap || tx_cap - t0 < a || w0 > wit_cap || wit_cap - w0 < b) {
        status[i] = (uint8_t)OURO_PACK_ECAP;
      } else {
        cbor::byron_witness_emit_one(raw, ldg8(off + i), (uint32_t)ldg1(len + i), rows, t0, w0, a,
                                     b, &m);
        if (magic_cfg >= 0) m = (uint64_t)magic_cfg;
      }
    }
    stg8(magic + i, m);
  }
}

// The tail of the SHA-512 input R || A || M of a Byron witness: M's 4 to 8
// prefix bytes (cbor_byron_witness.h byron_witness_prefix) from registers, then
// the 32 id bytes as four big-endian words loaded once from the 16-byte
// aligned tx_id row.  64 + 36 .. 40 bytes are always one SHA-512 block, so
// every word_be position is a compile-time multiple of 8 in the static block.
struct ShaByronTxTail {
  uint64_t pre;    // the prefix, left-aligned
  uint32_t pl;     // its length, 4 .. 8
  uint64_t id[4];  // the id, big-endian words
  OURO_FI uint32_t tail(uint32_t q) const {
    if (q < pl) return (uint32_t)(pre >> (56 - 8 * q)) & 0xffu;
    const uint32_t k = q - pl;
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) w = (k >> 3) == (uint32_t)j ? id[j] : w;
    return (uint32_t)(w >> (56 - 8 * (k & 7))) & 0xffu;
  }
  // bytes q .. q + 7 (q a multiple of 8; bytes at or beyond the end are zero):
  // word 0 is the prefix and the id's first 8 - pl bytes, word j the id's bytes
  // 8 j - pl onwards
  OURO_FI uint64_t word_be(uint32_t q, uint32_t) const {
    const uint32_t j = q >> 3, r = 8 * (8 - pl);  // r: 0 .. 32
    uint64_t hi = 0, lo = 0;                      // hi = word j - 1 of (pre, id...), lo = word j
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const uint64_t wk = k == 0 ? pre : id[k - 1], wn = k < 4 ? id[k] : 0;
      hi = j == (uint32_t)k ? wk : hi;
      lo = j == (uint32_t)k ? wn : lo;
    }
    if (j == 0) return r ? hi | (lo >> (64 - r)) : hi;  // (pre's unused low bytes are zero)
    return r ? (hi << r) | (lo >> (64 - r)) : hi;
  }
};

// One lane per witness row around ed25519_verify_lane (byron = true), with
// k_witness_verify's launch bounds, scratch slots and B table.  The grid is
// sized from the capacity; the row count comes from device memory (rows[1],
// the scan).  The message is built in the lane from the row's kind, its
// block's magic (blk: the row's block, found from wit_begin by bisection) and
// its transaction id (tx_id row wit_tx - tx_base).  A row nothing was emitted
// to (wit::kUnwritten) gets zeros.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_byron_witness_verify(
    const uint64_t* __restrict__ rows, const uint8_t* __restrict__ vk,
    const uint8_t* __restrict__ sig, const uint32_t* __restrict__ wit_tx,
    const uint8_t* __restrict__ tx_id, uint64_t tx_cap, uint64_t tx_base,
    const uint64_t* __restrict__ wit_begin, size_t nblk, const uint64_t* __restrict__ magic,
    uint8_t* __restrict__ kind, uint8_t* __restrict__ wit_ok, int32_t* scratch,
    const int32_t* __restrict__ btab) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  const size_t n = (size_t)ldg8(rows + 1);
  for (size_t i = tid; i < n; i += nth) {
    // wit_tx is the global row; tx_id holds this call's rows, the first tx_base
    const uint64_t t = (uint64_t)(uint32_t)ldg1(wit_tx + i) - tx_base;
    const uint8_t kd = kind[i];
    if (kd == wit::kUnwritten || t >= tx_cap) {  // (t < tx_cap always for an emitted row)
      kind[i] = 0;
      wit_ok[i] = 0;
      continue;
    }
    // the block that owns row i: the last b with wit_begin[b] <= i (an emitted
    // row lies inside its block's range, and begins only grow)
    size_t lo = 0, hi = nblk;
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      if (ldg8(wit_begin + mid) <= (uint64_t)i) lo = mid; else hi = mid;
    }
    uint32_t s[16], p[8];
    load_words(s, sig + 64 * i, 4);
    load_words(p, vk + 64 * i, 2);
    ShaByronTxTail m;
    m.pre = cbor::byron_witness_prefix(kd, ldg8(magic + lo), &m.pl);
    uint32_t w[8];
    load_words(w, tx_id + 32 * t, 2);
#pragma unroll
    for (int k = 0; k < 4; k++)
      m.id[k] = ((uint64_t)__builtin_bswap32(w[2 * k]) << 32) | __builtin_bswap32(w[2 * k + 1]);
    const bool ok = ed25519_verify_lane(s, p, m, m.pl + 32, lane, btab, true);
    wit_ok[i] = ok ? 1 : 0;
  }
}

namespace ouro_rt {

int launch_byron_witness_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes,
                               const uint64_t* off, const uint32_t* len, size_t n, uint8_t* status,
                               uint32_t* ntx, uint32_t* nwit) {
  return wit::launch_count<ByronWit>(st, raw, raw_bytes, off, len, n, status, ntx, nwit);
}

int launch_byron_witness_scan(hipStream_t st, size_t n, const WitnessDev& d) {
  return wit::launch_scan(st, n, d);
}

int launch_byron_witness_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off,
                              const uint32_t* len, size_t n, int64_t magic_cfg, const WitnessDev& d,
                              uint8_t* status) {
  if (n == 0) return OURO_OK;
  wit::launch_clear<ByronWit>(st, d);
  const cbor::BywRows rows{d.tx_off, d.tx_len, d.vk, d.sig, d.wit_tx, d.kind, d.tx_base};
  hipLaunchKernelGGL(k_byron_witness_emit, dim3(wit::lane_grid(n)), dim3(kBlock), 0, st, raw, off,
                     len, n, magic_cfg, d.ntx, d.nwit, d.tx_begin, d.wit_begin, (uint64_t)d.tx_cap,
                     (uint64_t)d.wit_cap, rows, d.magic, status);
  return launch_check();
}

int launch_byron_witness_verify(hipStream_t st, size_t n, const WitnessDev& d) {
  if (d.wit_cap == 0 || n == 0) return OURO_OK;
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, d.wit_cap, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_byron_witness_verify, dim3(grid), dim3(kBlock), 0, st, d.rows, d.vk, d.sig,
                     d.wit_tx, d.tx_id, (uint64_t)d.tx_cap, d.tx_base, d.wit_begin, n, d.magic,
                     d.kind, d.wit_ok, scr, ds->btab);
  wit::launch_tail(st, d);
  return launch_check();
}

int launch_byron_witness_finish(hipStream_t st, size_t n, const uint8_t* status,
                                const WitnessDev& d, uint8_t* verdict, uint32_t* n_bad) {
  return wit::launch_finish<ByronWit>(st, n, status, d, verdict, n_bad);
}

}  // namespace ouro_rt
