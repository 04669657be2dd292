// kernels_byron_block.hip -- the Byron whole-block integrity kernels
// (cbor_byron_block.h) and their launches (launches.h launch_byron_block_*).
//
// A translation unit of its own, as kernels_witness.hip and kernels_pbft.hip
// are: its copies of the slicers and of the Blake2b routines live in namespace
// ouro_byb, so no symbol is shared with kernels.hip's and every kernel there is
// built exactly as before.  The launches take plain pointers only.
//
// The sequence (byron_block_api.cpp byb_count_scan, byb_rows): count (one lane
// per block), the three-value exclusive scan (scan_excl.h), clear, emit
// (one lane per block, at the rows the scan gave it: no atomics), the leaf
// hashes (one lane per transaction row), the Merkle roots (one lane per
// block), the plain hashes and the ByronDSIGN launch (kernels.hip's
// launch_blake2b and launch_ed over the emitted rows) and finish (one lane per
// block).
#define ouro ouro_byb
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor_byron_block.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"
#include "scan_excl.h"

using namespace ouro;
using namespace ouro_rt;

// one lane per block: the count pass; zeros where the block is not a regular
// block that slices
__global__ void __launch_bounds__(kBlock) k_byron_block_count(
    const uint8_t* __restrict__ raw, size_t raw_bytes, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, size_t n, int64_t magic, uint8_t* __restrict__ status,
    uint32_t* __restrict__ ntx, uint32_t* __restrict__ gather, uint32_t* __restrict__ msg) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = ldg8(off + i);
    const uint32_t l0 = (uint32_t)ldg1(len + i);
    uint32_t a = 0, b = 0, c = 0;
    const uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                           ? (uint8_t)OURO_PACK_ESPAN
                           : cbor::byron_block_count_one(raw, o0, l0, magic, &a, &b, &c);
    status[i] = st;
    stg1(ntx + i, (int32_t)a);
    stg1(gather + i, (int32_t)b);
    stg1(msg + i, (int32_t)c);
  }
}

// every transaction row up to the capacity to "not written": a span outside the
// raw buffer, for which k_byron_leaf_hash writes a zero digest
__global__ void __launch_bounds__(kBlock) k_byron_block_clear(size_t tx_cap,
                                                              uint64_t* __restrict__ tx_off,
                                                              uint32_t* __restrict__ tx_len) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < tx_cap; i += nth) {
    stg8(tx_off + i, cbor::kNoSpan);
    stg1(tx_len + i, 0);
  }
}

// one lane per block: the emit pass of a regular block whose rows fit, at the
// rows the scan gave it (its message at msg + msg_off[i], the scan's begin);
// one that does not fit: OURO_PACK_ECAP.  Every other block's rows: zeros.
struct EmitCaps {
  uint64_t tx, gather, msg;
};
__global__ void __launch_bounds__(kBlock) k_byron_block_emit(
    const uint8_t* __restrict__ raw, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ len, size_t n, int64_t magic, const uint32_t* __restrict__ ntx,
    const uint32_t* __restrict__ gather, const uint32_t* __restrict__ msg,
    const uint64_t* __restrict__ tx_begin, const uint64_t* __restrict__ g_begin, EmitCaps caps,
    cbor::ByronOut o, cbor::BybRows rows, uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    bool emit = status[i] == OURO_PACK_OK;  // (its span was checked by the count pass)
    if (emit) {
      const uint64_t t0 = ldg8(tx_begin + i), g0 = ldg8(g_begin + i), m0 = ldg8(o.msg_off + i);
      const uint32_t a = (uint32_t)ldg1(ntx + i), b = (uint32_t)ldg1(gather + i),
                     c = (uint32_t)ldg1(msg + i);
      if (t0 > caps.tx || caps.tx - t0 < a || g0 > caps.gather || caps.gather - g0 < b ||
          m0 > caps.msg || caps.msg - m0 < c) {
        status[i] = (uint8_t)OURO_PACK_ECAP;
        emit = false;
      } else {
        cbor::byron_block_emit_one(raw, ldg8(off + i), (uint32_t)ldg1(len + i), magic, o, rows, i,
                                   t0, g0, a, b);
      }
    }
    if (!emit) cbor::byron_block_zero_row(o, rows, i);
  }
}

// digest[t] = Blake2b-256(0x00 || raw[tx_off[t] .. + tx_len[t])), one lane per
// transaction row in row order (workgroups of one wave, as k_header_hash).  No
// length-class sort: Byron transactions lie within a few compressions of each
// other, and the rows of a block stay neighbours for k_byron_merkle.  The row
// count comes from device memory (rows[0], the scan).  raw must
// be 4-byte aligned.  A row nothing was emitted to gets zeros.
constexpr int kLeafBlock = 64;
__global__ void __launch_bounds__(kLeafBlock) k_byron_leaf_hash(
    const uint64_t* __restrict__ rows, const uint8_t* __restrict__ raw, size_t raw_bytes,
    const uint64_t* __restrict__ tx_off, const uint32_t* __restrict__ tx_len,
    uint8_t* __restrict__ digest) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const size_t m = (size_t)ldg8(rows);
  for (size_t t = tid; t < m; t += nth) {
    const uint64_t o0 = ldg8(tx_off + t);
    const uint32_t l0 = (uint32_t)ldg1(tx_len + t);
    uint32_t d[8];
    if (o0 > raw_bytes || raw_bytes - o0 < l0) {
#pragma unroll
      for (int k = 0; k < 8; k++) d[k] = 0;
    } else {
      blake2b256_stream_prefixed(d, 0u, 1u, raw + o0, l0);
    }
    stg4(digest + 32 * t, make_int4((int)d[0], (int)d[1], (int)d[2], (int)d[3]));
    stg4(digest + 32 * t + 16, make_int4((int)d[4], (int)d[5], (int)d[6], (int)d[7]));
  }
}

// root[i] = the Merkle root of block i's leaf digests, one lane per block,
// reducing its rows in place: pair neighbours level by level and carry an odd
// last node up unchanged (the recursive definition's tree: its left subtree is
// always a full one).  H("") for a block without transactions; zeros for a
// block nothing was emitted for.
__global__ void __launch_bounds__(kBlock) k_byron_merkle(size_t n, const uint8_t* __restrict__ status,
                                                         const uint32_t* __restrict__ ntx,
                                                         const uint64_t* __restrict__ tx_begin,
                                                         uint8_t* digest, uint8_t* __restrict__ root) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (status[i] == OURO_PACK_OK)
      cbor::byron_merkle_root(d, digest + 32 * ldg8(tx_begin + i), (uint32_t)ldg1(ntx + i));
    store_words(root + 32 * i, d, 2);
  }
}

// one lane per block: the five comparisons of blockMatchesHeader and the merge
// with the signature verdict, the magic rule and the status
//   claimed: n x 128 (root | witnesses | dlg | upd); root, wit: n x 32; seg: 2n x 32
__global__ void __launch_bounds__(kBlock) k_byron_block_finish(
    size_t n, int64_t magic, const uint8_t* __restrict__ status, const uint32_t* __restrict__ ntx,
    const uint32_t* __restrict__ tx_num, const uint64_t* __restrict__ hdr_magic,
    const uint8_t* __restrict__ claimed, const uint8_t* __restrict__ root,
    const uint8_t* __restrict__ wit, const uint8_t* __restrict__ seg,
    const uint8_t* __restrict__ sig_ok, uint8_t* __restrict__ verdict,
    uint8_t* __restrict__ tx_root) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint8_t st = status[i];
    const bool hdr_ok = sig_ok[i] && (magic < 0 || ldg8(hdr_magic + i) == (uint64_t)magic);
    verdict[i] = cbor::byron_block_verdict(st, (uint32_t)ldg1(ntx + i), (uint32_t)ldg1(tx_num + i),
                                           hdr_ok, claimed + 128 * i, root + 32 * i, wit + 32 * i,
                                           seg + 64 * i, seg + 64 * i + 32);
    if (tx_root) {  // (k_byron_merkle left zeros unless the status is OK)
      uint32_t r[8];
      load_words(r, root + 32 * i, 2);
      store_words(tx_root + 32 * i, r, 2);
    }
  }
}

static unsigned lane_grid(size_t n) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((n + kBlock - 1) / kBlock, 4096));
}

namespace ouro_rt {

int launch_byron_block_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes,
                             const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
                             uint8_t* status, uint32_t* ntx, uint32_t* gather, uint32_t* msg) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_byron_block_count, dim3(lane_grid(n)), dim3(kBlock), 0, st, raw, raw_bytes,
                     off, len, n, magic, status, ntx, gather, msg);
  return launch_check();
}

int launch_byron_block_scan(hipStream_t st, size_t n, const uint32_t* ntx, const uint32_t* gather,
                            const uint32_t* msg, uint64_t* sums, uint64_t* tx_begin,
                            uint64_t* g_begin, uint64_t* msg_begin, size_t tx_cap,
                            size_t gather_cap, size_t msg_cap, uint64_t* rows) {
  if (n == 0) return OURO_OK;
  // (ntx, gather bytes, message bytes)
  const scan::Args<3> a{{ntx, gather, msg},
                        {tx_begin, g_begin, msg_begin},
                        {(uint64_t)tx_cap, (uint64_t)gather_cap, (uint64_t)msg_cap}};
  scan::launch<3>(st, n, a, sums, rows);
  return launch_check();
}

int launch_byron_block_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off,
                            const uint32_t* len, size_t n, int64_t magic, const uint32_t* ntx,
                            const uint32_t* gather, const uint32_t* msg, const uint64_t* tx_begin,
                            const uint64_t* g_begin, size_t tx_cap, size_t gather_cap,
                            size_t msg_cap, const ByronBlockDev& d, uint8_t* status) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_byron_block_clear, dim3(lane_grid(tx_cap)), dim3(kBlock), 0, st, tx_cap,
                     d.tx_off, d.tx_len);
  cbor::ByronOut o;
  o.pk = d.pk;
  o.sig = d.sig;
  o.genesis_vk = d.genesis_vk;
  o.delegate_vk = d.delegate_vk;
  o.msg = d.msg;
  o.msg_off = d.msg_off;
  o.magic = d.magic;
  o.msg_len = d.msg_len;
  const cbor::BybRows rows{d.claimed, d.tx_num, d.seg_off, d.seg_len, d.g_off,
                           d.g_len,   d.tx_off, d.tx_len,  d.gather};
  const EmitCaps caps{(uint64_t)tx_cap, (uint64_t)gather_cap, (uint64_t)msg_cap};
  hipLaunchKernelGGL(k_byron_block_emit, dim3(lane_grid(n)), dim3(kBlock), 0, st, raw, off, len, n,
                     magic, ntx, gather, msg, tx_begin, g_begin, caps, o, rows, status);
  return launch_check();
}

int launch_byron_leaf_hash(hipStream_t st, size_t tx_cap, const uint64_t* rows, const uint8_t* raw,
                           size_t raw_bytes, const uint64_t* tx_off, const uint32_t* tx_len,
                           uint8_t* digest) {
  if (tx_cap == 0) return OURO_OK;
  const unsigned blocks =
      (unsigned)std::min<size_t>((tx_cap + kLeafBlock - 1) / kLeafBlock, (size_t)1 << 20);
  hipLaunchKernelGGL(k_byron_leaf_hash, dim3(blocks), dim3(kLeafBlock), 0, st, rows, raw, raw_bytes,
                     tx_off, tx_len, digest);
  return launch_check();
}

int launch_byron_merkle(hipStream_t st, size_t n, const uint8_t* status, const uint32_t* ntx,
                        const uint64_t* tx_begin, uint8_t* digest, uint8_t* root) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_byron_merkle, dim3(lane_grid(n)), dim3(kBlock), 0, st, n, status, ntx,
                     tx_begin, digest, root);
  return launch_check();
}

int launch_byron_block_finish(hipStream_t st, size_t n, int64_t magic, const uint8_t* status,
                              const uint32_t* ntx, const uint32_t* tx_num,
                              const uint64_t* hdr_magic, const uint8_t* claimed,
                              const uint8_t* root, const uint8_t* wit, const uint8_t* seg,
                              const uint8_t* sig_ok, uint8_t* verdict, uint8_t* tx_root) {
  if (n == 0) return OURO_OK;
  hipLaunchKernelGGL(k_byron_block_finish, dim3(lane_grid(n)), dim3(kBlock), 0, st, n, magic, status,
                     ntx, tx_num, hdr_magic, claimed, root, wit, seg, sig_ok, verdict, tx_root);
  return launch_check();
}

}  // namespace ouro_rt
