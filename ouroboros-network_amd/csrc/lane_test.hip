// lane_test.hip -- TEST-ONLY: the lane routines as batch items (lane_items.h)
// on the device, one item per lane.  Every entry takes host arrays, uploads
// them, launches, and copies the results back; tests/test_lane_exact.py
// compares them with exact integer arithmetic, and runs the same items and
// records through the host build (devhost_test.hip dh_lt_*) first.  The chain
// kernels carry the product kernels' launch bounds; the product library does
// not contain this file.
#include <hip/hip_runtime.h>

#include <vector>

#include "lane_items.h"
#include "launch.h"

// k_hdr_dsm's budget (kernels.hip), for the dsm_lane_dsm_launch variant
#ifndef OURO_DSM_WAVES
#define OURO_DSM_WAVES 4
#endif

using namespace ouro;

namespace {

#define LT_TRY(expr)                          \
  do {                                        \
    const hipError_t lt_e = (expr);           \
    if (lt_e != hipSuccess) return (int)lt_e; \
  } while (0)

// device memory freed on return
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  hipError_t upload(const void* src, size_t bytes) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
  }
  hipError_t zeros(size_t bytes) {
    const hipError_t e = alloc(bytes);
    return e != hipSuccess ? e : hipMemset(p, 0, bytes);
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};
int finish_launch() {
  LT_TRY(hipGetLastError());
  LT_TRY(hipDeviceSynchronize());
  return 0;
}

// the fixed-base tables, built on the host as runtime.cpp builds them and kept
// on the device for the life of the process
int dev_table(const int32_t** out, int32_t** slot, size_t words, void (*build)(int32_t*)) {
  if (!*slot) {
    std::vector<int32_t> t(words);
    build(t.data());
    int32_t* d = nullptr;
    LT_TRY(hipMalloc(&d, words * sizeof(int32_t)));
    const hipError_t e = hipMemcpy(d, t.data(), words * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return (int)e;
    }
    *slot = d;
  }
  *out = *slot;
  return 0;
}
int dev_btab(const int32_t** out) {
  static int32_t* d = nullptr;
  return dev_table(out, &d, kBTabWords, build_btab);
}
int dev_ubtab(const int32_t** out) {
  static int32_t* d = nullptr;
  return dev_table(out, &d, kUBTabWords, build_ubtab);
}

// ---- the fixed-record items ----------------------------------------------------
template <int kOp>
__global__ void __launch_bounds__(kBlock) k_lt_op(int n, const uint32_t* __restrict__ in,
                                                  uint32_t* __restrict__ out, int param) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  lt::item<kOp>(in + (size_t)i * lt::kIn, out + (size_t)i * lt::kOut, param);
}
template <int kOp>
int launch_op(int op, int n, const uint32_t* in, uint32_t* out, int param) {
  if (op == kOp) {
    hipLaunchKernelGGL(k_lt_op<kOp>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0,
                       n, in, out, param);
    return 0;
  }
  if constexpr (kOp + 1 < lt::kOps) return launch_op<kOp + 1>(op, n, in, out, param);
  return -1;
}

__global__ void __launch_bounds__(kBlock) k_lt_sha512(int n, const uint32_t* __restrict__ pre,
                                                      const uint8_t* __restrict__ buf,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ len,
                                                      uint32_t* __restrict__ out) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  lt::sha512_item(pre + 16 * (size_t)i, buf + off[i], len[i], out + 16 * (size_t)i);
}

// ---- the chains ------------------------------------------------------------------
// Item i runs on global thread i * stride; every other thread returns before
// the chain, so with stride 64 an item is alone in its wave (wave_max_small
// sees its window count only) and with stride 1 the wave is packed.  -1: no item.
__device__ __forceinline__ long chain_item(int n, int stride) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (t % (size_t)stride) return -1;
  const size_t i = t / (size_t)stride;
  return i < (size_t)n ? (long)i : -1;
}
unsigned chain_blocks(int n, int stride) {
  return (unsigned)(((size_t)n * (size_t)stride + kBlock - 1) / kBlock);
}

__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_lt_ed(int n, int stride, int phase,
                                                             const uint32_t* __restrict__ in,
                                                             uint32_t* __restrict__ out,
                                                             int32_t* scratch,
                                                             const int32_t* __restrict__ btab) {
  const long i = chain_item(n, stride);
  if (i < 0) return;
  const Slot lane = slot_of(scratch, (size_t)i, kSlotWords);
  uint32_t* o = out + (size_t)i * lt::kChainOut;
  lt::ed_setup(in + (size_t)i * lt::kEdIn, o, lane, btab, phase);
  if (phase == kPhaseAll) lt::chain_finish(o, lane);
}
// the chain alone from the cfg word the pre phase left, at k_hdr_dsm's budget
__global__ void __launch_bounds__(kBlock, OURO_DSM_WAVES) k_lt_dsm(int n, int stride,
                                                                  int32_t* scratch,
                                                                  const int32_t* __restrict__ btab) {
  const long i = chain_item(n, stride);
  if (i < 0) return;
  const Slot lane = slot_of(scratch, (size_t)i, kSlotWords);
  dsm_lane_dsm_launch(lane, btab, (uint32_t)ldg1(lane.word(kSlotCfg)));
}
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_lt_finish(int n, int stride,
                                                                 uint32_t* __restrict__ out,
                                                                 int32_t* scratch) {
  const long i = chain_item(n, stride);
  if (i < 0) return;
  lt::chain_finish(out + (size_t)i * lt::kChainOut, slot_of(scratch, (size_t)i, kSlotWords));
}
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_lt_u(int n, int stride,
                                                            const uint32_t* __restrict__ in,
                                                            uint32_t* __restrict__ out,
                                                            int32_t* scratch,
                                                            const int32_t* __restrict__ btab) {
  const long i = chain_item(n, stride);
  if (i < 0) return;
  lt::u_item(in + (size_t)i * lt::kUIn, out + (size_t)i * lt::kChainOut,
             slot_of(scratch, (size_t)i, kSlotWords), btab);
}
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_lt_v(int n, int stride,
                                                            const uint32_t* __restrict__ in,
                                                            uint32_t* __restrict__ out,
                                                            int32_t* scratch,
                                                            const int32_t* __restrict__ btab) {
  const long i = chain_item(n, stride);
  if (i < 0) return;
  lt::v_item(in + (size_t)i * lt::kVIn, out + (size_t)i * lt::kChainOut,
             slot_of(scratch, (size_t)i, kSlotWords), btab);
}

// ---- U from the per-key tables: key k on one lane, then (key, window) on one
// lane, as k_vrfkey_base and k_vrfkey_fill run them, then the items
__global__ void __launch_bounds__(64) k_lt_vrfkey_base(int nkeys, const uint8_t* __restrict__ keys,
                                                       uint8_t* __restrict__ kflag, int32_t* kbase) {
  const int k = (int)(blockIdx.x * 64 + threadIdx.x);
  if (k >= nkeys) return;
  uint32_t p[8];
  ld_words(p, keys + 32 * (size_t)k, 2);
  kflag[k] = vrfkey_base(p, kbase + (size_t)k * kYBaseWords) ? 1 : 0;
}
__global__ void __launch_bounds__(64) k_lt_vrfkey_fill(int nkeys, const int32_t* __restrict__ kbase,
                                                       int32_t* ktab) {
  // consecutive lanes take one window of consecutive keys (k_vrfkey_fill)
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t blk = t / (64 * (size_t)kYWindows), r = t % (64 * (size_t)kYWindows);
  const size_t k = blk * 64 + (r & 63);
  const int j = (int)(r >> 6);
  if (k >= (size_t)nkeys) return;
  vrfkey_fill(kbase + k * kYBaseWords, ktab + k * kYKeyWords, j);
}
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_lt_u_table(
    ouro_tpraos_batch b, int stride, const uint32_t* __restrict__ kidx,
    const uint8_t* __restrict__ kflag, const int32_t* ktab, const int32_t* __restrict__ ubtab,
    uint32_t* __restrict__ out, int32_t* scratch, int32_t* res_buf) {
  const long i = chain_item((int)b.n, stride);
  if (i < 0) return;
  const uint32_t k = kidx[i];
  lt::u_table_item(b, (size_t)i, kflag[k] != 0, out + (size_t)i * lt::kChainOut,
                   slot_of(scratch, (size_t)i, kSlotWords), slot_of(res_buf, (size_t)i, kResWords),
                   ubtab, ktab + (size_t)k * kYKeyWords);
}

// n * stride threads at most; the items' records at most a few MB
bool chain_args_ok(int n, int stride) { return n > 0 && n <= (1 << 16) && stride > 0 && stride <= 64; }

}  // namespace

extern "C" {

// The entries return 0, -1 on bad arguments, or the HIP error code.

// item `op` (lane_items.h Op) over n records of kIn words; kOut words each out
int lt_op(int op, int n, const uint32_t* in, uint32_t* out, int param) {
  if (n <= 0 || n > (1 << 20) || !in || !out || op < 0 || op >= lt::kOps) return -1;
  DevBuf d_in, d_out;
  LT_TRY(d_in.upload(in, sizeof(uint32_t) * lt::kIn * (size_t)n));
  LT_TRY(d_out.zeros(sizeof(uint32_t) * lt::kOut * (size_t)n));
  if (launch_op<0>(op, n, d_in.as<uint32_t>(), d_out.as<uint32_t>(), param)) return -1;
  if (const int rc = finish_launch()) return rc;
  LT_TRY(hipMemcpy(out, d_out.p, sizeof(uint32_t) * lt::kOut * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
// SHA-512(pre_i (64 B) || buf[off_i .. off_i + len_i)), 64 bytes each out.  The
// tail's dword loads reach at most 3 bytes before a message and 3 past its
// end: the caller pads buf, and a message must lie inside it.
int lt_sha512(int n, const uint8_t* pre, const uint8_t* buf, size_t buflen, const uint32_t* off,
              const uint32_t* len, uint8_t* out) {
  if (n <= 0 || n > (1 << 20) || !pre || !buf || !off || !len || !out) return -1;
  for (int i = 0; i < n; i++)
    if (off[i] < 4 || (size_t)off[i] + len[i] + 4 > buflen) return -1;
  DevBuf d_pre, d_buf, d_off, d_len, d_out;
  LT_TRY(d_pre.upload(pre, 64 * (size_t)n));
  LT_TRY(d_buf.upload(buf, buflen));
  LT_TRY(d_off.upload(off, sizeof(uint32_t) * (size_t)n));
  LT_TRY(d_len.upload(len, sizeof(uint32_t) * (size_t)n));
  LT_TRY(d_out.zeros(64 * (size_t)n));
  hipLaunchKernelGGL(k_lt_sha512, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, n,
                     d_pre.as<uint32_t>(), d_buf.as<uint8_t>(), d_off.as<uint32_t>(),
                     d_len.as<uint32_t>(), d_out.as<uint32_t>());
  if (const int rc = finish_launch()) return rc;
  LT_TRY(hipMemcpy(out, d_out.p, 64 * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
// ED over n records of kEdIn words, kChainOut words each out.  variant 0:
// one kernel, the chain through dsm_lane; variant 1: the pre phase, the chain
// through dsm_lane_dsm_launch in a launch of its own at k_hdr_dsm's budget,
// and the finish -- the split header kernel's three launches.
int lt_ed(int n, int stride, int variant, const uint32_t* in, uint32_t* out) {
  if (!chain_args_ok(n, stride) || !in || !out) return -1;
  const int32_t* btab = nullptr;
  if (const int rc = dev_btab(&btab)) return rc;
  DevBuf d_in, d_out, d_scr;
  LT_TRY(d_in.upload(in, sizeof(uint32_t) * lt::kEdIn * (size_t)n));
  LT_TRY(d_out.zeros(sizeof(uint32_t) * lt::kChainOut * (size_t)n));
  LT_TRY(d_scr.zeros(sizeof(int32_t) * slot_region_words((size_t)n, kSlotWords)));
  const dim3 grid(chain_blocks(n, stride)), block(kBlock);
  hipLaunchKernelGGL(k_lt_ed, grid, block, 0, 0, n, stride, variant ? (int)kPhasePre : (int)kPhaseAll,
                     d_in.as<uint32_t>(), d_out.as<uint32_t>(), d_scr.as<int32_t>(), btab);
  if (variant) {
    hipLaunchKernelGGL(k_lt_dsm, grid, block, 0, 0, n, stride, d_scr.as<int32_t>(), btab);
    hipLaunchKernelGGL(k_lt_finish, grid, block, 0, 0, n, stride, d_out.as<uint32_t>(),
                       d_scr.as<int32_t>());
  }
  if (const int rc = finish_launch()) return rc;
  LT_TRY(hipMemcpy(out, d_out.p, sizeof(uint32_t) * lt::kChainOut * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
// U (which = 0: kUIn words per record) / V (1: kVIn), kChainOut words each out
static int lt_uv(int which, int n, int stride, const uint32_t* in, uint32_t* out) {
  if (!chain_args_ok(n, stride) || !in || !out) return -1;
  const int32_t* btab = nullptr;
  if (const int rc = dev_btab(&btab)) return rc;
  const int in_words = which ? lt::kVIn : lt::kUIn;
  DevBuf d_in, d_out, d_scr;
  LT_TRY(d_in.upload(in, sizeof(uint32_t) * in_words * (size_t)n));
  LT_TRY(d_out.zeros(sizeof(uint32_t) * lt::kChainOut * (size_t)n));
  LT_TRY(d_scr.zeros(sizeof(int32_t) * slot_region_words((size_t)n, kSlotWords)));
  const dim3 grid(chain_blocks(n, stride)), block(kBlock);
  if (which)
    hipLaunchKernelGGL(k_lt_v, grid, block, 0, 0, n, stride, d_in.as<uint32_t>(),
                       d_out.as<uint32_t>(), d_scr.as<int32_t>(), btab);
  else
    hipLaunchKernelGGL(k_lt_u, grid, block, 0, 0, n, stride, d_in.as<uint32_t>(),
                       d_out.as<uint32_t>(), d_scr.as<int32_t>(), btab);
  if (const int rc = finish_launch()) return rc;
  LT_TRY(hipMemcpy(out, d_out.p, sizeof(uint32_t) * lt::kChainOut * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
int lt_u(int n, int stride, const uint32_t* in, uint32_t* out) { return lt_uv(0, n, stride, in, out); }
int lt_v(int n, int stride, const uint32_t* in, uint32_t* out) { return lt_uv(1, n, stride, in, out); }
// U from the tables of nkeys keys (32 bytes each): item i from the table of
// key kidx[i] with the c and s of its 80-byte proof; kChainOut words each out
int lt_u_table(int nkeys, const uint8_t* keys, int n, const uint32_t* kidx, const uint8_t* proofs,
               int stride, uint32_t* out) {
  if (nkeys <= 0 || nkeys > 256 || !chain_args_ok(n, stride) || !keys || !kidx || !proofs || !out)
    return -1;
  for (int i = 0; i < n; i++)
    if (kidx[i] >= (uint32_t)nkeys) return -1;
  const int32_t* ubtab = nullptr;
  if (const int rc = dev_ubtab(&ubtab)) return rc;
  DevBuf d_keys, d_flag, d_base, d_tab, d_kidx, d_proofs, d_out, d_scr, d_res;
  LT_TRY(d_keys.upload(keys, 32 * (size_t)nkeys));
  LT_TRY(d_flag.zeros((size_t)nkeys));
  LT_TRY(d_base.zeros(sizeof(int32_t) * kYBaseWords * (size_t)nkeys));
  LT_TRY(d_tab.zeros(sizeof(int32_t) * kYKeyWords * (size_t)nkeys));
  LT_TRY(d_kidx.upload(kidx, sizeof(uint32_t) * (size_t)n));
  LT_TRY(d_proofs.upload(proofs, 80 * (size_t)n));
  LT_TRY(d_out.zeros(sizeof(uint32_t) * lt::kChainOut * (size_t)n));
  LT_TRY(d_scr.zeros(sizeof(int32_t) * slot_region_words((size_t)n, kSlotWords)));
  LT_TRY(d_res.zeros(sizeof(int32_t) * slot_region_words((size_t)n, kResWords)));
  const unsigned kblocks = (unsigned)((nkeys + 63) / 64);
  hipLaunchKernelGGL(k_lt_vrfkey_base, dim3(kblocks), dim3(64), 0, 0, nkeys, d_keys.as<uint8_t>(),
                     d_flag.as<uint8_t>(), d_base.as<int32_t>());
  hipLaunchKernelGGL(k_lt_vrfkey_fill, dim3(kblocks * kYWindows), dim3(64), 0, 0, nkeys,
                     d_base.as<int32_t>(), d_tab.as<int32_t>());
  ouro_tpraos_batch b{};
  b.n = (size_t)n;
  b.eta_proof = d_proofs.as<uint8_t>();
  hipLaunchKernelGGL(k_lt_u_table, dim3(chain_blocks(n, stride)), dim3(kBlock), 0, 0, b, stride,
                     d_kidx.as<uint32_t>(), d_flag.as<uint8_t>(), d_tab.as<int32_t>(), ubtab,
                     d_out.as<uint32_t>(), d_scr.as<int32_t>(), d_res.as<int32_t>());
  if (const int rc = finish_launch()) return rc;
  LT_TRY(hipMemcpy(out, d_out.p, sizeof(uint32_t) * lt::kChainOut * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}
}
