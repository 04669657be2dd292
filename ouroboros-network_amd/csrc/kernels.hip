// kernels.hip -- the gfx950 kernels and their launches (launches.h).  The host
// runtime and the C ABI are the host units (runtime.cpp, api_batch.cpp,
// raw_pipe.cpp, plan.cpp, multi.cpp); they reach a kernel only through the
// launch functions at the end of this file.
//
// One item per lane, 256-thread workgroups, grid-stride over the batch with a
// grid capped at the resident capacity the occupancy API reports, so the
// per-lane scratch slots (verify.h) are bounded by the grid, not the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "blake2b_stream.h"
#include "cbor_block.h"
#include "cbor_byron.h"
#include "host_path.h"
#include "knobs.h"
#include "launch.h"
#include "leader.h"
#include "task_pool.h"
#include "tpraos.h"
#include "vrfkey_ws.h"
#define OURO_KC_FN OURO_FI  // the directory's routines run in the kernels here
#include "key_cache.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;
using namespace ouro_rt;


// ---------------------------------------------------------------- kernels ----

__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_ed25519_verify(
    size_t n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
    const uint32_t* __restrict__ msg_len, uint8_t* __restrict__ verdict, int32_t* scratch,
    const int32_t* __restrict__ btab, uint32_t byron) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  for (size_t i = tid; i < n; i += nth) {
    uint32_t s[16], p[8];
    load_words(s, sig + 64 * i, 4);
    load_words(p, pk + 32 * i, 2);
    const bool ok = ed25519_verify_lane(s, p, ShaGlobalTail{msg + msg_off[i]}, msg_len[i], lane,
                                        btab, byron != 0);
    verdict[i] = ok ? 1 : 0;
  }
}

__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_vrf03_verify(
    size_t n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ proof,
    const uint8_t* __restrict__ alpha, const uint64_t* __restrict__ alpha_off,
    const uint32_t* __restrict__ alpha_len, uint8_t* __restrict__ beta,
    uint8_t* __restrict__ verdict, int32_t* scratch, const int32_t* __restrict__ btab,
    uint32_t flags) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  for (size_t i = tid; i < n; i += nth) {
    uint32_t p[8], pi[20], b[16];
    load_words(p, pk + 32 * i, 2);
    load_words(pi, proof + 80 * i, 5);
    bool ok = vrf03_verify_lane(b, p, pi, ShaGlobalTail{alpha + alpha_off[i]}, alpha_len[i], lane, btab);
    if ((flags & OURO_VRF_STRICT_S) && !sc_is_canonical(pi + 12)) ok = false;  // App. B.3
#pragma unroll
    for (int k = 0; k < 16; k++) b[k] = ok ? b[k] : 0u;
    store_words(beta + 64 * i, b, 4);
    verdict[i] = ok ? 1 : 0;
  }
}

// OURO_KES_STAGE=1: the leaf message's tail (the header body) staged by the
// wave into LDS with coalesced loads (sha512.h ShaStagedTail); the loop then
// runs whole waves (a lane past the batch end repeats the last item, its
// verdict not stored) because staging needs every lane.
#ifndef OURO_KES_STAGE
#define OURO_KES_STAGE 0
#endif
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_sum6kes_verify(
    size_t n, const uint8_t* __restrict__ vk, const uint32_t* __restrict__ t,
    const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
    const uint32_t* __restrict__ msg_len, const uint8_t* __restrict__ sig,
    uint8_t* __restrict__ verdict, int32_t* scratch, const int32_t* __restrict__ btab) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
#if OURO_KES_STAGE
  __shared__ uint32_t s_stage[kBlock / 64 * kStageWaveDw];
  uint32_t* rows = s_stage + (threadIdx.x >> 6) * kStageWaveDw;
  const size_t lid = threadIdx.x & 63u;
  for (size_t base = tid - lid; base < n; base += nth) {  // wave-uniform
    const size_t i0 = base + lid;
    const size_t i = i0 < n ? i0 : n - 1;
    uint32_t v[8];
    load_words(v, vk + 32 * i, 2);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sig + 448 * i);
    const bool ok = sum6kes_verify_lane(v, t[i], sw, ShaStagedTail{msg + msg_off[i], rows},
                                        msg_len[i], lane, btab);
    if (i0 < n) verdict[i0] = ok ? 1 : 0;
  }
  return;
#endif
  for (size_t i = tid; i < n; i += nth) {
    uint32_t v[8];
    load_words(v, vk + 32 * i, 2);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sig + 448 * i);
    const bool ok = sum6kes_verify_lane(v, t[i], sw, ShaGlobalTail{msg + msg_off[i]}, msg_len[i], lane, btab);
    verdict[i] = ok ? 1 : 0;
  }
}

// The six cores from one run-time-dispatched copy of the dispatch (1, the
// default since round 3) or six inlined calls (0): the same time (r01h 73.76
// vs 73.62 ms; r03e 70.92 vs 70.90 ms) with the kernel's VGPR spills
// 107 -> 48 and its scratch 3,904 -> 3,760 B/lane.
#ifndef OURO_HDR_LOOP
#define OURO_HDR_LOOP 1
#endif
// The finish (inversion, encodings, hashes) out of line with its own
// register allocation (1, the default since round 3): kernel VGPR spills
// 48 -> 9, scratch 3,760 -> 3,152 B/lane, time 69.57 -> 69.43 ms
// (profiles/r03/ab_finish_prefetch.json).
#ifndef OURO_HDR_FINISH_NI
#define OURO_HDR_FINISH_NI 1
#endif
#if OURO_HDR_FINISH_NI
// A/B: the finish (inversion, encodings, hashes) with its own register allocation
__device__ __noinline__ void hdr_finish_item_ni(const ouro_tpraos_batch& b, size_t i,
                                                uint32_t opts, Slot res, Slot tmp,
                                                uint8_t* verdict, uint8_t* beta_eta,
                                                uint8_t* beta_leader) {
  hdr_finish_item(b, i, opts, res, tmp, verdict, beta_eta, beta_leader);
}
#endif

// CLOCK PROBE (a separate diagnostic build, lib/libouro_verify_clock.so,
// -DOURO_CLOCK_STAMPS=1; in the product build no stamp executes): thread 0 of
// each workgroup stamps s_memtime (shader clock) and s_memrealtime (100 MHz)
// at entry and exit of k_tpraos_verify, so bench.py reads the clock the
// header kernel itself ran at (MI355X_MICROARCH.md "DVFS give-back" item 6)
// for roofline.frac_clock.  Every workgroup of the capped grid lives for the
// whole launch.
#ifndef OURO_CLOCK_STAMPS
#define OURO_CLOCK_STAMPS 0
#endif
[[maybe_unused]] constexpr int kClockSlots = 8192;
#if OURO_CLOCK_STAMPS
__device__ unsigned long long g_clock_stamps[kClockSlots][4];
#endif

// ---- one OCERT verification per distinct certificate (OURO_OCERT_SHARE) -----
// An operational certificate is issued once per KES key rotation, so the
// headers of a batch carry a handful of distinct ones per pool, and Ed25519
// verification is a pure function of (key, message, signature).  The verdicts
// are kept from launch to launch in the stream's certificate directory
// (key_cache.h, OURO_KEY_CACHE; the passes are listed at k_kc_begin).  Per
// call:
//   k_ocert_find    header i -> rep[i]: itself, with ocert_ok[i] copied from
//                   the directory, when its 144 key bytes (tpraos.h
//                   ocert_key_*) are found there; otherwise the first header
//                   of the batch seen with the same bytes, those
//                   representatives listed in uniq[0 .. fresh);
//   k_ocert_unique_wide / k_ocert_unique   ocert_ok[uniq[k]] = the check, one
//                   wave (small counts) or one lane per NEW certificate;
//   k_ocert_insert  the new certificates and their verdicts into the directory;
//   k_tpraos_verify takes ocert_ok[rep[i]] as header i's OCERT flag and runs
//                   the other five cores.
// The counts stay on the device (no synchronisation, capturable): every
// kernel reads them and picks its form.  Above kOcertShareMax(n) distinct
// certificates there is too little to share: the unique kernels return at
// once and the header kernel runs the OCERT core inline as without sharing,
// so a batch of distinct certificates costs the group pass and no more.  The
// threshold is a judgement, not a measurement: at count = n - n/8 the unique
// pass does 7/8 of the inline work in a kernel of its own, and the 1/8 saved
// is about what the extra launch and the flag loads cost; the all-distinct
// A/B only bounds it from above.  OURO_OCERT_BYPASS=0 builds
// the A/B form that always shares.
#ifndef OURO_OCERT_BYPASS
#define OURO_OCERT_BYPASS 1
#endif
__host__ __device__ constexpr size_t kOcertShareMax(size_t n) {
  return OURO_OCERT_BYPASS ? n - n / 8 : n;
}
// probes before a header gives up and represents itself (an adversarial batch
// degrades to the unshared cost, never to a wrong verdict or an unbounded loop)
constexpr int kOcertProbeCap = 64;

// ---- the key directories' passes (key_cache.h, OURO_KEY_CACHE) ---------------
// A pool's VRF key lasts for the life of the pool and its certificate for
// months, so what a launch works out per distinct key is kept in the stream's
// workspace and found again by the next launch on that stream.  Each of the
// two instances (certificates, VRF keys) runs, stream-ordered:
//   k_kc_begin     the next generation, the call's counts cleared; the per-call
//                  grouping table cleared only if the call before left
//                  entries in it (a warm step has none);
//   k_*_find       the lookup, read-only on the directory, and the per-call
//                  grouping of its misses (find_pass);
//   k_kc_decide    the batch's distinct count = found + new, the sharing
//                  decision from it as before, and whether the new keys fit;
//   k_kc_reset     (they do not fit) empties the directory; for the VRF keys
//                  k_vrfkey_find then runs again over the whole batch and
//                  k_kc_decide once more;
//   k_*_insert     one lane per new key: a slot, the key bytes, a cell;
//   the build kernels over the new keys' list only.
// The passes that have nothing to do return at once: their grids are sized on
// the host, the counts stay on the device.  No lane waits for another lane's
// write in any of them: probe, compare-and-swap, store.
__global__ void __launch_bounds__(kBlock) k_kc_begin(uint32_t* hdr, uint4* table, size_t quads,
                                                     uint32_t empty) {
  // (the flag is written by k_kc_decide only)
  const bool dirty = hdr[kKcDirty] != 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) kc_begin(hdr, empty != 0u);
  if (!dirty) return;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += nth)
    table[q] = make_uint4(0u, 0u, 0u, 0u);
}
__global__ void k_kc_decide(uint32_t* hdr, uint32_t share_max, uint32_t slots, uint32_t readd,
                            uint32_t after_reset) {
  if (blockIdx.x == 0 && threadIdx.x == 0)
    kc_decide(hdr, share_max, slots, readd != 0u, after_reset != 0u);
}
// table / quads: the per-call grouping table, cleared too when the grouping
// runs again (regroup)
__global__ void __launch_bounds__(kBlock) k_kc_reset(KcDir d, uint4* table, size_t quads,
                                                     uint32_t regroup) {
  // (k_kc_decide's flag; kc_reset_counts leaves it alone)
  if (!d.hdr[kKcReset]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) kc_reset_counts(d.hdr, regroup != 0u);
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint4* cells = reinterpret_cast<uint4*>(d.cells);
  for (size_t q = tid; q < ((size_t)d.mask + 1) / 4; q += nth) cells[q] = make_uint4(0u, 0u, 0u, 0u);
  if (regroup)
    for (size_t q = tid; q < quads; q += nth) table[q] = make_uint4(0u, 0u, 0u, 0u);
}

// Header i against the directory, then (a miss) against the batch's own
// headers.  table: cap_mask + 1 entries, all zero when the pass starts
// (0 = empty, else header index + 1).  Only the CAS's return value is used,
// never a plain load of the table; the keys compared were written before the
// launch, and the directory is only read here, so no fence is needed.
// hash_mask: all ones (the test build's OURO_TEST_OCERT_HASH_BITS narrows it
// to exercise probe chains and the cap).  idx / ok (either may be null): a
// found key's slot and its directory byte for header i.  retry: the pass
// after k_kc_reset, which returns at once unless the directory was emptied;
// nothing can be found then, so every header is grouped.
template <class Key>
__device__ __forceinline__ void find_pass(const ouro_tpraos_batch& b, const KcDir& d,
                                          uint32_t* table, uint32_t cap_mask, uint32_t hash_mask,
                                          uint32_t* __restrict__ rep,
                                          uint32_t* __restrict__ uniq,
                                          uint32_t* __restrict__ idx, uint8_t* __restrict__ ok,
                                          bool retry) {
  if (retry && !d.hdr[kKcReset]) return;
  const uint32_t gen = d.hdr[kKcGen];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const uint32_t lid = threadIdx.x & 63u;
  for (size_t base = tid - lid; base < b.n; base += nth) {  // wave-uniform
    const size_t i = base + lid;
    bool is_rep = false, first_hit = false;
    if (i < b.n) {
      uint32_t key[Key::kWords];
      Key::load(key, b, i);
      const uint64_t h = Key::hash(key);
      const int32_t found = retry ? -1 : kc_lookup<Key::kWords>(d, key, h, hash_mask);
      if (found >= 0) {
        rep[i] = (uint32_t)i;
        if (idx) idx[i] = (uint32_t)found;
        if (ok) ok[i] = d.val[found];
        first_hit = kc_stamp(d, (uint32_t)found, gen);
      } else {
        uint32_t slot = kc_start(h, hash_mask, cap_mask);
        uint32_t r = (uint32_t)i;
        is_rep = true;  // also when the probe cap is reached
        for (int probe = 0; probe < kOcertProbeCap; probe++) {
          const uint32_t prev = atomicCAS(&table[slot], 0u, (uint32_t)i + 1u);
          if (prev == 0u) break;
          uint32_t other[Key::kWords];
          Key::load(other, b, prev - 1u);
          if (Key::equal(key, other)) {
            r = prev - 1u;
            is_rep = false;
            break;
          }
          slot = (slot + 1u) & cap_mask;
        }
        rep[i] = r;
      }
    }
    // one add per wave of its representatives' count, one of its first stamps'
    const unsigned long long m = __ballot(is_rep);
    if (m) {
      uint32_t at = 0;
      if (lid == (uint32_t)__ffsll((long long)m) - 1u)
        at = atomicAdd(&d.hdr[kKcFresh], (uint32_t)__popcll(m));
      at = __shfl(at, __ffsll((long long)m) - 1);
      if (is_rep) uniq[at + __popcll(m & ((1ull << lid) - 1ull))] = (uint32_t)i;
    }
    const unsigned long long mh = __ballot(first_hit);
    if (mh && lid == (uint32_t)__ffsll((long long)mh) - 1u)
      atomicAdd(&d.hdr[kKcHit], (uint32_t)__popcll(mh));
  }
}
// (the key loaders: tpraos.h OcertKey, the 144 certificate bytes, and VrfKey,
// the 32 bytes of vrf_vk)
__global__ void __launch_bounds__(kBlock) k_ocert_find(ouro_tpraos_batch b, KcDir d,
                                                       uint32_t* table, uint32_t cap_mask,
                                                       uint32_t hash_mask,
                                                       uint32_t* __restrict__ rep,
                                                       uint32_t* __restrict__ uniq,
                                                       uint8_t* __restrict__ ocert_ok) {
  find_pass<OcertKey>(b, d, table, cap_mask, hash_mask, rep, uniq, nullptr, ocert_ok, false);
}
__global__ void __launch_bounds__(kBlock) k_vrfkey_find(ouro_tpraos_batch b, KcDir d,
                                                        uint32_t* table, uint32_t cap_mask,
                                                        uint32_t hash_mask,
                                                        uint32_t* __restrict__ rep,
                                                        uint32_t* __restrict__ uniq,
                                                        uint32_t* __restrict__ kidx,
                                                        uint32_t retry) {
  find_pass<VrfKey>(b, d, table, cap_mask, hash_mask, rep, uniq, kidx, nullptr, retry != 0u);
}
// The new certificates of uniq[0 .. fresh) and the verdicts the unique pass
// has just written, into the directory.  (A certificate that gets no slot or
// no cell is verified again by the next launch that carries it.)
__global__ void __launch_bounds__(kBlock) k_ocert_insert(ouro_tpraos_batch b, KcDir d,
                                                         uint32_t hash_mask,
                                                         const uint32_t* __restrict__ uniq,
                                                         const uint8_t* __restrict__ ocert_ok) {
  if (!d.hdr[kKcInsert]) return;
  const uint32_t count = d.hdr[kKcWork], gen = d.hdr[kKcGen];
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += nth) {
    const size_t i = uniq[k];
    uint32_t key[OcertKey::kWords];
    OcertKey::load(key, b, i);
    const int32_t slot = kc_insert<OcertKey::kWords>(d, key, OcertKey::hash(key), hash_mask, gen);
    if (slot >= 0) d.val[slot] = ocert_ok[i];
  }
}

// ---- one fixed-base table of -Y per distinct VRF key (OURO_VRFKEY_SHARE) -----
// A pool's VRF key is the same 32 bytes in every header it forges.  A key's
// table is built by the first launch on a stream that carries the key and
// kept in its slot of the stream's key directory (key_cache.h) until the
// directory is emptied: the workspace re-sized, the knobs reloaded, or new
// keys that no longer fit.  Per call, after k_vrfkey_find has found the
// batch's keys (krep[i]; kidx[i] = the slot of a key already there; the new
// ones' representatives in kuniq[0 .. fresh)):
//   k_vrfkey_insert  new key k on one lane: its slot s, kidx[kuniq[k]] = s and
//                  nslot[k] = s, so header i finds its table at kidx[krep[i]];
//   k_vrfkey_base  new key k on one lane: its flag (the checks of vrf_u_core)
//                  and its window base points (verify.h vrfkey_base);
//   k_vrfkey_fill  (new key, window) on one lane: the window's entries;
//   k_tpraos_verify runs both U cores from the tables: additions only.
// The counts stay on the device.  Above kmax distinct keys in THIS batch (too
// few headers per key, or the tables would not fit the budget: vrfkey_ws.h)
// nothing is inserted or built and the header kernel runs the inline U cores,
// a wave-uniform choice like the certificates'.
// (the header kernel takes one pointer to this record in device memory, null
// when sharing is off; k_vrfkey_base writes it from its own arguments, so the
// header kernel holds two registers for it, not twelve)
struct VrfKeyShare {
  const uint32_t* count = nullptr;  // the batch's distinct keys (the directory's kKcTotal)
  const uint32_t* krep = nullptr;
  const uint32_t* kidx = nullptr;
  const uint8_t* kflag = nullptr;
  const int32_t* ktab = nullptr;    // key k at ktab + k * kYKeyWords
  const int32_t* ubtab = nullptr;   // the chain's fixed-base table (verify.h build_ubtab)
  uint32_t kmax = 0;
};
static_assert(sizeof(VrfKeyShare) <= 64, "the record's place in the grouping buffer (vrfkey_ws.h)");
__global__ void __launch_bounds__(64) k_vrfkey_insert(ouro_tpraos_batch b, KcDir d,
                                                      uint32_t hash_mask,
                                                      const uint32_t* __restrict__ uniq,
                                                      uint32_t* __restrict__ kidx,
                                                      uint32_t* __restrict__ nslot) {
  if (!d.hdr[kKcInsert]) return;
  const uint32_t count = d.hdr[kKcWork], gen = d.hdr[kKcGen];
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += nth) {
    const size_t i = uniq[k];
    uint32_t key[VrfKey::kWords];
    VrfKey::load(key, b, i);
    // (k_kc_decide lets this pass run only when every new key gets a slot)
    const int32_t slot = kc_insert<VrfKey::kWords>(d, key, VrfKey::hash(key), hash_mask, gen);
    kidx[i] = nslot[k] = slot >= 0 ? (uint32_t)slot : 0u;
  }
}
// ctr: the new keys' count, or all ones when the launch does not share (the
// directory's kKcWork)
__global__ void __launch_bounds__(64) k_vrfkey_base(ouro_tpraos_batch b,
                                                    const uint32_t* __restrict__ ctr,
                                                    const uint32_t* __restrict__ uniq,
                                                    const uint32_t* __restrict__ nslot,
                                                    uint8_t* __restrict__ kflag, int32_t* kbase,
                                                    uint32_t kmax, VrfKeyShare desc,
                                                    VrfKeyShare* out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = desc;
  const uint32_t count = *ctr;
  if (count > kmax) return;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += nth) {
    const size_t i = uniq[k], s = nslot[k];
    uint32_t p[8];
    ld_words(p, b.vrf_vk + 32 * i, 2);
    kflag[s] = vrfkey_base(p, kbase + s * kYBaseWords) ? 1 : 0;
  }
}
__global__ void __launch_bounds__(64) k_vrfkey_fill(const uint32_t* __restrict__ ctr,
                                                    const uint32_t* __restrict__ nslot,
                                                    const int32_t* __restrict__ kbase,
                                                    int32_t* ktab, uint32_t kmax) {
  const uint32_t count = *ctr;
  if (count > kmax) return;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  // consecutive lanes take one window of consecutive keys, so a wave's lanes
  // all have the same entry count
  const size_t keys64 = ((size_t)count + 63) / 64 * 64;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < keys64 * kYWindows; t += nth) {
    const size_t blk = t / (64 * (size_t)kYWindows), r = t % (64 * (size_t)kYWindows);
    const size_t k = blk * 64 + (r & 63);
    const int j = (int)(r >> 6);
    if (k >= count) continue;
    const size_t s = nslot[k];
    vrfkey_fill(kbase + s * kYBaseWords, ktab + s * kYKeyWords, j);
  }
}

// The lane form of the unique pass (counts above wide_max, up to share_max):
// certificate k of uniq[] on one lane, in the header kernel's scratch slots,
// which are free until the header kernel starts.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_ocert_unique(
    ouro_tpraos_batch b, const uint32_t* __restrict__ ctr, const uint32_t* __restrict__ uniq,
    uint8_t* __restrict__ ocert_ok, int32_t* scratch, const int32_t* __restrict__ btab,
    uint32_t wide_max, uint32_t share_max) {
  const uint32_t count = *ctr;
  if (count <= wide_max || count > share_max) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kSlotWords);
  for (size_t k = tid; k < count; k += nth) {
    const size_t i = uniq[k];
    uint32_t s[16], p[8], hv[8];
    ld_words(s, b.ocert_sigma + 64 * i, 4);
    ld_words(p, b.issuer_vk + 32 * i, 2);
    ld_words(hv, b.hot_vk + 32 * i, 2);
    OcertMsg m;
    ocert_msg(m, hv, b.ocert_counter[i], b.ocert_kes_period[i]);
    ocert_ok[i] = ed25519_verify_lane(s, p, m, 48, lane, btab) ? 1 : 0;
  }
}

// A U core of header i from its key's table, out of line with its own register
// allocation (like the finish): the header kernel's own spills stay where
// they were without it.
__device__ __noinline__ void hdr_u_shared_ni(const ouro_tpraos_batch& b, size_t i, bool leader,
                                             Slot lane, Slot res, const VrfKeyShare* ks) {
  const uint32_t k = ks->kidx[ks->krep[i]];
  hdr_u_shared(b, i, leader, ks->kflag[k] != 0, lane, res, ks->ubtab,
               ks->ktab + (size_t)k * kYKeyWords);
}

// Throughput mode: one lane per header runs every core of tpraos.h, sharing
// the VRF key decode and its table, then the single-inversion finish.
// rep / ocert_ok / ocert_count (all null when sharing is off): the OCERT
// verdicts of the unique pass; with at most kOcertShareMax(n) distinct
// certificates the OCERT core is not run here (a wave-uniform choice).
// ks (null when sharing is off): the per-key VRF tables; with at most
// ks->kmax distinct keys both U cores run from them (hdr_u_shared_ni), and no
// key is decoded or tabulated here.
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_tpraos_verify(ouro_tpraos_batch b,
                                                             uint8_t* __restrict__ verdict,
                                                             uint8_t* __restrict__ beta_eta,
                                                             uint8_t* __restrict__ beta_leader,
                                                             int32_t* scratch,
                                                             const int32_t* __restrict__ btab,
                                                             const uint32_t* __restrict__ rep,
                                                             const uint8_t* __restrict__ ocert_ok,
                                                             const uint32_t* __restrict__ ocert_count,
                                                             uint32_t xopts,
                                                             const VrfKeyShare* ks) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const Slot lane = slot_of(scratch, tid, kHdrLaneWords);
  const Slot res = lane + kLaneWords;
  const uint32_t opts = batch_opts(b) | xopts;  // xopts: kOptEpochs (launch_hdr)
  const bool shared = ocert_count != nullptr && *ocert_count <= kOcertShareMax(b.n);
  const int core0 = shared ? kCoreKes : kCoreOcert;
  // both U cores from the key's table (ks: null when sharing is off)
  const bool kshared = ks != nullptr && *ks->count <= ks->kmax;
#if OURO_CLOCK_STAMPS
  unsigned long long c0 = 0, r0 = 0;
  if (threadIdx.x == 0) {
    r0 = __builtin_amdgcn_s_memrealtime();
    c0 = __builtin_amdgcn_s_memtime();
  }
#endif
  for (size_t i = tid; i < b.n; i += nth) {
    if (shared) stg1(res.word(kResFlags + kCoreOcert), ocert_ok[rep[i]] ? kFlagOk : 0);
#if OURO_HDR_LOOP
    // one copy of the core dispatch, the core chosen at run time
#pragma unroll 1
    for (int c = core0; c <= kCoreVl; c++) {
      if (kshared && (c == kCoreUe || c == kCoreUl)) {
        hdr_u_shared_ni(b, i, c == kCoreUl, lane, res, ks);
        continue;
      }
      hdr_core(b, i, opts, c, lane, res, btab);
    }
#else
    if (!shared) hdr_core(b, i, opts, kCoreOcert, lane, res, btab);
    hdr_core(b, i, opts, kCoreKes, lane, res, btab);
    if (kshared) {
      hdr_u_shared_ni(b, i, false, lane, res, ks);
      hdr_u_shared_ni(b, i, true, lane, res, ks);
    } else {
      hdr_core(b, i, opts, kCoreUe, lane, res, btab);
      hdr_core(b, i, opts, kCoreUl, lane, res, btab);
    }
    hdr_core(b, i, opts, kCoreVe, lane, res, btab);
    hdr_core(b, i, opts, kCoreVl, lane, res, btab);
#endif
#if OURO_HDR_FINISH_NI
    hdr_finish_item_ni(b, i, opts, res, lane, verdict, beta_eta, beta_leader);
#else
    hdr_finish_item(b, i, opts, res, lane, verdict, beta_eta, beta_leader);
#endif
  }
#if OURO_CLOCK_STAMPS
  __syncthreads();  // the whole workgroup's work inside the stamps
  if (threadIdx.x == 0 && blockIdx.x < kClockSlots) {
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    g_clock_stamps[blockIdx.x][0] = c0;
    g_clock_stamps[blockIdx.x][1] = c1;
    g_clock_stamps[blockIdx.x][2] = r0;
    g_clock_stamps[blockIdx.x][3] = r1;
  }
#endif
}

// ---- the split header kernel (OURO_SPLIT, round 4) ---------------------------
// The same cores as k_tpraos_verify in three launches per chunk of headers, so
// the double-scalar multiplications -- ~70 % of a header's time, and code
// whose chains fit in 128 VGPRs -- run at OURO_DSM_WAVES waves per SIMD while
// the decodes, hashes, table builds and the finish keep the 2-wave budget they
// need (3 waves spill there: +2.7 %, profiles/r04b/ab_waves_w2_vs_w3.json):
//   k_hdr_pre   header li of the chunk: every core's kPhasePre into its own
//               task slot (core * chunk + li), flags into the header's record;
//   k_hdr_dsm   task t: dsm_lane with the cfg the pre phase left in the slot
//               (t = core * chunk + li: a wave's 64 tasks are one core of 64
//               consecutive headers, the same grouping the pre phase's
//               wave_max_small saw, so the window count is wave-uniform);
//   k_hdr_post  header li: every core's kPhasePost, then the finish.
#ifndef OURO_DSM_WAVES
#define OURO_DSM_WAVES 4
#endif
#ifndef OURO_PRE_WAVES
#define OURO_PRE_WAVES OURO_WAVES  // the pre / post kernels' own budgets (A/B)
#endif
#ifndef OURO_POST_WAVES
#define OURO_POST_WAVES OURO_WAVES
#endif
constexpr int kHdrResWords = round_slot(kResWords);
__global__ void __launch_bounds__(kBlock, OURO_PRE_WAVES) k_hdr_pre(ouro_tpraos_batch b, size_t base,
                                                               size_t count, size_t chunk,
                                                               int32_t* tasks, int32_t* res_buf,
                                                               const int32_t* __restrict__ btab,
                                                               uint32_t xopts) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const uint32_t opts = batch_opts(b) | xopts;
  for (size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x; li < count; li += nth) {
    const size_t i = base + li;
    const Slot res = slot_of(res_buf, li, kHdrResWords);
    const Slot ukey = slot_of(tasks, (size_t)kCoreUe * chunk + li, kSlotWords);
#pragma unroll 1
    for (int c = kCoreOcert; c <= kCoreVl; c++)
      hdr_core(b, i, opts, c, slot_of(tasks, (size_t)c * chunk + li, kSlotWords), res, btab, true,
               false, false, kPhasePre, ukey);
  }
}
__global__ void __launch_bounds__(kBlock, OURO_DSM_WAVES) k_hdr_dsm(size_t count, size_t chunk,
                                                                   int ncores, int32_t* tasks,
                                                                   const int32_t* __restrict__ btab) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const size_t ntasks = (size_t)ncores * chunk;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < ntasks; t += nth) {
    if (t % chunk >= count) continue;  // the last chunk's unused headers
    const Slot s = slot_of(tasks, t, kSlotWords);
    dsm_lane_dsm_launch(s, btab, (uint32_t)ldg1(s.word(kSlotCfg)));
  }
}
__global__ void __launch_bounds__(kBlock, OURO_POST_WAVES) k_hdr_post(ouro_tpraos_batch b, size_t base,
                                                                size_t count, size_t chunk,
                                                                int32_t* tasks, int32_t* res_buf,
                                                                uint8_t* __restrict__ verdict,
                                                                uint8_t* __restrict__ beta_eta,
                                                                uint8_t* __restrict__ beta_leader,
                                                                uint32_t xopts) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  const uint32_t opts = batch_opts(b) | xopts;
  for (size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x; li < count; li += nth) {
    const size_t i = base + li;
    const Slot res = slot_of(res_buf, li, kHdrResWords);
#pragma unroll 1
    for (int c = kCoreOcert; c <= kCoreVl; c++)
      hdr_core(b, i, opts, c, slot_of(tasks, (size_t)c * chunk + li, kSlotWords), res, nullptr,
               true, false, false, kPhasePost);
    // the finish's 8 x 12 scratch words: the header's (spent) OCERT task slot
#if OURO_HDR_FINISH_NI
    hdr_finish_item_ni(b, i, opts, res, slot_of(tasks, li, kSlotWords), verdict, beta_eta,
                       beta_leader);
#else
    hdr_finish_item(b, i, opts, res, slot_of(tasks, li, kSlotWords), verdict, beta_eta,
                    beta_leader);
#endif
  }
}

// The standalone Ed25519 / Sum6KES kernels split the same way (one task per
// item; the checks before the dsm in the slot's spare word kSlotCfg + 1).
constexpr int kSlotPreOk = kSlotCfg + 1;
__global__ void __launch_bounds__(kBlock, OURO_PRE_WAVES) k_ed25519_pre(
    size_t base, size_t count, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
    const uint32_t* __restrict__ msg_len, int32_t* tasks, const int32_t* __restrict__ btab,
    uint32_t byron) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x; li < count; li += nth) {
    const size_t i = base + li;
    const Slot s = slot_of(tasks, li, kSlotWords);
    uint32_t sg[16], p[8];
    load_words(sg, sig + 64 * i, 4);
    load_words(p, pk + 32 * i, 2);
    const bool ok = ed25519_verify_lane(sg, p, ShaGlobalTail{msg + msg_off[i]}, msg_len[i], s, btab,
                                        byron != 0, false, kPhasePre);
    stg1(s.word(kSlotPreOk), ok ? 1 : 0);
  }
}
__global__ void __launch_bounds__(kBlock, OURO_PRE_WAVES) k_sum6kes_pre(
    size_t base, size_t count, const uint8_t* __restrict__ vk, const uint32_t* __restrict__ t,
    const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
    const uint32_t* __restrict__ msg_len, const uint8_t* __restrict__ sig, int32_t* tasks,
    const int32_t* __restrict__ btab) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x; li < count; li += nth) {
    const size_t i = base + li;
    const Slot s = slot_of(tasks, li, kSlotWords);
    uint32_t v[8];
    load_words(v, vk + 32 * i, 2);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(sig + 448 * i);
    const bool ok = sum6kes_verify_lane(v, t[i], sw, ShaGlobalTail{msg + msg_off[i]}, msg_len[i], s,
                                        btab, false, kPhasePre);
    stg1(s.word(kSlotPreOk), ok ? 1 : 0);
  }
}
// verdict = the pre checks and [the dsm's result] == O
__global__ void __launch_bounds__(kBlock) k_ed_post(size_t base, size_t count, int32_t* tasks,
                                                    uint8_t* __restrict__ verdict) {
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t li = (size_t)blockIdx.x * blockDim.x + threadIdx.x; li < count; li += nth) {
    const Slot s = slot_of(tasks, li, kSlotWords);
    verdict[base + li] = (ldg1(s.word(kSlotPreOk)) && dsm_result_is_identity(s)) ? 1 : 0;
  }
}

// Latency mode (k_tpraos_cores, k_tpraos_finish): kernels_lat.hip, its own
// translation unit built with the row-order field products (lane quads issue
// one product per lane, whose dependent column-scan chains would stall: A/B
// p50 0.5875 -> 0.5712 ms, profiles/r02d/ablat_rows_scan.json).
__global__ void k_tpraos_cores(ouro_tpraos_batch b, const uint32_t* __restrict__ d_n,
                               int32_t* res_buf, int32_t* scratch,
                               const int32_t* __restrict__ btab, int mode, int wide_waves,
                               uint8_t* __restrict__ verdict, uint8_t* __restrict__ beta_eta,
                               uint8_t* __restrict__ beta_leader, uint32_t* win_ctr,
                               uint32_t* done);
__global__ void k_ed25519_wide(size_t n, const uint8_t* __restrict__ pk,
                               const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
                               const uint64_t* __restrict__ msg_off,
                               const uint32_t* __restrict__ msg_len, uint8_t* __restrict__ verdict,
                               const int32_t* __restrict__ btab, uint32_t byron);
__global__ void k_vrf03_wide(size_t n, const uint8_t* __restrict__ pk,
                             const uint8_t* __restrict__ proof, const uint8_t* __restrict__ alpha,
                             const uint64_t* __restrict__ alpha_off,
                             const uint32_t* __restrict__ alpha_len, uint8_t* __restrict__ beta,
                             uint8_t* __restrict__ verdict, const int32_t* __restrict__ btab,
                             uint32_t flags);
__global__ void k_tpraos_finish(ouro_tpraos_batch b, const uint32_t* __restrict__ d_n,
                                int32_t* res_buf, uint8_t* __restrict__ verdict,
                                uint8_t* __restrict__ beta_eta, uint8_t* __restrict__ beta_leader,
                                int32_t* scratch, int quad);
// the wave form of the OCERT unique pass (counts up to wide_max)
__global__ void k_ocert_unique_wide(ouro_tpraos_batch b, const uint32_t* __restrict__ ctr,
                                    const uint32_t* __restrict__ uniq,
                                    uint8_t* __restrict__ ocert_ok,
                                    const int32_t* __restrict__ btab, uint32_t wide_max,
                                    uint32_t share_max);

// Raw wire headers -> the SoA on the device, one lane
// per header: the host slicer's parse (cbor.h, pinned to header.py by
// tests/test_pack.py), spans checked against raw_bytes here (status
// OURO_PACK_ESPAN) since a device call cannot return OURO_EINVAL per header.
__global__ void __launch_bounds__(kBlock) k_tpraos_pack(const uint8_t* __restrict__ raw,
                                                        size_t raw_bytes,
                                                        const uint64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ len, size_t n,
                                                        uint64_t spkp, cbor::Out o,
                                                        uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = off[i];
    const uint32_t l0 = len[i];
    uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                     ? (uint8_t)OURO_PACK_ESPAN
                     : cbor::pack_one(raw, o0, l0, spkp, o, i);
    if (st != OURO_PACK_OK) cbor::zero_row(o, i);
    status[i] = st;
  }
}

// The Byron slicer (cbor_byron.h byron_pack_one, the host slicer's parse) on
// the device, one lane per header, over a chunk staged densely by raw_stage:
// header i's bytes at off[i] = the lengths' prefix sum, so its message slot
// (len + kByronMsgExtra bytes, ouro_byron_pack_cbor's layout) starts at
// off[i] + kByronMsgExtra * i.  A rejected row is zeroed (msg_len 0).
__global__ void __launch_bounds__(kBlock) k_byron_pack(const uint8_t* __restrict__ raw,
                                                       size_t raw_bytes,
                                                       const uint64_t* __restrict__ off,
                                                       const uint32_t* __restrict__ len, size_t n,
                                                       int64_t magic, cbor::ByronOut o,
                                                       uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = off[i];
    const uint32_t l0 = len[i];
    o.msg_off[i] = o0 + cbor::kByronMsgExtra * i;
    uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                     ? (uint8_t)OURO_PACK_ESPAN
                     : cbor::byron_pack_one(raw, o0, l0, magic, o, i);
    if (st != OURO_PACK_OK) cbor::byron_zero_row(o, i);
    status[i] = st;
  }
}

// ---- whole-block storage integrity (cbor_block.h) ----
// The block slicer on the device, one lane per block: the TPraos header rows
// of item 0 (the KES kernel's inputs), the claimed bodyHash and the spans of
// items 1..3.  A rejected block's rows are zeroed (its three spans are then
// empty: the hash kernel reads nothing for them).
__global__ void __launch_bounds__(kBlock) k_block_pack(const uint8_t* __restrict__ raw,
                                                       size_t raw_bytes,
                                                       const uint64_t* __restrict__ off,
                                                       const uint32_t* __restrict__ len, size_t n,
                                                       uint64_t spkp, cbor::Out o, cbor::BlockOut bo,
                                                       uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = off[i];
    const uint32_t l0 = len[i];
    uint8_t st = (o0 > raw_bytes || raw_bytes - o0 < l0)
                     ? (uint8_t)OURO_PACK_ESPAN
                     : cbor::block_one(raw, o0, l0, spkp, o, bo, i);
    if (st != OURO_PACK_OK) cbor::block_zero_row(o, bo, i);
    status[i] = st;
  }
}

// The length class of a message: the bit length of its compression count
// (1 for up to 128 bytes, the empty message included; at most 26).
__device__ __forceinline__ uint32_t b2b_class(uint32_t len) {
  const uint32_t nc = len ? (len >> 7) + ((len & 127u) ? 1u : 0u) : 1u;
  return 32u - (uint32_t)__clz((int)nc);
}
// the sort's 64 counters cleared on the stream (a kernel, not a memset: no
// host-side wait on a stream that other chunks' work shares the device with)
__global__ void k_b2b_clear(uint32_t* cnt) {
  if (blockIdx.x == 0 && threadIdx.x < 64) cnt[threadIdx.x] = 0;
}
// The counting sort of the work items by length class, so that the 64 lanes
// of a wave hash spans of similar length (a wave runs as long as its longest
// lane): counts per class (cnt[0..31], cleared by k_b2b_clear), ...
__global__ void __launch_bounds__(kBlock) k_b2b_count(size_t m, const uint32_t* __restrict__ len,
                                                      uint32_t* cnt) {
  __shared__ uint32_t s_cnt[32];
  if (threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < m; i += nth) atomicAdd(&s_cnt[b2b_class(len[i])], 1u);
  __syncthreads();
  if (threadIdx.x < 32 && s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
}
// ... each class's first position, the longest class first (start[c] =
// cnt[32 + c]; one thread: 32 counters), ...
__global__ void k_b2b_starts(uint32_t* cnt) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t at = 0;
  for (int c = 31; c >= 0; c--) {
    cnt[32 + c] = at;
    at += cnt[c];
  }
}
// ... and the permutation: lane j of the hash kernel takes item perm[j].  A
// workgroup ranks its 256 items per class in LDS and reserves each class's
// range with ONE global atomic, so a batch of one class does not serialise
// on a single counter, and neighbouring items stay neighbours inside a class
// (the three segments of a block are adjacent in memory).
__global__ void __launch_bounds__(kBlock) k_b2b_scatter(size_t m, const uint32_t* __restrict__ len,
                                                        uint32_t* cnt, uint32_t* __restrict__ perm) {
  __shared__ uint32_t s_cnt[32], s_base[32];
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  // (whole workgroups: every thread reaches the barriers)
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < m; base += nth) {
    const size_t i = base + threadIdx.x;
    if (threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c = 0, rank = 0;
    if (i < m) {
      c = b2b_class(len[i]);
      rank = atomicAdd(&s_cnt[c], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 32 && s_cnt[threadIdx.x])
      s_base[threadIdx.x] = atomicAdd(&cnt[32 + threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (i < m) {
      const size_t pos = (size_t)s_base[c] + rank;
      if (pos < m) perm[pos] = (uint32_t)i;  // (pos < m always: the counts sum to m)
    }
    __syncthreads();
  }
}

// Workgroups of one wave: in sorted order the long messages fill the first
// waves, and single-wave workgroups spread those over the CUs instead of
// packing four of them onto one.
constexpr int kB2bBlock = 64;
// out[i] = Blake2b-256(msg[off[i] .. off[i] + len[i])), one lane per message
// (blake2b_stream.h), item perm[j] on lane j (perm null: item j).  msg must
// be 4-byte aligned: the lane reads the aligned dwords its span touches.  A
// span outside msg_bytes is not read; its digest is zero.
__global__ void __launch_bounds__(kB2bBlock) k_blake2b256(size_t m, const uint8_t* __restrict__ msg,
                                                       size_t msg_bytes,
                                                       const uint64_t* __restrict__ off,
                                                       const uint32_t* __restrict__ len,
                                                       const uint32_t* __restrict__ perm,
                                                       uint8_t* __restrict__ out) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t j = tid; j < m; j += nth) {
    const size_t i = perm ? (size_t)perm[j] : j;
    if (i >= m) continue;
    const uint64_t o0 = off[i];
    const uint32_t l0 = len[i];
    uint32_t d[8];
    if (o0 > msg_bytes || msg_bytes - o0 < l0) {
#pragma unroll
      for (int k = 0; k < 8; k++) d[k] = 0;
    } else {
      blake2b256_stream(d, msg + o0, l0);
    }
    stg4(out + 32 * i, make_int4((int)d[0], (int)d[1], (int)d[2], (int)d[3]));
    stg4(out + 32 * i + 16, make_int4((int)d[4], (int)d[5], (int)d[6], (int)d[7]));
  }
}

// ---- the header envelope (envelope.h; include/ouro_verify.h
// ouro_chain_envelope_cbor) ----
// The envelope slicer, one lane per header in the caller's order: the
// header's era (cbor.h era_class), then that era's slicer WITHOUT its rows
// (pack_one<false> / byron_pack_one<false>: the same acceptance, so status[i]
// is what the crypto entries report) filling record i -- fields, previous
// hash and the span the header hash covers.  A header that is rejected, or
// whose envelope fields have another shape, keeps a zero record.
__global__ void __launch_bounds__(kBlock) k_envelope_slice(const uint8_t* __restrict__ raw,
                                                           size_t raw_bytes,
                                                           const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ len,
                                                           size_t n, uint64_t epoch_slots,
                                                           env::Rec* __restrict__ rec,
                                                           uint8_t* __restrict__ status) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const uint64_t o0 = off[i];
    const uint32_t l0 = len[i];
    env::Rec* r = rec + i;
    env::rec_clear(r);
    uint8_t st;
    if (o0 > raw_bytes || raw_bytes - o0 < l0) {
      st = (uint8_t)OURO_PACK_ESPAN;
    } else if (cbor::era_class(raw + o0, l0) == OURO_PROTO_PBFT) {
      st = cbor::byron_pack_one<false>(raw, o0, l0, -1, cbor::ByronOut{}, i, r, epoch_slots);
      if (epoch_slots == 0) env::rec_clear(r);  // no Byron slot without the epoch's length
    } else {
      st = cbor::pack_one<false>(raw, o0, l0, 1, cbor::Out{}, i, r);
    }
    status[i] = st;
  }
}

// Record i's header hash, one lane per header (workgroups of one wave, as
// k_blake2b256): Blake2b-256 of the sliced span behind the era's prefix
// (blake2b_stream.h blake2b256_stream_prefixed).  raw must be 4-byte aligned.
// No length-class sort: the headers of one era are within a compression or
// two of each other.  An unusable record keeps its zero hash.
__global__ void __launch_bounds__(kB2bBlock) k_header_hash(size_t n,
                                                           const uint8_t* __restrict__ raw,
                                                           size_t raw_bytes, env::Rec* rec) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    env::Rec* r = rec + i;
    if (!r->sliced) continue;
    const uint64_t o0 = r->hdr_off;
    const uint32_t l0 = r->hdr_len;
    if (o0 > raw_bytes || raw_bytes - o0 < l0) continue;  // (cannot happen: the slicer's span)
    uint32_t npre;
    const uint32_t pre = env::hash_prefix(*r, &npre);
    uint32_t d[8];
    blake2b256_stream_prefixed(d, pre, npre, raw + o0, l0);
    stg4(r->hash, make_int4((int)d[0], (int)d[1], (int)d[2], (int)d[3]));
    stg4(r->hash + 16, make_int4((int)d[4], (int)d[5], (int)d[6], (int)d[7]));
  }
}

// envelope[i] = envelope_link(record i - 1, record i) in the caller's order
// (header 0 on top of `tip`), the hash out of the record, and the last
// header as the next call's tip.  header_hash: 16-byte aligned.  ends
// (optional): the first and the last record, for the raw pipeline's host to
// link a chunk to the one before it (raw_pipe.cpp raw_drain).
__global__ void __launch_bounds__(kBlock) k_envelope_link(size_t n, const env::Rec* __restrict__ rec,
                                                          env::Rec tip, ouro_envelope_cfg cfg,
                                                          uint8_t* __restrict__ envelope,
                                                          uint8_t* __restrict__ header_hash,
                                                          ouro_chain_tip* tip_out,
                                                          env::Rec* __restrict__ ends) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const env::Rec cur = rec[i];
    const env::Rec prev = i ? rec[i - 1] : tip;
    envelope[i] = env::envelope_link(prev, cur, cfg);
    stg4(header_hash + 32 * i, ldg4(rec[i].hash));
    stg4(header_hash + 32 * i + 16, ldg4(rec[i].hash + 16));
    if (i == n - 1 && tip_out) env::tip_of_rec(tip_out, cur);
    if (ends && i == 0) ends[0] = cur;
    if (ends && i == n - 1) ends[1] = cur;
  }
}

// bbHash = Blake2b-256 of the block's three segment digests (96 bytes: one
// final compression with t = 96), compared with the claimed bodyHash and
// merged with the KES verdict: verdict[i] = OURO_BLK_* bits, 0 (and a zero
// body_hash) for a block that did not slice.  body_hash may be null.
__global__ void __launch_bounds__(kBlock) k_block_finish(size_t n, const uint8_t* __restrict__ status,
                                                         const uint8_t* __restrict__ digest,
                                                         const uint8_t* __restrict__ claimed,
                                                         const uint8_t* __restrict__ kes,
                                                         uint8_t* __restrict__ verdict,
                                                         uint8_t* __restrict__ body_hash) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t h[8];
    uint8_t v = 0;
    if (status[i] == OURO_PACK_OK) {
      uint32_t in[24], c[8];
      load_words(in, digest + 96 * i, 6);
      load_words(c, claimed + 32 * i, 2);
      blake2b256_96(h, in);
      uint32_t diff = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) diff |= h[k] ^ c[k];
      v = (uint8_t)((kes[i] ? OURO_BLK_KES_OK : 0u) | (diff == 0 ? OURO_BLK_BODY_OK : 0u));
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) h[k] = 0;
    }
    verdict[i] = v;
    if (body_hash) {
      // (the caller's buffer: n x 32 at any alignment)
      for (int k = 0; k < 32; k++) body_hash[32 * i + k] = (uint8_t)(h[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// leader threshold (leader.h), one item per lane; verdict 1 / 0 / 0xff
__global__ void __launch_bounds__(kBlock) k_leader_check(size_t n, const uint8_t* __restrict__ beta,
                                                         const uint64_t* __restrict__ num,
                                                         const uint64_t* __restrict__ den,
                                                         uint64_t act_log_lo, int64_t act_log_hi,
                                                         uint32_t f_is_one,
                                                         uint8_t* __restrict__ verdict) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    const int32_t r = f_is_one ? kLeaderYes
                               : leader_check_lane(beta + 64 * i, num[i], den[i], act_log_lo,
                                                   act_log_hi);
    verdict[i] = r < 0 ? (uint8_t)0xff : (uint8_t)r;
  }
}

// proof_to_hash only (no verification): beta = H(0x04 || 0x03 || [8]Gamma)
__global__ void __launch_bounds__(kBlock, OURO_WAVES) k_vrf03_proof_to_hash(size_t n,
                                                                const uint8_t* __restrict__ proof,
                                                                uint8_t* __restrict__ beta,
                                                                uint8_t* __restrict__ verdict) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nth = (size_t)gridDim.x * blockDim.x;
  for (size_t i = tid; i < n; i += nth) {
    uint32_t G[8];
    load_words(G, proof + 80 * i, 2);
    ge_p3 Gamma;
    bool ok = ge_is_canonical(G);
    ok = ge_decode(&Gamma, G, false) && ok;
    ge_p3 G8 = ge_mul8(Gamma);
    uint32_t enc[8];
    ge_encode_with_inv(enc, G8.X, G8.Y, fe_invert(G8.Z));
    uint32_t bp[9];
    bp[0] = 0x04u | (0x03u << 8) | (enc[0] << 16);
#pragma unroll
    for (int k = 1; k < 8; k++) bp[k] = (enc[k - 1] >> 16) | (enc[k] << 16);
    bp[8] = enc[7] >> 16;
    uint64_t H[8];
    sha512_prefixed<34>(H, bp, ShaNoTail{}, 0);
    uint32_t w[16];
    sha512_digest_words(w, H);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = ok ? w[k] : 0u;
    store_words(beta + 64 * i, w, 4);
    verdict[i] = ok ? 1 : 0;
  }
}


// A plan's window read straight from its pinned input block by a copy kernel
// (OURO_PLAN_STAGE >= 1; A/B against the DMA copy node): one 16-B load per
// thread, every load of the window in flight at once.
// stamp (a plan's timing probe, OURO_PLAN_TIMING; else null): the copy's start
// in s_memrealtime ticks (100 MHz), written to the plan's pinned done block.
__device__ __forceinline__ void plan_stamp(uint64_t* stamp) {
  if (stamp && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(stamp, (uint64_t)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(256) k_plan_stage(const uint4* __restrict__ src,
                                                    uint4* __restrict__ dst, size_t n16,
                                                    uint64_t* stamp) {
  plan_stamp(stamp);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) dst[i] = src[i];
}
// The same over the byte ranges a window actually uses (the block header, and
// per member given its n rows or the body span -- not the capacity), in 16-B
// units: thread t copies unit t of the concatenated ranges (round 5: the
// copy reads pinned memory over PCIe, so its bytes are its time).
// (kPlanMaxRanges, PlanRanges: launches.h -- the plan fills them)
__global__ void __launch_bounds__(256) k_plan_stage_ranges(const uint4* __restrict__ src,
                                                           uint4* __restrict__ dst,
                                                           PlanRanges r, uint64_t* stamp) {
  plan_stamp(stamp);
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t k = 0; k < r.count; k++) {
    if (t < r.len16[k]) {
      const uint32_t i = r.start16[k] + t;
      dst[i] = src[i];
      return;
    }
    t -= r.len16[k];
  }
}

// --------------------------------------------------------------- launches ----
// (launches.h: all the host units see of this file)
namespace ouro_rt {

const void* kernel_ptr(int id) {
  switch (id) {
    case kEd: return reinterpret_cast<const void*>(&k_ed25519_verify);
    case kVrf: return reinterpret_cast<const void*>(&k_vrf03_verify);
    case kKes: return reinterpret_cast<const void*>(&k_sum6kes_verify);
    case kHdr: return reinterpret_cast<const void*>(&k_tpraos_verify);
    case kCores: return reinterpret_cast<const void*>(&k_tpraos_cores);
    case kFinish: return reinterpret_cast<const void*>(&k_tpraos_finish);
    case kLeader: return reinterpret_cast<const void*>(&k_leader_check);
    case kHdrPre: return reinterpret_cast<const void*>(&k_hdr_pre);
    case kHdrDsm: return reinterpret_cast<const void*>(&k_hdr_dsm);
    case kHdrPost: return reinterpret_cast<const void*>(&k_hdr_post);
    case kEdPre: return reinterpret_cast<const void*>(&k_ed25519_pre);
    case kKesPre: return reinterpret_cast<const void*>(&k_sum6kes_pre);
    case kOcertUnique: return reinterpret_cast<const void*>(&k_ocert_unique);
    default: return reinterpret_cast<const void*>(&k_vrf03_proof_to_hash);
  }
}

// ---- device-pointer launches (shared by the host-buffer and device APIs) ----
namespace {
int wide_grid(size_t n) { return (int)std::min<size_t>(n, 8192); }
// One Ed25519-shaped item per task: chunks of 4 resident grids of the pre
// kernel, so the 4-wave dsm launch has 2 grids of tasks to spread.
template <class LaunchPre>
int launch_split_items(DeviceState* ds, hipStream_t st, size_t n, int pre_id, uint8_t* verdict,
                       LaunchPre&& launch_pre) {
  const size_t cap = (size_t)ds->max_blocks[pre_id] * kBlock;
  const size_t chunk = std::min<size_t>((n + kBlock - 1) / kBlock * kBlock, 4 * cap);
  Buf& sb = ctx().scratch[st];
  int rc = ensure(sb, slot_region_words(chunk, kSlotWords) * sizeof(int32_t));
  if (rc) return rc;
  int32_t* tasks = static_cast<int32_t*>(sb.p);
  const int gp = (int)std::min<size_t>(chunk / kBlock, (size_t)ds->max_blocks[pre_id]);
  const int gd = (int)std::min<size_t>(chunk / kBlock, (size_t)ds->max_blocks[kHdrDsm]);
  for (size_t base = 0; base < n; base += chunk) {
    const size_t count = std::min(chunk, n - base);
    launch_pre(gp, base, count, tasks);
    hipLaunchKernelGGL(k_hdr_dsm, dim3(gd), dim3(kBlock), 0, st, count, chunk, 1, tasks, ds->btab);
    hipLaunchKernelGGL(k_ed_post, dim3(gp), dim3(kBlock), 0, st, base, count, tasks, verdict);
    if ((rc = launch_check())) return rc;
  }
  return OURO_OK;
}
}  // namespace
// byron = 1: ByronDSIGN acceptance (cardano-crypto)
int launch_ed(hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
              const uint64_t* off, const uint32_t* len, uint8_t* verdict, uint32_t byron) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  if (n <= wide_small_max()) {
    hipLaunchKernelGGL(k_ed25519_wide, dim3(wide_grid(n)), dim3(64), 0, st, n, pk, sig, msg, off,
                       len, verdict, ds->btab, byron);
    return launch_check();
  }
  if (split_launch())
    return launch_split_items(ds, st, n, kEdPre, verdict, [&](int g, size_t base, size_t count,
                                                               int32_t* tasks) {
      hipLaunchKernelGGL(k_ed25519_pre, dim3(g), dim3(kBlock), 0, st, base, count, pk, sig, msg,
                         off, len, tasks, ds->btab, byron);
    });
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kEd, n, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_ed25519_verify, dim3(grid), dim3(kBlock), 0, st, n, pk, sig, msg, off, len,
                     verdict, scr, ds->btab, byron);
  return launch_check();
}

int launch_vrf(hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* proof,
               const uint8_t* alpha, const uint64_t* off, const uint32_t* len, uint8_t* beta,
               uint8_t* verdict, uint32_t flags) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  if (n <= wide_small_max()) {
    hipLaunchKernelGGL(k_vrf03_wide, dim3(wide_grid(n)), dim3(64), 0, st, n, pk, proof, alpha,
                       off, len, beta, verdict, ds->btab, flags);
    return launch_check();
  }
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kVrf, n, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_vrf03_verify, dim3(grid), dim3(kBlock), 0, st, n, pk, proof, alpha, off,
                     len, beta, verdict, scr, ds->btab, flags);
  return launch_check();
}

int launch_kes(hipStream_t st, size_t n, const uint8_t* vk, const uint32_t* t, const uint8_t* msg,
               const uint64_t* off, const uint32_t* len, const uint8_t* sig, uint8_t* verdict) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  if (split_launch())
    return launch_split_items(ds, st, n, kKesPre, verdict, [&](int g, size_t base, size_t count,
                                                                int32_t* tasks) {
      hipLaunchKernelGGL(k_sum6kes_pre, dim3(g), dim3(kBlock), 0, st, base, count, vk, t, msg, off,
                         len, sig, tasks, ds->btab);
    });
  int grid;
  int32_t* scr;
  if ((rc = plan(ds, kKes, n, st, &grid, &scr))) return rc;
  hipLaunchKernelGGL(k_sum6kes_verify, dim3(grid), dim3(kBlock), 0, st, n, vk, t, msg, off, len,
                     sig, verdict, scr, ds->btab);
  return launch_check();
}


// ---- a key directory's host side (key_cache.h, runtime.h KeyDirWs) ----
// certificates a stream's directory holds at the most (157 B each)
constexpr size_t kOcertDirSlots = 65536;
struct KeyDir {
  KcDir d;
  uint32_t* extra = nullptr;  // a word per slot of the caller's (KcLayout off_extra)
  bool empty = false;         // the host empties it for this launch: the cells ...
  bool restart = false;       // ... and the counters too (generation, times emptied)
  bool clear_tab = false;     // the host clears the per-call grouping table
  // what the workspace records once the launch is enqueued whole (keydir_commit)
  unsigned long long epoch = 0, tab_gen = 0, aux_gen = 0;
  size_t tab_off = 0, tab_cap = 0;
};
// The directory of a launch that needs room for `slots` keys of `kw` words.
// The workspace's record is taken down here (ws.valid) and put back by
// keydir_commit after the launch's last kernel is enqueued: an error return
// in between leaves a workspace that the next launch lays out and empties
// from scratch, whatever its buffers hold by then.  The directory is laid out
// anew and emptied, counters and all, when there is no valid record, when it
// or the key tables (aux, null for the certificates) were allocated again,
// when it has to grow, and when the knobs were reloaded.  OURO_KEY_CACHE=0
// empties its cells at every launch and lets the counters run on.  The
// per-call table (tab_cap entries at tab_off of tabbuf) is cleared from the
// host unless the record says that the launch before left this very table,
// in this very allocation, clear.
static int keydir_prepare(KeyDirWs& ws, size_t slots, size_t kw, bool extra, const Buf& tabbuf,
                          size_t tab_off, size_t tab_cap, KeyDir* out) {
  const bool was_valid = ws.valid;
  ws.valid = false;
  const unsigned long long epoch = knob_epoch();
  bool anew = !was_valid || slots > ws.slots || ws.epoch != epoch;
  if (anew) ws.slots = slots;
  const KcLayout L = kc_layout(ws.slots, kw, extra);
  int rc = ensure(ws.dir, L.bytes);
  if (rc) return rc;
  anew = anew || ws.dir.gen != ws.dir_gen;
  out->d = kc_dir(ws.dir.p, L, ws.slots);
  out->extra = extra ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws.dir.p) + L.off_extra)
                     : nullptr;
  out->restart = anew;
  out->empty = anew || !key_cache();
  out->clear_tab = out->empty || tabbuf.gen != ws.tab_gen || tab_off != ws.tab_off ||
                   tab_cap != ws.tab_cap;
  out->epoch = epoch;
  out->tab_gen = tabbuf.gen;
  out->tab_off = tab_off;
  out->tab_cap = tab_cap;
  return OURO_OK;
}
// the slots' payload buffer (the VRF key tables), ensured after keydir_prepare:
// allocated again, it holds no slot's table, so the directory starts over
static void keydir_aux(const KeyDirWs& ws, const Buf& aux, KeyDir* kd) {
  kd->aux_gen = aux.gen;
  if (aux.gen != ws.aux_gen) kd->restart = kd->empty = kd->clear_tab = true;
}
// every kernel of the launch is enqueued: the next launch may rely on it
static void keydir_commit(KeyDirWs& ws, const KeyDir& kd) {
  ws.epoch = kd.epoch;
  ws.dir_gen = ws.dir.gen;
  ws.tab_gen = kd.tab_gen;
  ws.aux_gen = kd.aux_gen;
  ws.tab_off = kd.tab_off;
  ws.tab_cap = kd.tab_cap;
  ws.valid = true;
}
// grids of the passes that clear: a few workgroups per CU at the most
static unsigned keydir_grid(size_t quads) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>((quads + kBlock - 1) / kBlock, 1024));
}
static int keydir_begin(hipStream_t st, const KeyDir& kd, uint32_t* table, size_t cap) {
  if (kd.restart)
    OURO_HIP(hipMemsetAsync(kd.d.hdr, 0, 4 * ((size_t)kKcWords + kd.d.mask + 1), st));
  else if (kd.empty)
    OURO_HIP(hipMemsetAsync(kd.d.cells, 0, 4 * ((size_t)kd.d.mask + 1), st));
  if (kd.clear_tab) OURO_HIP(hipMemsetAsync(table, 0, 4 * cap, st));
  hipLaunchKernelGGL(k_kc_begin, dim3(keydir_grid(cap / 4)), dim3(kBlock), 0, st, kd.d.hdr,
                     reinterpret_cast<uint4*>(table), cap / 4, kd.empty ? 1u : 0u);
  return OURO_OK;
}
static void keydir_reset(hipStream_t st, const KeyDir& kd, uint32_t* table, size_t cap,
                         bool regroup) {
  const size_t quads = std::max<size_t>(((size_t)kd.d.mask + 1) / 4, regroup ? cap / 4 : 0);
  hipLaunchKernelGGL(k_kc_reset, dim3(keydir_grid(quads)), dim3(kBlock), 0, st, kd.d,
                     reinterpret_cast<uint4*>(table), cap / 4, regroup ? 1u : 0u);
}

// epochs (device memory, tpraos.h EpochTab block; null = none): the batch's
// slots are looked up in it per header (kOptEpochs); the kernels find it where
// the single eta0 would be
int launch_hdr(hipStream_t st, const ouro_tpraos_batch& b_in, uint8_t* verdict, uint8_t* be,
               uint8_t* bl, const uint8_t* epochs) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  ouro_tpraos_batch b = b_in;
  uint32_t xopts = 0;
  if (epochs) {
    if (!b.slot) return fail(OURO_EINVAL, "an epoch schedule needs the headers' slots");
    b.epoch_nonce = epochs;
    xopts = kOptEpochs;
  }
  int grid;
  int32_t* scr;
  if (split_launch()) {
    // chunks of one resident grid of the pre / post kernels; per chunk the
    // six task slots of each header and its result record
    const size_t chunk = std::min<size_t>((b.n + kBlock - 1) / kBlock * kBlock,
                                          (size_t)ds->max_blocks[kHdrPre] * kBlock);
    const size_t words = (size_t)kHdrCores * slot_region_words(chunk, kSlotWords) +
                         slot_region_words(chunk, kHdrResWords);
    Buf& sb = ctx().scratch[st];
    if ((rc = ensure(sb, words * sizeof(int32_t)))) return rc;
    int32_t* tasks = static_cast<int32_t*>(sb.p);
    int32_t* res = tasks + (size_t)kHdrCores * slot_region_words(chunk, kSlotWords);
    const int gpp = (int)std::min<size_t>(chunk / kBlock, (size_t)ds->max_blocks[kHdrPre]);
    const int gpo = (int)std::min<size_t>(chunk / kBlock, (size_t)ds->max_blocks[kHdrPost]);
    const int gd = (int)std::min<size_t>((size_t)kHdrCores * chunk / kBlock,
                                         (size_t)ds->max_blocks[kHdrDsm]);
    for (size_t base = 0; base < b.n; base += chunk) {
      const size_t count = std::min(chunk, b.n - base);
      hipLaunchKernelGGL(k_hdr_pre, dim3(gpp), dim3(kBlock), 0, st, b, base, count, chunk, tasks,
                         res, ds->btab, xopts);
      hipLaunchKernelGGL(k_hdr_dsm, dim3(gd), dim3(kBlock), 0, st, count, chunk, (int)kHdrCores,
                         tasks, ds->btab);
      hipLaunchKernelGGL(k_hdr_post, dim3(gpo), dim3(kBlock), 0, st, b, base, count, chunk, tasks,
                         res, verdict, be, bl, xopts);
      if ((rc = launch_check())) return rc;
    }
    ctx().ocert[st].last = nullptr;
    ctx().vrfkey[st].last = nullptr;
    return OURO_OK;
  }
  // One OCERT verification per distinct certificate (see k_ocert_find); the
  // per-call table's entries are header index + 1 and its capacity 2n in 32
  // bits.  The directory holds as many certificates as the largest batch so
  // far has headers, 65,536 at the most.
  OcertWs& ow = ctx().ocert[st];
  ow.last = nullptr;
  const uint32_t* rep = nullptr;
  const uint8_t* ocert_ok = nullptr;
  const uint32_t* count = nullptr;
  const uint32_t hash_mask = ocert_hash_mask();
  KeyDir okd, vkd;  // committed to their workspaces after the last kernel is enqueued
  if (ocert_share() && b.n >= 1 && b.n <= ((size_t)1 << 30)) {
    size_t cap = 64;
    while (cap < 2 * b.n) cap <<= 1;
    // table | rep | uniq | ocert_ok
    const size_t bytes = 4 * cap + 4 * b.n + 4 * b.n + b.n;
    if ((rc = ensure(ow.buf, bytes))) return rc;
    uint32_t* table = static_cast<uint32_t*>(ow.buf.p);
    uint32_t* repw = table + cap;
    uint32_t* uniq = repw + b.n;
    uint8_t* okw = reinterpret_cast<uint8_t*>(uniq + b.n);
    if ((rc = keydir_prepare(ow.kd, std::min(cap / 2, kOcertDirSlots), kOcertKeyWords, false,
                             ow.buf, 0, cap, &okd)))
      return rc;
    // the unique lane kernel in the header kernel's scratch slots: both plans
    // before either launch, the pointer taken after the buffer last grew
    int gu;
    if ((rc = plan(ds, kOcertUnique, b.n, st, &gu, &scr))) return rc;
    if ((rc = plan(ds, kHdr, b.n, st, &grid, &scr, kHdrLaneWords))) return rc;
    const uint32_t wide_max = (uint32_t)std::min<size_t>(wide_small_max(), 0xffffffffu);
    const uint32_t share_max = (uint32_t)kOcertShareMax(b.n);
    const KeyDir& kd = okd;
    const uint32_t* work = kd.d.hdr + kKcWork;
    if ((rc = keydir_begin(st, kd, table, cap))) return rc;
    hipLaunchKernelGGL(k_ocert_find, dim3((unsigned)((b.n + kBlock - 1) / kBlock)), dim3(kBlock),
                       0, st, b, kd.d, table, (uint32_t)(cap - 1), hash_mask, repw, uniq, okw);
    hipLaunchKernelGGL(k_kc_decide, dim3(1), dim3(64), 0, st, kd.d.hdr, share_max, kd.d.slots, 0u,
                       0u);
    if (wide_max)
      hipLaunchKernelGGL(k_ocert_unique_wide, dim3(wide_grid(std::min<size_t>(b.n, wide_max))),
                         dim3(64), 0, st, b, work, uniq, okw, ds->btab, wide_max, share_max);
    hipLaunchKernelGGL(k_ocert_unique, dim3(gu), dim3(kBlock), 0, st, b, work, uniq, okw, scr,
                       ds->btab, wide_max, share_max);
    keydir_reset(st, kd, table, cap, false);
    hipLaunchKernelGGL(k_ocert_insert,
                       dim3((unsigned)((std::min<size_t>(b.n, kd.d.slots) + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, st, b, kd.d, hash_mask, uniq, okw);
    rep = repw;
    ocert_ok = okw;
    count = kd.d.hdr + kKcTotal;
    ow.last = count;
  } else if ((rc = plan(ds, kHdr, b.n, st, &grid, &scr, kHdrLaneWords))) {
    return rc;
  }
  // One fixed-base table of -Y per distinct VRF key (see k_vrfkey_base).  The
  // tables and their directory are laid out on the host for the largest kmax
  // so far (vrfkey_ws.h); the counts stay on the device and the kernels
  // compare this batch's with this batch's kmax.
  VrfKeyWs& kw = ctx().vrfkey[st];
  kw.last = nullptr;
  const VrfKeyShare* ks = nullptr;
  const VrfKeyLayout L =
      vrfkey_share() ? vrfkey_layout(b.n, kYKeyBytes, vrfkey_tab_bytes()) : VrfKeyLayout{};
  if (L.kmax) {
    if ((rc = ensure(kw.group, L.group_bytes))) return rc;
    uint8_t* g = static_cast<uint8_t*>(kw.group.p);
    VrfKeyShare* desc = reinterpret_cast<VrfKeyShare*>(g + L.off_desc);
    uint32_t* table = reinterpret_cast<uint32_t*>(g + L.off_table);
    uint32_t* krep = reinterpret_cast<uint32_t*>(g + L.off_rep);
    uint32_t* kuniq = reinterpret_cast<uint32_t*>(g + L.off_uniq);
    uint32_t* kidx = reinterpret_cast<uint32_t*>(g + L.off_kidx);
    KeyDir& kd = vkd;
    if ((rc = keydir_prepare(kw.kd, L.kmax, kVrfKeyWords, true, kw.group, L.off_table, L.cap, &kd)))
      return rc;
    // the slots' tables first (128-B entries on 128-B lines), their base points
    // after; a directory laid out anew has just been emptied, so no table of
    // the old allocation is looked for
    const size_t slots = kd.d.slots;
    if ((rc = ensure(kw.tables, slots * kYKeyBytes))) return rc;
    keydir_aux(kw.kd, kw.tables, &kd);
    int32_t* ktab = static_cast<int32_t*>(kw.tables.p);
    int32_t* kbase = ktab + slots * kYKeyWords;
    uint8_t* kflag = kd.d.val;
    uint32_t* nslot = kd.extra;
    const uint32_t kmax = (uint32_t)L.kmax;
    const uint32_t* work = kd.d.hdr + kKcWork;
    const unsigned gg = (unsigned)((b.n + kBlock - 1) / kBlock);
    if ((rc = keydir_begin(st, kd, table, L.cap))) return rc;
    hipLaunchKernelGGL(k_vrfkey_find, dim3(gg), dim3(kBlock), 0, st, b, kd.d, table,
                       (uint32_t)(L.cap - 1), hash_mask, krep, kuniq, kidx, 0u);
    hipLaunchKernelGGL(k_kc_decide, dim3(1), dim3(64), 0, st, kd.d.hdr, kmax, kd.d.slots, 1u, 0u);
    // new keys that do not fit: the directory emptied and every key of the
    // batch grouped and inserted again (three returns otherwise)
    keydir_reset(st, kd, table, L.cap, true);
    hipLaunchKernelGGL(k_vrfkey_find, dim3(gg), dim3(kBlock), 0, st, b, kd.d, table,
                       (uint32_t)(L.cap - 1), hash_mask, krep, kuniq, kidx, 1u);
    hipLaunchKernelGGL(k_kc_decide, dim3(1), dim3(64), 0, st, kd.d.hdr, kmax, kd.d.slots, 1u, 1u);
    // one wave per workgroup: the few lanes of a build spread over the CUs
    hipLaunchKernelGGL(k_vrfkey_insert, dim3((unsigned)((L.kmax + 63) / 64)), dim3(64), 0, st, b,
                       kd.d, hash_mask, kuniq, kidx, nslot);
    VrfKeyShare d;
    d.count = kd.d.hdr + kKcTotal;
    d.krep = krep;
    d.kidx = kidx;
    d.kflag = kflag;
    d.ktab = ktab;
    d.ubtab = ds->ubtab;
    d.kmax = kmax;
    hipLaunchKernelGGL(k_vrfkey_base, dim3((unsigned)((L.kmax + 63) / 64)), dim3(64), 0, st, b,
                       work, kuniq, nslot, kflag, kbase, kmax, d, desc);
    hipLaunchKernelGGL(k_vrfkey_fill, dim3((unsigned)((L.kmax + 63) / 64 * kYWindows)), dim3(64),
                       0, st, work, nslot, kbase, ktab, kmax);
    ks = desc;
    kw.last = d.count;
    kw.last_kmax = kmax;
  }
  hipLaunchKernelGGL(k_tpraos_verify, dim3(grid), dim3(kBlock), 0, st, b, verdict, be, bl, scr,
                     ds->btab, rep, ocert_ok, count, xopts, ks);
  if ((rc = launch_check())) return rc;
  if (count) keydir_commit(ow.kd, okd);
  if (ks) keydir_commit(kw.kd, vkd);
  return OURO_OK;
}

int launch_leader(hipStream_t st, size_t n, const uint8_t* beta, const uint64_t* num,
                  const uint64_t* den, int64_t lhi, uint64_t llo, int f_is_one,
                  uint8_t* verdict) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  int grid;
  if ((rc = plan(ds, kLeader, n, st, &grid, nullptr))) return rc;
  hipLaunchKernelGGL(k_leader_check, dim3(grid), dim3(kBlock), 0, st, n, beta, num, den, llo, lhi,
                     f_is_one ? 1u : 0u, verdict);
  return launch_check();
}

int lat_shape(size_t n_cap, LatShape* s) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  const int blk = lat_block();
  const size_t per = kBlock / blk;
  auto grid = [&](size_t items, int id) {
    size_t g = (items + blk - 1) / blk;
    return (int)std::max<size_t>(1, std::min<size_t>(g, (size_t)ds->max_blocks[id] * per));
  };
  const int quad = lat_quad();
  // the wide cores on one wave each (nwide n_cap waves, rounded to whole
  // workgroups) ahead of the other cores' lanes
  const int wmask = lat_wide_mask();
  const int nwide = __builtin_popcount((unsigned)wmask);
  // fused (all eight cores wide): the last core of a header finishes it, no
  // second launch (OURO_LAT_FUSE=0 keeps the finish launch, for A/B); its
  // items per header: kernels_lat.hip kFusedItems
  const bool fused = wmask == 0xff && lat_fuse();
  const size_t wide_waves = (size_t)(fused ? lat_fused_items_host() : nwide) * n_cap;
  const size_t wide_blocks = (wide_waves * 64 + blk - 1) / blk;
  const size_t quad_items = (size_t)(kLatCores - nwide) * n_cap;
  // timing probe: OURO_LAT_SKIP = mask of cores left out (verdicts then
  // wrong), honoured by the test-hook build only (runtime.cpp lat_skip_mask)
  const int skip = lat_skip_mask();
  s->g1 = (int)wide_blocks + grid(quad_items << (quad ? 2 : 0), kCores);
  s->g2 = grid(n_cap << (quad ? 2 : 0), kFinish);
  s->blk = blk;
  s->quad = quad;
  s->wide_lanes = (int)(wide_blocks * blk / 64);
  s->fused = fused;
  s->flags = (uint32_t)(quad | (skip << 8) | (wmask << 16) | (fused ? 1 << 24 : 0) |
                        (ouro_knobs::get().lat_stamps.load(std::memory_order_relaxed) ? 1 << 25 : 0));
  s->btab = ds->btab;
  return OURO_OK;
}

// (win_ctr / done: a plan's window counter and done word, or null)
void lat_issue(hipStream_t st, const LatShape& s, const ouro_tpraos_batch& b, const uint32_t* d_n,
               int32_t* res_buf, int32_t* scratch, uint8_t* verdict, uint8_t* be, uint8_t* bl,
               uint32_t* win_ctr, uint32_t* done) {
  hipLaunchKernelGGL(k_tpraos_cores, dim3(s.g1), dim3(s.blk), 0, st, b, d_n, res_buf, scratch,
                     s.btab, (int)s.flags, s.wide_lanes, verdict, be, bl, win_ctr, done);
  if (s.fused) return;
  hipLaunchKernelGGL(k_tpraos_finish, dim3(s.g2), dim3(s.blk), 0, st, b, d_n, res_buf, verdict, be,
                     bl, scratch, s.quad);
}

int launch_lowlat(hipStream_t st, const ouro_tpraos_batch& b, const uint32_t* d_n, size_t n_cap,
                  int32_t* res_buf, int32_t* scratch, uint8_t* verdict, uint8_t* be,
                  uint8_t* bl) {
  LatShape s;
  int rc = lat_shape(n_cap, &s);
  if (rc) return rc;
  lat_issue(st, s, b, d_n, res_buf, scratch, verdict, be, bl);
  return launch_check();
}

size_t lowlat_scratch_words(DeviceState* ds, size_t n_cap) {
  size_t b1 = std::min<size_t>(((size_t)kLatCores * n_cap + kBlock - 1) / kBlock,
                               (size_t)ds->max_blocks[kCores]);
  size_t b2 = std::min<size_t>((n_cap + kBlock - 1) / kBlock, (size_t)ds->max_blocks[kFinish]);
  return std::max<size_t>(1, std::max(b1, b2)) * kBlock * kSlotWords;
}

// ---- the kernels the runtime launches itself (the caller checks the launch:
// runtime.h launch_check) ----
void launch_tpraos_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                        const uint64_t* off, const uint32_t* len, size_t n, uint64_t spkp,
                        const cbor::Out& o, uint8_t* status) {
  hipLaunchKernelGGL(k_tpraos_pack, dim3(blocks), dim3(kBlock), 0, st, raw, raw_bytes, off, len, n,
                     spkp, o, status);
}
void launch_byron_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                       const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
                       const cbor::ByronOut& o, uint8_t* status) {
  hipLaunchKernelGGL(k_byron_pack, dim3(blocks), dim3(kBlock), 0, st, raw, raw_bytes, off, len, n,
                     magic, o, status);
}
void launch_vrf03_proof_to_hash(hipStream_t st, unsigned blocks, size_t n, const uint8_t* proof,
                                uint8_t* beta, uint8_t* verdict) {
  hipLaunchKernelGGL(k_vrf03_proof_to_hash, dim3(blocks), dim3(kBlock), 0, st, n, proof, beta,
                     verdict);
}
void launch_plan_stage(hipStream_t st, unsigned blocks, const uint4* src, uint4* dst, size_t n16,
                       uint64_t* stamp) {
  hipLaunchKernelGGL(k_plan_stage, dim3(blocks), dim3(256), 0, st, src, dst, n16, stamp);
}
void launch_plan_stage_ranges(hipStream_t st, unsigned blocks, const uint4* src, uint4* dst,
                              const PlanRanges& r, uint64_t* stamp) {
  hipLaunchKernelGGL(k_plan_stage_ranges, dim3(blocks), dim3(256), 0, st, src, dst, r, stamp);
}

// ---- whole-block storage integrity ----
void launch_block_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                       const uint64_t* off, const uint32_t* len, size_t n, uint64_t spkp,
                       const cbor::Out& o, const cbor::BlockOut& bo, uint8_t* status) {
  hipLaunchKernelGGL(k_block_pack, dim3(blocks), dim3(kBlock), 0, st, raw, raw_bytes, off, len, n,
                     spkp, o, bo, status);
}
// m messages hashed on `st`; work: cbor::b2b_work_bytes(m) bytes of device
// memory, 64-byte aligned (the permutation and its class counters).
// OURO_BLOCK_SORT=0: no ordering, lane j hashes item j (A/B).
int launch_blake2b(hipStream_t st, size_t m, const uint8_t* msg, size_t msg_bytes,
                   const uint64_t* off, const uint32_t* len, uint8_t* out, void* work) {
  if (m == 0) return OURO_OK;
  if (m > 0xffffffffull) return fail(OURO_EINVAL, "more than 2^32 - 1 messages");
  const unsigned blocks = (unsigned)std::min<size_t>((m + kBlock - 1) / kBlock, 4096);
  const uint32_t* perm = nullptr;
  if (ouro_knobs::get().block_sort.load(std::memory_order_relaxed) != 0) {
    uint32_t* p = static_cast<uint32_t*>(work);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(work) + cbor::a64(4 * m));
    hipLaunchKernelGGL(k_b2b_clear, dim3(1), dim3(64), 0, st, cnt);
    hipLaunchKernelGGL(k_b2b_count, dim3(blocks), dim3(kBlock), 0, st, m, len, cnt);
    hipLaunchKernelGGL(k_b2b_starts, dim3(1), dim3(64), 0, st, cnt);
    hipLaunchKernelGGL(k_b2b_scatter, dim3(blocks), dim3(kBlock), 0, st, m, len, cnt, p);
    perm = p;
  }
  const unsigned hblocks = (unsigned)std::min<size_t>((m + kB2bBlock - 1) / kB2bBlock, 1u << 20);
  hipLaunchKernelGGL(k_blake2b256, dim3(hblocks), dim3(kB2bBlock), 0, st, m, msg, msg_bytes, off,
                     len, perm, out);
  return launch_check();
}
// the header envelope of n raw headers on `st`: slicer, hashes, links
// (rec: n records of device memory, 64-byte aligned)
int launch_envelope(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                    const uint32_t* len, size_t n, const ouro_envelope_cfg& cfg,
                    const env::Rec& tip, env::Rec* rec, uint8_t* status, uint8_t* header_hash,
                    uint8_t* envelope, ouro_chain_tip* tip_out, env::Rec* ends) {
  if (n == 0) return OURO_OK;
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  const unsigned hblocks = (unsigned)std::min<size_t>((n + kB2bBlock - 1) / kB2bBlock, 1u << 20);
  hipLaunchKernelGGL(k_envelope_slice, dim3(blocks), dim3(kBlock), 0, st, raw, raw_bytes, off, len,
                     n, cfg.byron_epoch_slots, rec, status);
  hipLaunchKernelGGL(k_header_hash, dim3(hblocks), dim3(kB2bBlock), 0, st, n, raw, raw_bytes, rec);
  hipLaunchKernelGGL(k_envelope_link, dim3(blocks), dim3(kBlock), 0, st, n, rec, tip, cfg, envelope,
                     header_hash, tip_out, ends);
  return launch_check();
}
void launch_block_finish(hipStream_t st, unsigned blocks, size_t n, const uint8_t* status,
                         const uint8_t* digest, const uint8_t* claimed, const uint8_t* kes,
                         uint8_t* verdict, uint8_t* body_hash) {
  hipLaunchKernelGGL(k_block_finish, dim3(blocks), dim3(kBlock), 0, st, n, status, digest, claimed,
                     kes, verdict, body_hash);
}

}  // namespace ouro_rt

extern "C" {

// CLOCK PROBE (bench.py roofline.frac_clock): the last k_tpraos_verify
// launch's per-workgroup {s_memtime, s_memtime, s_memrealtime, s_memrealtime}
// at entry / exit, min(grid, max_slots) rows, from a -DOURO_CLOCK_STAMPS=1
// build (lib/libouro_verify_clock.so); -1 in the product build.
int ouro_debug_clock_stamps(unsigned long long* out, int max_slots) {
#if OURO_CLOCK_STAMPS
  if (!out || max_slots <= 0) return fail(OURO_EINVAL, "null buffer");
  const int n = std::min(max_slots, kClockSlots);
  if (hipDeviceSynchronize() != hipSuccess) return fail(OURO_EDEVICE, "sync");
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clock_stamps), sizeof(unsigned long long) * 4 * n) !=
      hipSuccess)
    return fail(OURO_EDEVICE, "hipMemcpyFromSymbol");
  return n;
#else
  (void)out;
  (void)max_slots;
  return -1;
#endif
}

}  // extern "C"
