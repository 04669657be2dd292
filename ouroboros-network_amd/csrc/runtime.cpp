// runtime.cpp -- the host runtime under the C ABI (runtime.h): last error,
// device state, the per-thread context pool, staging, the knob accessors, and
// the entries that are about the runtime itself (ouro_set_device,
// ouro_last_error, the debug getters).  Compiled for the host only, and a
// second time with -DOURO_TEST_HOOKS=1 for lib/libouro_verify_test.so.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "../../include/ouro_verify_debug.h"
#include "hooks.h"
#include "host_path.h"
#include "key_cache.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"

using namespace ouro;

// ---------------------------------------------------------------- runtime ----

namespace ouro_rt {

thread_local std::string t_last_error;
namespace {
thread_local int t_device = -1;
std::mutex g_dev_mu;
std::map<int, DeviceState> g_dev;
}  // namespace

int fail(int code, const std::string& what) {
  t_last_error = what;
  return code;
}

// ---- NUMA placement (numa.cpp) ----
// the NUMA node of device `dev` (sysfs numa_node of its PCI function), -1 if unknown
int device_numa_node(int dev) {
  char busid[64] = {0};
  if (hipDeviceGetPCIBusId(busid, (int)sizeof(busid), dev) != hipSuccess) return -1;
  return ouro_numa::node_of_pci(busid);
}

int current_device(int* dev) {
  // no usable device at all is OURO_ENODEV (not a device error: nothing is
  // recomputed on the host path behind the caller's back)
  auto nodev = [](hipError_t e) {
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver;
  };
  if (t_device < 0) {
    int d = 0;
    const hipError_t e = hipGetDevice(&d);
    if (nodev(e)) return fail(OURO_ENODEV, std::string("hipGetDevice: ") + hipGetErrorString(e));
    OURO_HIP(e);
    t_device = d;
  }
  const hipError_t e = hipSetDevice(t_device);
  if (nodev(e)) return fail(OURO_ENODEV, std::string("hipSetDevice: ") + hipGetErrorString(e));
  OURO_HIP(e);
  *dev = t_device;
  return OURO_OK;
}

int device_state(DeviceState** out) {
  int dev;
  int rc = current_device(&dev);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(g_dev_mu);
  DeviceState& s = g_dev[dev];
  if (!s.ready) {
    hipDeviceProp_t prop;
    OURO_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      return fail(OURO_ENODEV, std::string("device is ") + prop.gcnArchName + ", need gfx950");
    s.cus = prop.multiProcessorCount;
    // niels B tables, then their wave-wide form (latency mode, wide.h), then
    // the doubling-free U chain's table (built once per process)
    static const std::vector<int32_t>* const utab = [] {
      auto* t = new std::vector<int32_t>(kUBTabWords);
      build_ubtab(t->data());
      return t;
    }();
    std::vector<int32_t> tab(kBTabWords + kBTabWideWords + kUBTabWords);
    memcpy(tab.data() + kBTabWords + kBTabWideWords, utab->data(), sizeof(int32_t) * kUBTabWords);
    memcpy(tab.data(), ouro_host::btab(), sizeof(int32_t) * kBTabWords);  // built once per process
    build_btab_wide(reinterpret_cast<uint16_t*>(tab.data() + kBTabWords), tab.data());
    OURO_HIP(hipMalloc(&s.btab, sizeof(int32_t) * tab.size()));
    OURO_HIP(hipMemcpy(s.btab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
    s.ubtab = s.btab + kBTabWords + kBTabWideWords;
    for (int id = 0; id < kNumKernels; id++) {
      int per_cu = 0;
      OURO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_ptr(id), kBlock, 0));
      s.max_blocks[id] = std::max(1, per_cu) * s.cus;
    }
    s.ready = true;
  }
  *out = &s;
  return OURO_OK;
}

namespace {
struct CtxPool {
  std::mutex mu;
  std::map<int, std::vector<ThreadCtx*>> free;  // per device
  std::map<int, size_t> created;
};
CtxPool& ctx_pool() {
  static CtxPool* p = new CtxPool;  // leaked on purpose (runtime.h ThreadCtx)
  return *p;
}
struct Lease {
  std::map<int, ThreadCtx*> held;  // device -> the context this thread borrowed
  ~Lease() {
    if (held.empty()) return;
    CtxPool& P = ctx_pool();
    std::lock_guard<std::mutex> g(P.mu);
    for (auto& kv : held) P.free[kv.first].push_back(kv.second);
  }
};
thread_local Lease t_lease;
}  // namespace

// the calling thread's context on device `dev`
ThreadCtx& ctx_of(int dev) {
  auto it = t_lease.held.find(dev);
  if (it != t_lease.held.end()) return *it->second;
  ThreadCtx* c = nullptr;
  {
    CtxPool& P = ctx_pool();
    std::lock_guard<std::mutex> g(P.mu);
    std::vector<ThreadCtx*>& v = P.free[dev];
    if (!v.empty()) {
      c = v.back();
      v.pop_back();
    } else {
      c = new ThreadCtx;
      P.created[dev]++;
    }
  }
  t_lease.held[dev] = c;
  return *c;
}
// ... on its current device (valid after current_device())
ThreadCtx& ctx() { return ctx_of(t_device); }

int ensure(Buf& b, size_t bytes) {
  if (b.cap >= bytes) return OURO_OK;
  if (b.p) OURO_HIP(hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  size_t want = std::max<size_t>(bytes, 4096);
  OURO_HIP(hipMalloc(&b.p, want));
  b.cap = want;
  b.gen++;
  return OURO_OK;
}

int thread_stream(hipStream_t* s) {
  int dev;
  int rc = current_device(&dev);
  if (rc) return rc;
  ThreadCtx& c = ctx_of(dev);
  if (c.stream == nullptr) OURO_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
  *s = c.stream;
  return OURO_OK;
}

// grid for n items of kernel `id`; returns the scratch slot count
int plan(DeviceState* ds, int id, size_t n, hipStream_t stream, int* grid, int32_t** scratch,
         int lane_words) {
  size_t blocks = (n + kBlock - 1) / kBlock;
  blocks = std::max<size_t>(1, std::min<size_t>(blocks, (size_t)ds->max_blocks[id]));
  *grid = (int)blocks;
  if (scratch) {
    Buf& b = ctx().scratch[stream];
    int rc = ensure(b, blocks * kBlock * sizeof(int32_t) * lane_words);
    if (rc) return rc;
    *scratch = static_cast<int32_t*>(b.p);
  }
  return OURO_OK;
}

// (hooks.h: injected_device_error)

int launch_check() {
  OURO_HIP(hipGetLastError());
  if (injected_device_error()) return fail(OURO_EDEVICE, "injected device error (OURO_TEST_DEVICE_ERROR)");
  return OURO_OK;
}

std::atomic<unsigned long long> g_host_single{0}, g_host_recompute{0};
bool recompute_on_error() {
  return !ouro_knobs::get().on_device_error_fail.load(std::memory_order_relaxed);
}
// Single items run on the host path (one GPU round trip is ~220-420 us, the
// host path ~1.5x libsodium); OURO_SINGLE_ITEM=gpu sends them to the device
// (A/B, bench.py single_item).
bool single_on_gpu() { return ouro_knobs::get().single_on_gpu.load(std::memory_order_relaxed); }

// Small batches (n <= OURO_WIDE_SMALL_MAX, default 2048; 0 = never) run one
// item per wave (kernels_lat.hip k_ed25519_wide / k_vrf03_wide): a single
// item's latency is then one wave's chain, not one lane's.
size_t wide_small_max() { return ouro_knobs::get().wide_small_max.load(std::memory_order_relaxed); }

// ---- the split kernels' switch ----
// The split kernels (pre / dsm at OURO_DSM_WAVES / post) instead of the
// one-pass k_tpraos_verify, k_ed25519_verify and k_sum6kes_verify (measured
// and rejected): fixed at compile time in the product
// (OURO_SPLIT_DEFAULT); only the test-hook build lets OURO_SPLIT=1 select them
// (tests/test_gpu_variants.py keeps them bit-exact).
#ifndef OURO_SPLIT_DEFAULT
#define OURO_SPLIT_DEFAULT 0
#endif
bool split_launch() {
#if OURO_TEST_HOOKS
  if (ouro_knobs::get().split.load(std::memory_order_relaxed)) return true;
#endif
  return OURO_SPLIT_DEFAULT != 0;
}

// Header batches verify each distinct operational certificate once
// (kernels.hip k_ocert_group; OURO_OCERT_SHARE=0: every header's own check,
// with no group or unique pass).
bool ocert_share() { return ouro_knobs::get().ocert_share.load(std::memory_order_relaxed) != 0; }

// Header batches build one fixed-base table of -Y per distinct VRF key and
// run both U cores from it (kernels.hip k_vrfkey_base; OURO_VRFKEY_SHARE=0:
// every header's own doubling chain, with no group or build pass).  The
// tables of one stream take at most OURO_VRFKEY_TAB_MB (default 512, which
// holds 5,900 keys at width 6); a batch with more distinct keys than fit, or
// with fewer than vrfkey_ws.h kVrfKeyMinPerKey headers per key, runs inline.
bool vrfkey_share() { return ouro_knobs::get().vrfkey_share.load(std::memory_order_relaxed) != 0; }
size_t vrfkey_tab_bytes() {
  const long long mb = ouro_knobs::get().vrfkey_tab_mb.load(std::memory_order_relaxed);
  return mb <= 0 ? 0 : (size_t)std::min<long long>(mb, 1ll << 20) << 20;
}

// The verdict of each distinct certificate and the table of each distinct VRF
// key are kept per stream from one header launch to the next (key_cache.h;
// kernels.hip k_kc_begin).  OURO_KEY_CACHE=0: every launch starts from empty
// directories and works everything out again, for an A/B in one process.
// knob_epoch: the directories are emptied when the knobs are reloaded.
bool key_cache() { return ouro_knobs::get().key_cache.load(std::memory_order_relaxed) != 0; }
unsigned long long knob_epoch() { return ouro_knobs::epoch(); }

// The bits of the certificate hash the group pass uses.  The test-hook build
// narrows them (OURO_TEST_OCERT_HASH_BITS=k) so that a few hundred headers
// exercise probe chains and the probe cap; the product uses all of them.
uint32_t ocert_hash_mask() {
#if OURO_TEST_HOOKS
  const int k = ouro_knobs::get().test_ocert_hash_bits.load(std::memory_order_relaxed);
  if (k > 0 && k < 32) return (1u << k) - 1u;
#endif
  return 0xffffffffu;
}

// Workgroup size of the latency-mode launches (OURO_LAT_BLOCK = 64/128/256).
// A small window fills only a few waves; one-wave workgroups spread them over
// as many CUs (own L1, TA and instruction fetch per wave) instead of packing
// four onto each CU.
int lat_block() {
  const int v = ouro_knobs::get().lat_block.load(std::memory_order_relaxed);
  return v == 64 || v == 128 || v == 256 ? v : kLatBlock;
}

// Latency-mode cores on lane quads (1, default) or one lane per core
// (OURO_LAT_QUAD=0, for A/B).
int lat_quad() { return ouro_knobs::get().lat_quad.load(std::memory_order_relaxed) != 0; }

// Latency-mode cores run on one wave each (wide_cores.h): a mask over
// tpraos.h HdrCore + kCoreGe/kCoreGl, default all eight (OURO_LAT_WIDE; 0 =
// every core on lane quads, for A/B).
int lat_wide_mask() { return ouro_knobs::get().lat_wide.load(std::memory_order_relaxed) & 0xff; }

int lat_fuse() { return ouro_knobs::get().lat_fuse.load(std::memory_order_relaxed) != 0; }

// timing probe: OURO_LAT_SKIP = mask of cores left out (verdicts then
// wrong), honoured by the test-hook build only
int lat_skip_mask() {
#if OURO_TEST_HOOKS
  return ouro_knobs::get().lat_skip.load(std::memory_order_relaxed) & 0xff;
#else
  return 0;
#endif
}

// Window of a batch (see struct Window); EINVAL when an offset + length
// overflows.
int window_of(size_t n, const uint64_t* off, const uint32_t* len, Window* w) {
  uint64_t lo = ~0ull, hi = 0;
  for (size_t i = 0; i < n; i++) {
    if (!len[i]) continue;
    const uint64_t e = off[i] + len[i];
    if (e < off[i]) return fail(OURO_EINVAL, "offset + length overflows");
    lo = std::min(lo, off[i]);
    hi = std::max(hi, e);
  }
  if (hi == 0) lo = 0;
  w->lo = lo;
  w->hi = hi;
  w->off.resize(n);
  for (size_t i = 0; i < n; i++) w->off[i] = len[i] ? off[i] - lo : 0;
  return OURO_OK;
}

int finish(hipStream_t st) {
  OURO_HIP(hipStreamSynchronize(st));
  return OURO_OK;
}

int download(hipStream_t st, void* host, const void* dev, size_t bytes) {
  if (!host || !bytes) return OURO_OK;
  OURO_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
  return OURO_OK;
}

// ---- header batches ----
// The required members present?  (The alphas only when the batch has no slots.)
int check_hdr_batch(const ouro_tpraos_batch* b) {
  if (!b->issuer_vk || !b->vrf_vk || !b->eta_proof || !b->leader_proof || !b->hot_vk ||
      !b->ocert_counter || !b->ocert_kes_period || !b->ocert_sigma || !b->kes_t || !b->kes_sig ||
      !b->body_off || !b->body_len)
    return fail(OURO_EINVAL, "null argument");
  if (!b->slot && (!b->eta_alpha || !b->leader_alpha))
    return fail(OURO_EINVAL, "null alpha (and no slots to derive it from)");
  return OURO_OK;
}

int stage_hdr(Stager& sg, const ouro_tpraos_batch* b, size_t lo, size_t m, StagedHdr* s) {
  int rc = window_of(m, b->body_off + lo, b->body_len + lo, &s->body);
  if (rc) return rc;
  const size_t span = s->body.span();
  if (span && !b->body) return fail(OURO_EINVAL, "null body buffer");
  ouro_tpraos_batch& d = s->d;
  d = ouro_tpraos_batch{};
  d.n = m;
  d.issuer_vk = sg.up(b->issuer_vk + 32 * lo, 32 * m);
  d.vrf_vk = sg.up(b->vrf_vk + 32 * lo, 32 * m);
  d.eta_proof = sg.up(b->eta_proof + 80 * lo, 80 * m);
  d.leader_proof = sg.up(b->leader_proof + 80 * lo, 80 * m);
  if (b->slot) {
    d.slot = sg.up(b->slot + lo, m);
    if (b->epoch_nonce) d.epoch_nonce = sg.up(b->epoch_nonce, 32);
  } else {
    d.eta_alpha = sg.up(b->eta_alpha + 32 * lo, 32 * m);
    d.leader_alpha = sg.up(b->leader_alpha + 32 * lo, 32 * m);
  }
  d.hot_vk = sg.up(b->hot_vk + 32 * lo, 32 * m);
  d.ocert_counter = sg.up(b->ocert_counter + lo, m);
  d.ocert_kes_period = sg.up(b->ocert_kes_period + lo, m);
  d.ocert_sigma = sg.up(b->ocert_sigma + 64 * lo, 64 * m);
  d.kes_t = sg.up(b->kes_t + lo, m);
  d.kes_sig = sg.up(b->kes_sig + 448 * lo, 448 * m);
  d.body = sg.up(span ? b->body + s->body.lo : b->body, span);
  d.body_off = sg.up(s->body.off.data(), m);
  d.body_len = sg.up(b->body_len + lo, m);
  if (b->eta_output) d.eta_output = sg.up(b->eta_output + 64 * lo, 64 * m);
  if (b->leader_output) d.leader_output = sg.up(b->leader_output + 64 * lo, 64 * m);
  s->ver = sg.out<uint8_t>(m);
  s->be = sg.out<uint8_t>(64 * m);
  s->bl = sg.out<uint8_t>(64 * m);
  if (b->eta_nonce) d.eta_nonce = s->nonce = sg.out<uint8_t>(32 * m);
  return sg.rc;
}

}  // namespace ouro_rt

using namespace ouro_rt;

// ---------------------------------------------------------------- C ABI ------
extern "C" {

int ouro_set_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
    return fail(OURO_ENODEV, "no such device");
  t_device = device;
  return OURO_OK;
}

const char* ouro_last_error(void) { return t_last_error.c_str(); }

// DIAGNOSTIC: 1 in the test-hook build (lib/libouro_verify_test.so), 0 in the product
int ouro_debug_test_hooks(void) { return OURO_TEST_HOOKS; }

void ouro_debug_reload_knobs(void) { ouro_knobs::reload(); }

// Items the host path has verified: single items routed there, and host-
// buffer batches recomputed there after a device error.
int ouro_debug_host_path(unsigned long long* single_items, unsigned long long* recomputed_batches) {
  if (single_items) *single_items = g_host_single.load();
  if (recomputed_batches) *recomputed_batches = g_host_recompute.load();
  return OURO_OK;
}

// DIAGNOSTIC (tests): the distinct operational certificates the last header
// launch of the calling thread on `stream` found (runtime.h OcertWs); 0 when
// that launch did not share.  Synchronises the stream.
int ouro_debug_last_ocert_groups(void* stream) {
  int dev;
  int rc = current_device(&dev);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ThreadCtx& c = ctx_of(dev);
  auto it = c.ocert.find(st);
  if (it == c.ocert.end() || !it->second.last) return 0;
  OURO_HIP(hipStreamSynchronize(st));
  uint32_t count = 0;
  OURO_HIP(hipMemcpy(&count, it->second.last, sizeof count, hipMemcpyDeviceToHost));
  return (int)count;
}

// DIAGNOSTIC (tests): the distinct VRF keys the last header launch of the
// calling thread on `stream` found (runtime.h VrfKeyWs), and in *shared
// whether that launch ran the U cores from per-key tables; 0 and not shared
// when it did no grouping.  Synchronises the stream.
int ouro_debug_last_vrfkey_groups(void* stream, int* shared) {
  if (shared) *shared = 0;
  int dev;
  int rc = current_device(&dev);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ThreadCtx& c = ctx_of(dev);
  auto it = c.vrfkey.find(st);
  if (it == c.vrfkey.end() || !it->second.last) return 0;
  OURO_HIP(hipStreamSynchronize(st));
  uint32_t count = 0;
  OURO_HIP(hipMemcpy(&count, it->second.last, sizeof count, hipMemcpyDeviceToHost));
  if (shared) *shared = count <= it->second.last_kmax ? 1 : 0;
  return (int)count;
}

// DIAGNOSTIC (tests, tools): the key directories of the calling thread on
// `stream` (runtime.h KeyDirWs, key_cache.h): out = {VRF keys resident, built
// by the last launch, times emptied; the same three for certificates; the
// generation; 0}.  Zeros for a directory that does not exist yet.
// OURO_DEBUG_ALL_STREAMS: the sums over every stream of the thread's context
// (the host-buffer entries' own streams among them), the largest generation.
// Synchronises the stream(s).
int ouro_debug_key_cache(void* stream, uint64_t out[8]) {
  if (!out) return fail(OURO_EINVAL, "null argument");
  std::fill(out, out + 8, (uint64_t)0);
  int dev;
  int rc = current_device(&dev);
  if (rc) return rc;
  ThreadCtx& c = ctx_of(dev);
  // (a directory a knob reload has overtaken is emptied by its next launch:
  // it counts as empty here)
  auto read = [&](hipStream_t st, const KeyDirWs& kd, uint64_t* o) -> int {
    if (!kd.dir.p || !kd.slots || !kd.valid || kd.epoch != knob_epoch()) return OURO_OK;
    OURO_HIP(hipStreamSynchronize(st));
    uint32_t hdr[ouro::kKcWords];
    OURO_HIP(hipMemcpy(hdr, kd.dir.p, sizeof hdr, hipMemcpyDeviceToHost));
    o[0] += hdr[ouro::kKcResident];
    o[1] += hdr[ouro::kKcBuilt];
    o[2] += hdr[ouro::kKcEmptied];
    out[6] = std::max<uint64_t>(out[6], hdr[ouro::kKcGen]);
    return OURO_OK;
  };
  const bool all = stream == OURO_DEBUG_ALL_STREAMS;
  for (auto& kv : c.vrfkey)
    if ((all || kv.first == static_cast<hipStream_t>(stream)) &&
        (rc = read(kv.first, kv.second.kd, out)))
      return rc;
  for (auto& ko : c.ocert)
    if ((all || ko.first == static_cast<hipStream_t>(stream)) &&
        (rc = read(ko.first, ko.second.kd, out + 3)))
      return rc;
  return OURO_OK;
}

// Contexts of the per-thread pool on `device` (runtime.h ThreadCtx):
// created so far and idle (returned by exited threads).
int ouro_debug_contexts(int device, size_t* created, size_t* idle) {
  CtxPool& P = ctx_pool();
  std::lock_guard<std::mutex> g(P.mu);
  if (created) *created = P.created[device];
  if (idle) *idle = P.free[device].size();
  return OURO_OK;
}

}  // extern "C"
