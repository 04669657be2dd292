// plan.cpp -- latency plans (ouro_tpraos_plan_*): pinned staging of a window,
// its copy kernel and the latency kernels on the plan's own stream.  Host code
// only: kernels are reached through launches.h.  Compiled a second time with
// -DOURO_TEST_HOOKS=1 for lib/libouro_verify_test.so (plan_poison, the
// sentinel).
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "hooks.h"
#include "host_path.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"
#include "runtime.h"
#include "tpraos.h"

using namespace ouro;
using namespace ouro_rt;

// ---- plans: pinned staging, the window's copy kernel + latency kernel -------
// issued straight on the plan's stream per window (default), or replayed from
// one captured hipGraph (OURO_PLAN_GRAPH=1, A/B): the graph's GPU-side
// dispatch of its two kernel nodes cost 8-10 us more per window than two
// stream launches (profiles/r04m/ablat_plan_graph.json, lat_phases_graph.json).
// The packed input block: 16 bytes {n, option bits (tpraos.h kOpt*), the
// launch's generation (wide_cores.h arrive_last), 0}, then
// every member of ouro_tpraos_batch in order, each 16-byte aligned at
// capacity size; the output block: verdict | beta_eta | beta_leader | eta_nonce.
namespace {
constexpr int kPlanFields = 19;
// bytes per header of each member; 0 = the body (capacity-sized), -1 = a
// fixed 32 bytes (epoch_nonce)
constexpr int kFieldBytes[kPlanFields] = {32, 32, 80, 80, 32, 32, 32, 8, 8, 64,
                                          4,  448, 0, 8, 4, 64, 64, 8, -1};
enum PlanField { kFBody = 12, kFBodyOff = 13, kFEtaAlpha = 4, kFLeaderAlpha = 5, kFEpochNonce = 18 };
constexpr size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
}  // namespace

struct ouro_tpraos_plan {
  int dev = -1;
  size_t cap = 0, body_cap = 0;
  hipStream_t st = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
  size_t in_bytes = 0, out_bytes = 0;
  int32_t *res = nullptr, *scratch = nullptr;
  size_t off[kPlanFields] = {0};  // byte offsets of the members in the packed input block
  ouro_tpraos_batch dev_batch{};
  uint32_t gen = 0;             // generation of the last launch (arrive_last), 1..2^28-1
  size_t pending = 0;           // headers of the batch in flight (submit .. wait)
  uint8_t* nonce_dst = nullptr;  // that batch's eta_nonce (written by wait)
  uint32_t opts = 0;             // that batch's option bits (tpraos.h kOpt*)
  bool inflight = false;
  bool failed = false;           // its launch failed: wait recomputes it on the host path
  // TIMING PROBE (OURO_PLAN_TIMING set at submit; bench.py latency phases):
  // events around the window's launches on the plan's stream
  // (without the done word, the A/B forms: events around the launches; with
  // it, the kernels' own s_memrealtime stamps in the done block -- events
  // recorded every window made the runtime stall one submit in ~250 for
  // ~125 us, profiles/r06b/submit_probe.json)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  uint64_t* stamps = nullptr;  // device view of the done block's stamps (timing + flag)
  const volatile uint64_t* stamps_host = nullptr;
  bool timing = false;  // OURO_PLAN_TIMING at create
  float last_gpu_ms = -1.0f;
  float copy_us = -1.0f, launch_us = -1.0f;  // host side of its last submit
  int stage = 2;  // OURO_PLAN_STAGE at capture (plan_build)
  int spin = 0;   // OURO_PLAN_SPIN at capture: wait spins on hipStreamQuery
  int use_graph = 0;  // OURO_PLAN_GRAPH at build: 1 = the launches captured into one hipGraph
  void* hin = nullptr;  // device view of h_in (stage >= 1)
  uint8_t *dver = nullptr, *dbe = nullptr, *dbl = nullptr;  // the latency kernel's outputs
  LatShape shape;  // the latency launch at capacity (lat_shape, once)
  // OURO_PLAN_FLAG (default 1; stage 2, fused kernel): the latency kernel's
  // last header tail writes the generation into a done word in the pinned
  // output block, and wait spins on it instead of the stream's completion
  bool flag = false;
  uint32_t* done_dev = nullptr;              // that word as the kernel sees it
  const volatile uint32_t* done_host = nullptr;
  // the window's used byte ranges of the input block (recorded at submit):
  // the copy kernel moves those instead of the whole capacity block
  // (OURO_PLAN_TRIM=0 at create: the whole block, the round-4 form)
  bool trim = true;
  PlanRanges ranges{};
};

namespace {
void plan_free(ouro_tpraos_plan* p) {
  if (!p) return;
  // no DMA into freed staging (and, with the done word, a waited-for launch
  // may still be retiring its last waves)
  if (p->st) (void)hipStreamSynchronize(p->st);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  if (p->h_in) (void)hipHostFree(p->h_in);
  if (p->h_out) (void)hipHostFree(p->h_out);
  if (p->d_in) (void)hipFree(p->d_in);
  if (p->d_out) (void)hipFree(p->d_out);
  if (p->res) (void)hipFree(p->res);
  if (p->scratch) (void)hipFree(p->scratch);
  if (p->st) (void)hipStreamDestroy(p->st);
  delete p;
}

// the window's launches on the plan's stream: issued per submit (the
// default), or captured once into the graph (OURO_PLAN_GRAPH=1, A/B)
int plan_enqueue(ouro_tpraos_plan* p) {
  if ((p->stage == 1 || p->stage == 2) && p->ranges.count && !p->use_graph) {
    uint32_t units = 0;
    for (uint32_t k = 0; k < p->ranges.count; k++) units += p->ranges.len16[k];
    launch_plan_stage_ranges(p->st, (units + 255) / 256, static_cast<const uint4*>(p->hin),
                             reinterpret_cast<uint4*>(p->d_in), p->ranges, p->stamps);
  } else if (p->stage == 1 || p->stage == 2) {
    const size_t n16 = p->in_bytes / 16;  // in_bytes is a multiple of 16
    launch_plan_stage(p->st, (unsigned)((n16 + 255) / 256), static_cast<const uint4*>(p->hin),
                      reinterpret_cast<uint4*>(p->d_in), n16, p->stamps);
  } else if (p->stage <= 0) {
    OURO_HIP(hipMemcpyAsync(p->d_in, p->h_in, p->in_bytes, hipMemcpyHostToDevice, p->st));
  }
  const uint8_t* d = p->stage >= 3 ? static_cast<const uint8_t*>(p->hin) : p->d_in;
  // the window counter: word 3 of the input block, zeroed by the copy
  lat_issue(p->st, p->shape, p->dev_batch, reinterpret_cast<const uint32_t*>(d), p->res,
            p->scratch, p->dver, p->dbe, p->dbl,
            p->flag ? reinterpret_cast<uint32_t*>(p->d_in) + 3 : nullptr, p->done_dev);
  OURO_HIP(hipGetLastError());
  if (p->stage < 2)
    OURO_HIP(hipMemcpyAsync(p->h_out, p->d_out, p->out_bytes, hipMemcpyDeviceToHost, p->st));
  return OURO_OK;
}

size_t field_cap_bytes(const ouro_tpraos_plan* p, int f) {
  return kFieldBytes[f] > 0 ? (size_t)kFieldBytes[f] * p->cap
                            : (kFieldBytes[f] == 0 ? p->body_cap : 32);
}

int plan_build(ouro_tpraos_plan* p) {
  DeviceState* ds;
  int rc = device_state(&ds);
  if (rc) return rc;
  if ((rc = current_device(&p->dev))) return rc;
  OURO_HIP(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
  size_t o = 16;  // n and the option bits live in the first 16 bytes
  for (int f = 0; f < kPlanFields; f++) {
    p->off[f] = o;
    o += align16(field_cap_bytes(p, f));
  }
  p->in_bytes = o;
  p->out_bytes = align16(p->cap) + 160 * p->cap + 64;  // + the done word (OURO_PLAN_FLAG)
  OURO_HIP(hipHostMalloc(&p->h_in, p->in_bytes, hipHostMallocNumaUser));
  OURO_HIP(hipHostMalloc(&p->h_out, p->out_bytes, hipHostMallocNumaUser));
  OURO_HIP(hipMalloc(&p->d_in, p->in_bytes));
  OURO_HIP(hipMalloc(&p->d_out, p->out_bytes));
  OURO_HIP(hipMalloc(&p->res, sizeof(int32_t) * slot_region_words(p->cap, kLatResWords)));
  // the arrival records are generation-tagged (each submit bumps the plan's
  // generation) and never reset by the kernel; they start from zero once here
  OURO_HIP(hipMemset(p->res, 0, sizeof(int32_t) * slot_region_words(p->cap, kLatResWords)));
  OURO_HIP(hipMalloc(&p->scratch, sizeof(int32_t) * lowlat_scratch_words(ds, p->cap)));
  memset(p->h_in, 0, p->in_bytes);
  memset(p->h_out, 0, p->out_bytes);  // the done word starts at 0, never a generation
  // OURO_PLAN_STAGE (the window's copies, read here once): 0 = DMA copies in
  // and out; 1 = a copy kernel reads the pinned input block; 2 (default) =
  // that, and the latency kernel writes the results straight into the pinned
  // output block -- one node fewer, 2-3 us of the window (profiles/r04c:
  // ablat_plan_stage.json, lat_phases.json; the copy nodes' own time is
  // ~5 us each, the rest is the graph's node-to-node dispatch); 3 = no input
  // copy either: the latency kernel reads the pinned block over PCIe (A/B).
  // OURO_PLAN_GRAPH=1: capture them into a hipGraph (the form before r04m).
  const ouro_knobs::Knobs& kn = ouro_knobs::get();
  p->stage = kn.plan_stage.load(std::memory_order_relaxed);
  p->spin = kn.plan_spin.load(std::memory_order_relaxed);
  p->use_graph = kn.plan_graph.load(std::memory_order_relaxed) != 0;
  p->trim = kn.plan_trim.load(std::memory_order_relaxed) != 0;
  p->timing = kn.plan_timing.load(std::memory_order_relaxed) != 0;
  if (p->stage >= 1) OURO_HIP(hipHostGetDevicePointer(&p->hin, p->h_in, 0));
  uint8_t* d = p->stage >= 3 ? static_cast<uint8_t*>(p->hin) : p->d_in;
  ouro_tpraos_batch& b = p->dev_batch;
  b.n = p->cap;
  b.issuer_vk = d + p->off[0];
  b.vrf_vk = d + p->off[1];
  b.eta_proof = d + p->off[2];
  b.leader_proof = d + p->off[3];
  b.eta_alpha = d + p->off[4];
  b.leader_alpha = d + p->off[5];
  b.hot_vk = d + p->off[6];
  b.ocert_counter = reinterpret_cast<const uint64_t*>(d + p->off[7]);
  b.ocert_kes_period = reinterpret_cast<const uint64_t*>(d + p->off[8]);
  b.ocert_sigma = d + p->off[9];
  b.kes_t = reinterpret_cast<const uint32_t*>(d + p->off[10]);
  b.kes_sig = d + p->off[11];
  b.body = d + p->off[12];
  b.body_off = reinterpret_cast<const uint64_t*>(d + p->off[13]);
  b.body_len = reinterpret_cast<const uint32_t*>(d + p->off[14]);
  b.eta_output = d + p->off[15];
  b.leader_output = d + p->off[16];
  b.slot = reinterpret_cast<const uint64_t*>(d + p->off[17]);
  b.epoch_nonce = d + p->off[18];
  uint8_t* dver = p->d_out;
  uint8_t* dbe = dver + align16(p->cap);
  uint8_t* dbl = dbe + 64 * p->cap;
  b.eta_nonce = dbl + 64 * p->cap;  // written only when the option bit says so
  if (p->stage >= 2) {
    void* hout = nullptr;
    OURO_HIP(hipHostGetDevicePointer(&hout, p->h_out, 0));
    dver = static_cast<uint8_t*>(hout);
    dbe = dver + align16(p->cap);
    dbl = dbe + 64 * p->cap;
    b.eta_nonce = dbl + 64 * p->cap;
  }
  p->dver = dver;
  p->dbe = dbe;
  p->dbl = dbl;
  if ((rc = lat_shape(p->cap, &p->shape))) return rc;
  {
    p->flag = p->stage == 2 && p->shape.fused && kn.plan_flag.load(std::memory_order_relaxed) != 0;
    if (p->flag) {
      uint8_t* w = p->h_out + p->out_bytes - 64;
      void* wd = nullptr;
      OURO_HIP(hipHostGetDevicePointer(&wd, w, 0));
      p->done_dev = static_cast<uint32_t*>(wd);
      p->done_host = reinterpret_cast<const volatile uint32_t*>(w);
      if (p->timing) {
        // the done block: word 0 the done word; u64 1 the copy kernel's
        // start, u64 2 the latency kernel's start, u64 3 the last tail's end
        p->stamps = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(wd) + 8);
        p->stamps_host = reinterpret_cast<const volatile uint64_t*>(w + 8);
        p->shape.flags |= 1u << 26;
      }
    }
  }
  if (!p->use_graph) return OURO_OK;
  OURO_HIP(hipStreamBeginCapture(p->st, hipStreamCaptureModeThreadLocal));
  if ((rc = plan_enqueue(p))) {
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(p->st, &g);
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  OURO_HIP(hipStreamEndCapture(p->st, &p->graph));
  OURO_HIP(hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0));
  return OURO_OK;
}

// The batch in the plan's pinned input block as a host batch (the layout
// ouro_tpraos_plan_submit wrote), for the host recompute after a failed
// launch; results go straight to the caller's buffers.
ouro_tpraos_batch plan_host_batch(const ouro_tpraos_plan* p) {
  const uint8_t* h = p->h_in;
  ouro_tpraos_batch b{};
  b.n = p->pending;
  b.issuer_vk = h + p->off[0];
  b.vrf_vk = h + p->off[1];
  b.eta_proof = h + p->off[2];
  b.leader_proof = h + p->off[3];
  b.hot_vk = h + p->off[6];
  b.ocert_counter = reinterpret_cast<const uint64_t*>(h + p->off[7]);
  b.ocert_kes_period = reinterpret_cast<const uint64_t*>(h + p->off[8]);
  b.ocert_sigma = h + p->off[9];
  b.kes_t = reinterpret_cast<const uint32_t*>(h + p->off[10]);
  b.kes_sig = h + p->off[11];
  b.body = h + p->off[12];
  b.body_off = reinterpret_cast<const uint64_t*>(h + p->off[13]);
  b.body_len = reinterpret_cast<const uint32_t*>(h + p->off[14]);
  if (p->opts & kOptEtaClaim) b.eta_output = h + p->off[15];
  if (p->opts & kOptLeaderClaim) b.leader_output = h + p->off[16];
  if (p->opts & kOptSeeds) {
    b.slot = reinterpret_cast<const uint64_t*>(h + p->off[17]);
    if (p->opts & kOptEpochNonce) b.epoch_nonce = h + p->off[18];
  } else {
    b.eta_alpha = h + p->off[4];
    b.leader_alpha = h + p->off[5];
  }
  if (p->opts & kOptEtaNonce) b.eta_nonce = p->nonce_dst;
  return b;
}

// TEST HOOK (tests/test_gpu_claims.py::test_plan_counters_from_cut_off_launch;
// the test build only, OURO_TEST_HOOKS): OURO_TEST_PLAN_POISON set at
// ouro_tpraos_plan_submit leaves every arrival counter of the
// plan's records as a launch of its last generation would have left them had
// it been cut off one arrival short of each finish, so the test can show the
// next launch ignores them.
#if OURO_TEST_HOOKS
int plan_poison(ouro_tpraos_plan* p) {
  OURO_HIP(hipSetDevice(p->dev));
  OURO_HIP(hipStreamSynchronize(p->st));  // the last launch retired (done word: maybe not yet)
  const size_t words = slot_region_words(p->cap, kLatResWords);
  std::vector<int32_t> h(words);
  OURO_HIP(hipMemcpy(h.data(), p->res, sizeof(int32_t) * words, hipMemcpyDeviceToHost));
  const int32_t tag = (int32_t)((p->gen & 0x0fffffffu) << 4);
  for (size_t i = 0; i < p->cap; i++) {
    const Slot r = slot_of(h.data(), i, kLatResWords);
    *r.word(kLatCtr) = tag | (kLatCores - 1);     // the header's tail one arrival away
    *r.word(kLatCtr + 1) = tag | 1;                // each V / Gamma pair (or V / V2 /
    *r.word(kLatCtr + 2) = tag | 1;                // Gamma triple), one in
    for (int e = 0; e < 2; e++) {
      *r.word(kLatEd + kEdWords * e + 125) = tag | 1;  // each Ed25519 points / scalars pair
      for (int k = 17; k <= 19; k++)                // split form: the chain and done counters
        *r.word(kLatEd + kEdWords * e + k) = tag | 1;
    }
  }
  OURO_HIP(hipMemcpy(p->res, h.data(), sizeof(int32_t) * words, hipMemcpyHostToDevice));
  return OURO_OK;
}
#endif
}  // namespace

extern "C" {

ouro_tpraos_plan* ouro_tpraos_plan_create(size_t max_headers, size_t max_body_bytes) {
  if (max_headers == 0 || max_headers > 0xffffffffu) {
    fail(OURO_EINVAL, "bad plan size");
    return nullptr;
  }
  auto* p = new ouro_tpraos_plan;
  p->cap = max_headers;
  p->body_cap = std::max<size_t>(max_body_bytes, 16);
  if (plan_build(p) != OURO_OK) {
    plan_free(p);
    return nullptr;
  }
  return p;
}

int ouro_tpraos_plan_submit(ouro_tpraos_plan* p, const ouro_tpraos_batch* b) {
  if (!p || !b) return fail(OURO_EINVAL, "null argument");
  if (p->inflight) return fail(OURO_EINVAL, "the plan already has a batch in flight");
  const size_t n = b->n;
  if (n > p->cap) return fail(OURO_EINVAL, "batch larger than the plan");
  if (n == 0) {
    p->pending = 0;
    p->nonce_dst = nullptr;
    p->inflight = true;
    return OURO_OK;
  }
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, b->body_off, b->body_len, &w))) return rc;
  if (w.span() > p->body_cap) return fail(OURO_EINVAL, "body bytes exceed the plan");
  if (w.span() && !b->body) return fail(OURO_EINVAL, "null body buffer");
  const void* src[kPlanFields] = {
      b->issuer_vk,  b->vrf_vk,           b->eta_proof,   b->leader_proof, b->eta_alpha,
      b->leader_alpha, b->hot_vk,         b->ocert_counter, b->ocert_kes_period,
      b->ocert_sigma, b->kes_t,           b->kes_sig,     w.span() ? b->body + w.lo : nullptr,
      w.off.data(),  b->body_len,         b->eta_output,  b->leader_output, b->slot,
      b->epoch_nonce};
  p->timed = p->timing;
  const auto tc0 = std::chrono::steady_clock::now();
  if (b->slot) src[kFEtaAlpha] = src[kFLeaderAlpha] = nullptr;  // derived on the device
  else src[kFEpochNonce] = nullptr;
  bool trim = p->trim;
  p->ranges.count = 0;
  if (trim) {  // the block header: n, option bits, generation, window counter
    p->ranges.start16[0] = 0;
    p->ranges.len16[0] = 1;
    p->ranges.count = 1;
  }
  for (int f = 0; f < kPlanFields; f++) {
    const size_t bytes = kFieldBytes[f] > 0 ? (size_t)kFieldBytes[f] * n
                                            : (kFieldBytes[f] == 0 ? w.span() : 32);
    if (bytes && src[f]) {
      memcpy(p->h_in + p->off[f], src[f], bytes);
      if (trim) {
        PlanRanges& r = p->ranges;
        const uint32_t s16 = (uint32_t)(p->off[f] / 16), l16 = (uint32_t)((bytes + 15) / 16);
        if (r.start16[r.count - 1] + r.len16[r.count - 1] == s16) r.len16[r.count - 1] += l16;
        else if (r.count < (uint32_t)kPlanMaxRanges) {
          r.start16[r.count] = s16;
          r.len16[r.count++] = l16;
        } else {
          r.count = 0;  // (cannot happen: 19 members) copy the whole block
          trim = false;
        }
      }
    }
  }
  if (p->timed)
    p->copy_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - tc0).count();
#if OURO_TEST_HOOKS
  if (p->gen && ouro_knobs::get().test_plan_poison.load() && (rc = plan_poison(p))) return rc;
#endif
  // every launch a new generation, so no counter an earlier launch left
  // behind (one that never completed) is ever counted again
  p->gen = p->gen % 0x0fffffffu + 1u;
  p->opts = batch_opts(*b);
  const uint32_t nw[3] = {(uint32_t)n, p->opts, p->gen};
  memcpy(p->h_in, nw, sizeof nw);
  p->pending = n;
  p->nonce_dst = b->eta_nonce;
  p->failed = false;
#if OURO_TEST_HOOKS
  // TEST HOOK (tests/test_gpu_hooks_plan.py): every result byte of the pinned
  // output block (not the done word) set to a sentinel before the launch, so
  // a wait that returned before the kernel's stores were visible would hand
  // back the sentinel instead of the oracle's verdicts and outputs
  if (ouro_knobs::get().test_plan_sentinel.load()) memset(p->h_out, 0xEE, p->out_bytes - 64);
#endif
  const bool injected = injected_device_error();
  hipError_t e = hipSetDevice(p->dev);
  const bool events = p->timed && !p->stamps;
  if (events && !p->ev0 && e == hipSuccess) {
    e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
  }
  if (events && e == hipSuccess) e = hipEventRecord(p->ev0, p->st);
  const auto tl0 = std::chrono::steady_clock::now();
  if (e == hipSuccess && !injected) {
    if (p->exec) e = hipGraphLaunch(p->exec, p->st);
    else if (plan_enqueue(p) != OURO_OK) e = hipErrorLaunchFailure;
  }
  if (p->timed)
    p->launch_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - tl0).count();
  if (events && e == hipSuccess) e = hipEventRecord(p->ev1, p->st);
  if (e != hipSuccess || injected) {
    fail(OURO_EDEVICE, std::string("plan launch: ") +
                           (e != hipSuccess ? hipGetErrorString(e) : "injected device error"));
    if (!recompute_on_error()) return OURO_EDEVICE;
    p->failed = true;  // the inputs stay staged in h_in: wait verifies them on the host
  }
  p->inflight = true;
  return OURO_OK;
}

int ouro_tpraos_plan_wait(ouro_tpraos_plan* p, uint8_t* verdict, uint8_t* beta_eta,
                          uint8_t* beta_leader) {
  if (!p) return fail(OURO_EINVAL, "null plan");
  if (!p->inflight) return fail(OURO_EINVAL, "no batch in flight on this plan");
  const size_t n = p->pending;
  if (n && !verdict) return fail(OURO_EINVAL, "null verdict");
  p->inflight = false;
  if (n == 0) return OURO_OK;
  int rc = OURO_OK;
  if (!p->failed) {
    hipError_t e = hipSetDevice(p->dev);
    if (e == hipSuccess && p->flag) {
      // the kernel's done word; the stream is asked now and then, so a launch
      // that never writes it (a fault) still ends the wait with its error
      for (uint32_t k = 1;; k++) {
        if (*p->done_host == p->gen) break;
        if ((k & 255u) == 0) {
          e = hipStreamQuery(p->st);
          if (e != hipErrorNotReady) break;
          e = hipSuccess;
        }
        __builtin_ia32_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (e == hipSuccess && p->timed && !p->stamps) e = hipEventSynchronize(p->ev1);
    } else if (e == hipSuccess && p->spin) {
      // poll the stream instead of the runtime's wait, which may sleep on the
      // completion interrupt
      while ((e = hipStreamQuery(p->st)) == hipErrorNotReady) __builtin_ia32_pause();
    }
    if (e == hipSuccess && !p->flag) e = hipStreamSynchronize(p->st);
    if (e != hipSuccess) rc = fail(OURO_EDEVICE, std::string("plan wait: ") + hipGetErrorString(e));
  } else {
    rc = OURO_EDEVICE;
  }
  if (rc) {
    const ouro_tpraos_batch hb = plan_host_batch(p);
    p->nonce_dst = nullptr;
    p->failed = false;
    return or_host(rc, [&] { return ouro_host::hdr_batch(&hb, verdict, beta_eta, beta_leader); });
  }
  p->last_gpu_ms = -1.0f;
  if (p->timed && p->stamps) {
    // the copy kernel's start to the last header's end, 100 MHz ticks
    const uint64_t t0 = p->stamps_host[0], t2 = p->stamps_host[2];
    p->last_gpu_ms = t2 > t0 ? (float)((double)(t2 - t0) * 1e-5) : -1.0f;
  } else if (p->timed) {
    (void)hipEventElapsedTime(&p->last_gpu_ms, p->ev0, p->ev1);
  }
  const uint8_t* o = p->h_out + align16(p->cap);
  memcpy(verdict, p->h_out, n);
  if (beta_eta) memcpy(beta_eta, o, 64 * n);
  if (beta_leader) memcpy(beta_leader, o + 64 * p->cap, 64 * n);
  if (p->nonce_dst) memcpy(p->nonce_dst, o + 128 * p->cap, 32 * n);
  p->nonce_dst = nullptr;
  return OURO_OK;
}

int ouro_tpraos_plan_run(ouro_tpraos_plan* p, const ouro_tpraos_batch* b, uint8_t* verdict,
                         uint8_t* beta_eta, uint8_t* beta_leader) {
  if (!p || !b || !verdict) return fail(OURO_EINVAL, "null argument");
  if (b->n == 0) return OURO_OK;
  int rc = ouro_tpraos_plan_submit(p, b);
  if (rc) return rc;
  return ouro_tpraos_plan_wait(p, verdict, beta_eta, beta_leader);
}

void ouro_tpraos_plan_destroy(ouro_tpraos_plan* p) { plan_free(p); }

// TIMING PROBE (tools/lat_stamps.py): header 0's per-item stamps of the last
// fused latency launch, 16 items x 24 tags of s_memrealtime (100 MHz), from a
// library built with -DOURO_LAT_STAMPS=1 and run with OURO_LAT_STAMPS set;
// returns the count, or -1 in the product build.
int ouro_debug_lat_stamps(unsigned long long* out) { return lat_stamps_read(out); }

// TIMING PROBE: the GPU time of the plan's last waited-for window (events
// around its launches: input copy, the latency kernel, output), recorded when
// OURO_PLAN_TIMING was set at its submit; -1 otherwise.
int ouro_debug_plan_timing(ouro_tpraos_plan* p, float* gpu_ms, float* copy_us, float* launch_us) {
  if (!p) return fail(OURO_EINVAL, "null plan");
  if (gpu_ms) *gpu_ms = p->last_gpu_ms;
  if (copy_us) *copy_us = p->timed ? p->copy_us : -1.0f;
  if (launch_us) *launch_us = p->timed ? p->launch_us : -1.0f;
  return OURO_OK;
}

}  // extern "C"
