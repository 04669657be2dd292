// runtime.h -- the host runtime under the C ABI (runtime.cpp), shared by the
// host units (api_batch.cpp, raw_pipe.cpp, raw_host.cpp, chain_api.cpp,
// plan.cpp, multi.cpp and the *_api.cpp units) and by the launch functions of
// the kernel units: the thread's last error, the per-device state, the pooled
// per-thread contexts and their staging (the raw-CBOR pipeline's slots among
// them), the host-path recompute after a device error, and the knob
// accessors.  What one raw-CBOR call is made of is raw_call.h; the steps the
// entries share are host_util.h.  Everything here is internal to the library
// (hidden visibility) and host code: the host units are compiled host-only
// (launch.h is included for the slot sizes).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "launch.h"

// numa.cpp: NUMA placement of a device's host side
namespace ouro_numa {
int node_of_pci(const char* busid);
int bind_thread(int node);
}  // namespace ouro_numa

#pragma GCC visibility push(hidden)
namespace ouro_rt {

// the calling thread's last error (ouro_last_error)
extern thread_local std::string t_last_error;
int fail(int code, const std::string& what);

#define OURO_HIP(call)                                                               \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess)                                                            \
      return fail(OURO_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct DeviceState {
  bool ready = false;
  int err = OURO_OK;
  std::string err_msg;
  int32_t* btab = nullptr;
  int32_t* ubtab = nullptr;  // inside btab's allocation: the U chain's table (verify.h build_ubtab)
  int cus = 0;
  int max_blocks[16] = {0};  // per KernelId (kNumKernels <= 16)
};

// the NUMA node of device `dev` (sysfs numa_node of its PCI function), -1 if unknown
int device_numa_node(int dev);
int current_device(int* dev);
int device_state(DeviceState** out);

// Per-thread, per-DEVICE stream and growable device buffers: a buffer
// allocated on one GPU is never handed to a launch on another, whatever the
// order of ouro_set_device calls or of a multi-GPU call's device list.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  // allocations so far (ensure): what was written into an earlier allocation
  // is gone even when the new one comes back at the same address
  unsigned long long gen = 0;
};

// The bytes a batch addresses by (offset, length) pairs: the window
// [lo, hi) over the items with length > 0, and the offsets rebased to lo, so
// only that window is uploaded (a slice or shard of a larger batch with
// absolute offsets does not drag the bytes before it along).
struct Window {
  uint64_t lo = 0, hi = 0;
  std::vector<uint64_t> off;  // rebased; alive until the upload has completed
  size_t span() const { return (size_t)(hi - lo); }
};

// rows [lo, lo + m) of a host batch on the device: `d` points at the copies
// (optional members only when given), ver/be/bl/nonce at the result buffers
struct StagedHdr {
  ouro_tpraos_batch d{};
  uint8_t *ver = nullptr, *be = nullptr, *bl = nullptr, *nonce = nullptr;
  Window body;
};

// ---- pipelined host-buffer header batches (state) ----
// A large batch from pageable host memory is cut into chunks of one full grid
// of lanes.  Two slots (stream, device buffers, pinned result staging) take
// turns: while chunk c's kernel runs on one stream, the host uploads chunk
// c + 1 on the other and copies chunk c - 1's results out, so PCIe and the
// host copies hide behind the kernel instead of adding to it.
constexpr size_t kOutRow = 1 + 64 + 64 + 32;  // verdict | beta_eta | beta_leader | eta_nonce
struct PipeSlot {
  hipStream_t st = nullptr;
  hipEvent_t done = nullptr;
  Buf in[28];
  uint8_t* h_out = nullptr;  // pinned: verdict (m) | beta_eta (64 m) | beta_leader (64 m) | eta_nonce (32 m)
  size_t h_cap = 0;
  StagedHdr staged;  // its rebased body offsets stay alive for the async upload
  size_t lo = 0, m = 0;
  bool busy = false;
};
struct Pipe {
  bool ready = false;
  PipeSlot s[2];
};

// ---- raw header CBOR from host memory (state; the engine is raw_pipe.cpp raw_run) ----
// A slot of the raw-CBOR pipeline: its stream, pinned NUMA-local staging for
// one chunk's gathered header bytes and for its results, and the chunk's
// device buffers (raw bytes, the slicer's arena, results).
constexpr int kRawMaxSlots = 8;
struct RawSlot {
  hipStream_t st = nullptr;
  hipEvent_t done = nullptr;
  uint8_t* h_in = nullptr;   // rebased offsets | lengths | eta0 | alphas | raw bytes
  size_t h_in_cap = 0;
  uint8_t* h_out = nullptr;  // status | verdict | beta_eta | beta_leader | eta_nonce
  size_t h_out_cap = 0;
  Buf d_in, d_arena, d_out;
  // the envelope of a validating call (RawCall env): the chunk's records, its
  // hashes | bits | first and last record, and their pinned copy
  Buf d_env;
  uint8_t* h_env = nullptr;
  size_t h_env_cap = 0;
  // the ledger-view checks of a call with RawCall ledger: bits | rows on the
  // device; bits | rows | the counter column in pinned memory
  Buf d_lv;
  uint8_t* h_lv = nullptr;
  size_t h_lv_cap = 0;
  // the Byron ledger-view checks of a call with RawCall pbft: bits | rows |
  // slots of the chunk's PBFT rows (and a mixed chunk's index list) on the
  // device; bits | rows | slots in pinned memory
  Buf d_pb;
  uint8_t* h_pb = nullptr;
  size_t h_pb_cap = 0;
  size_t lo = 0, m = 0;
  bool busy = false;
  // the combined entry (kRawChain): the chunk's era make-up and, for a mixed
  // chunk, its TPraos headers' indices (mt of them) followed by its PBFT
  // headers' -- the order the per-class offset / length lists are in
  int mode = 0;  // RawMode
  size_t mt = 0;
  std::vector<uint32_t> idx;
};
enum RawMode { kModeTpraos = 0, kModeByron = 1, kModeMixed = 2 };
struct RawPipe {
  bool ready = false;
  RawSlot s[kRawMaxSlots];
  Buf d_views;  // a call's packed ledger views (RawLedger), uploaded once per call
  hipEvent_t views_up = nullptr;
  Buf d_pviews;  // a call's packed delegation schedule (RawPbft), likewise
};

// Everything a calling thread needs on one device: its stream, the scratch
// slots of each stream it launches on, staging buffers and the two-slot
// pipeline.  Contexts are POOLED per device ("a per-thread
// or pooled stream"): a thread borrows one on its first call for a device and
// its thread-exit guard (Lease) hands it back, so the node's churning FFI
// worker threads reuse a few contexts instead of leaking one each.  A
// returned context has nothing in flight: host-buffer calls synchronise
// before returning, and device-API launches on a caller stream only use the
// scratch keyed by that stream (work later enqueued on the same stream is
// ordered after them).  Only the pool itself outlives the process (never
// freed: the HIP runtime may be gone at teardown).
// What a sharing workspace keeps from launch to launch (key_cache.h): the
// directory's buffer and the slots it is laid out for.  The rest is what the
// last header launch that was enqueued WHOLE left behind, and what the next
// one may rely on instead of clearing again: `valid` is taken down when a
// launch starts and put back only when all of it is enqueued, so a launch
// that returns an error half-way leaves a workspace the next launch empties.
// epoch: the knob epoch (a reload empties the directory); dir_gen / tab_gen /
// aux_gen: the allocations (Buf gen) of the directory, of the buffer the
// per-call grouping table lies in and of the VRF tables; tab_off / tab_cap:
// where in its buffer that table lay and its entries.  Allocations are told
// apart by their count, never by their address.
struct KeyDirWs {
  Buf dir;
  size_t slots = 0;
  bool valid = false;
  unsigned long long epoch = 0;
  unsigned long long dir_gen = 0, tab_gen = 0, aux_gen = 0;
  size_t tab_off = 0, tab_cap = 0;
};

// The OCERT sharing workspace of one stream (kernels.hip launch_hdr): per call
// the open-addressing table, rep[n], uniq[n] and ocert_ok[n] -- 4 (next power
// of two >= 2n) + 9n bytes, about 17 MB at 1M headers -- and, kept between
// calls, the certificate directory (kd: up to 65,536 certificates at 157 B
// each, 10 MB).  last: the device count of the stream's last header launch
// (null when that launch did not share), for ouro_debug_last_ocert_groups.
struct OcertWs {
  Buf buf;
  KeyDirWs kd;
  const uint32_t* last = nullptr;
};

// The VRF key sharing workspace of one stream (kernels.hip launch_hdr,
// vrfkey_ws.h): per call the grouping buffer (80 + 4 (next power of two >= 2n)
// + 12n bytes); kept between calls the tables of up to kd.slots keys (verify.h
// kYKeyBytes each, at most OURO_VRFKEY_TAB_MB in all) and their directory (kd,
// under 60 B per slot).  last / last_kmax: the device count of the stream's last
// header launch and the kmax it ran with (null when that launch did no
// grouping), for ouro_debug_last_vrfkey_groups.
struct VrfKeyWs {
  Buf group, tables;
  KeyDirWs kd;
  const uint32_t* last = nullptr;
  uint32_t last_kmax = 0;
};

struct ThreadCtx {
  hipStream_t stream = nullptr;
  std::map<hipStream_t, Buf> scratch;  // per stream: concurrent launches never share slots
  std::map<hipStream_t, OcertWs> ocert;  // per stream, grown like scratch
  std::map<hipStream_t, VrfKeyWs> vrfkey;  // per stream, grown like scratch
  Buf in[32];  // staging slots; a header batch uses up to 24
  Pipe pipe;
  RawPipe raw;  // ouro_tpraos_verify_cbor / ouro_integrity_verify_cbor
};

// the calling thread's context on device `dev`
ThreadCtx& ctx_of(int dev);
// ... on its current device (valid after current_device())
ThreadCtx& ctx();
int ensure(Buf& b, size_t bytes);
int thread_stream(hipStream_t* s);
// grid for n items of kernel `id`; returns the scratch slot count
int plan(DeviceState* ds, int id, size_t n, hipStream_t stream, int* grid, int32_t** scratch,
         int lane_words = ouro::kSlotWords);
// the last launch's error, if any (and the test build's injected one, hooks.h)
int launch_check();

// ---- the host path (host_path.h) -------------------------------------------
// A host-buffer batch whose device run fails with OURO_EDEVICE is recomputed
// on the host path (SURVEY.md §5, §8(b) "Errors": never a silent accept, and
// the caller still gets verdicts); OURO_ON_DEVICE_ERROR=fail returns the error
// instead.  Device-pointer calls (*_batch_device) cannot: their buffers are
// device memory, so they return the error.
extern std::atomic<unsigned long long> g_host_single, g_host_recompute;
bool recompute_on_error();
template <class F>
int or_host(int rc, F&& recompute) {
  if (rc != OURO_EDEVICE || !recompute_on_error()) return rc;
  g_host_recompute++;
  const std::string why = t_last_error;
  const int r = recompute();
  t_last_error = r == OURO_OK ? "recomputed on the host path after: " + why
                              : "host path failed (" + t_last_error + ") after: " + why;
  return r;
}

// ---- the knob accessors (knobs.h; documented at their definitions) ----
bool single_on_gpu();
size_t wide_small_max();
bool split_launch();
bool ocert_share();
uint32_t ocert_hash_mask();
bool vrfkey_share();
size_t vrfkey_tab_bytes();
bool key_cache();
unsigned long long knob_epoch();
int lat_block();
int lat_quad();
int lat_wide_mask();
int lat_fuse();
int lat_skip_mask();

// ---- host-buffer staging ----
struct Stager {
  hipStream_t st;
  int slot = 0;
  int rc = OURO_OK;
  Buf* bufs = ctx().in;  // device buffers, one per up()/out() call
  int nbufs = 32;
  Buf* next() {
    if (slot >= nbufs) {
      rc = fail(OURO_EDEVICE, "staging slots exhausted");
      return nullptr;
    }
    return &bufs[slot++];
  }
  template <class T>
  T* up(const T* host, size_t count) {
    if (rc) return nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    Buf* b = next();
    if (!b || (rc = ensure(*b, bytes))) return nullptr;
    if (count) {
      hipError_t e = hipMemcpyAsync(b->p, host, count * sizeof(T), hipMemcpyHostToDevice, st);
      if (e != hipSuccess) rc = fail(OURO_EDEVICE, std::string("H2D: ") + hipGetErrorString(e));
    }
    return static_cast<T*>(b->p);
  }
  template <class T>
  T* out(size_t count) {
    if (rc) return nullptr;
    Buf* b = next();
    if (!b || (rc = ensure(*b, std::max<size_t>(count * sizeof(T), 16)))) return nullptr;
    return static_cast<T*>(b->p);
  }
};

// Window of a batch (see struct Window); EINVAL when an offset + length
// overflows.
int window_of(size_t n, const uint64_t* off, const uint32_t* len, Window* w);
int finish(hipStream_t st);
int download(hipStream_t st, void* host, const void* dev, size_t bytes);
// The required members present?  (The alphas only when the batch has no slots.)
int check_hdr_batch(const ouro_tpraos_batch* b);
int stage_hdr(Stager& sg, const ouro_tpraos_batch* b, size_t lo, size_t m, StagedHdr* s);

// an ouro_epoch_nonces checked (OURO_EINVAL) and packed as the block the lane
// code reads (tpraos.h epoch_tab_*; api_batch.cpp)
int epoch_tab_build(const ouro_epoch_nonces* e, std::vector<uint64_t>* tab);

}  // namespace ouro_rt
#pragma GCC visibility pop
