// multi.cpp -- one process, several GPUs: the per-device worker pool and the
// *_multi entries (the raw-CBOR ones shard a raw_call.h RawCall over
// raw_pipe.cpp's raw_verify), the device count and NUMA entries.  Host code
// only.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ouro_verify.h"
#include "host_util.h"
#include "raw_call.h"

using namespace ouro_rt;

// ---- one process, several GPUs ----------------------------
// Persistent worker threads, pooled per device: a multi-device call borrows
// one worker per shard (a device listed k times gets k workers) and returns
// them when every shard is done, so two callers -- ChainSync windows and
// ChainDB's suffix re-validation, say -- run their calls at once on workers of
// their own instead of queueing behind one process-wide lock (VERDICT r05
// item 2).  A worker's thread-local context -- streams, device buffers,
// pinned staging, the raw-CBOR slots -- belongs to its one device and lives as
// long as the process, so repeated calls allocate nothing; the worker is
// bound to its GPU's NUMA node.  Each worker verifies one contiguous shard
// straight into the caller's buffers; in one process no collective is needed.
namespace {
struct Worker {
  std::mutex mu;
  std::condition_variable cv;
  bool has_job = false, done = false;
  int dev = 0, rc = OURO_OK;
  int numa_node = -1, bound_cpus = 0;
  std::string err;
  std::function<int()> job;

  void loop() {
    // this worker's host side -- its copies, its pinned staging (allocated
    // with hipHostMallocNumaUser), its gathers -- on the GPU's node
    numa_node = device_numa_node(dev);
    if (numa_node >= 0) bound_cpus = ouro_numa::bind_thread(numa_node);
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return has_job; });
      has_job = false;
      std::function<int()> f = std::move(job);
      lk.unlock();
      int r = ouro_set_device(dev);
      // nothing thrown in a shard (a host allocation, say) may end the
      // process from this detached thread: it fails the shard instead
      if (r == OURO_OK) {
        try {
          r = f();
        } catch (const std::bad_alloc&) {
          r = fail(OURO_EDEVICE, "out of host memory");
        } catch (...) {
          r = fail(OURO_EDEVICE, "shard failed with an exception");
        }
      }
      lk.lock();
      rc = r;
      err = r ? t_last_error : std::string();
      done = true;
      cv.notify_all();
    }
  }
};

struct WorkerPool {
  std::mutex mu;
  std::map<int, std::vector<Worker*>> idle;  // per device
  std::vector<Worker*> all;                   // never freed: threads outlive every call
};
WorkerPool& worker_pool() {
  static WorkerPool* p = new WorkerPool;
  return *p;
}

// an idle worker of `dev`, or a new one; nullptr if no thread could be
// started (no exception ever crosses the C ABI)
Worker* borrow_worker(int dev) {
  WorkerPool& P = worker_pool();
  std::lock_guard<std::mutex> g(P.mu);
  std::vector<Worker*>& v = P.idle[dev];
  if (!v.empty()) {
    Worker* w = v.back();
    v.pop_back();
    return w;
  }
  Worker* w = new (std::nothrow) Worker;
  if (!w) return nullptr;
  w->dev = dev;
  try {
    P.all.reserve(P.all.size() + 1);
    std::thread([w] { w->loop(); }).detach();
  } catch (...) {
    delete w;
    return nullptr;
  }
  P.all.push_back(w);
  return w;
}

void return_worker(Worker* w) {
  WorkerPool& P = worker_pool();
  std::lock_guard<std::mutex> g(P.mu);
  P.idle[w->dev].push_back(w);
}

// the device list of a multi-device call (NULL: every visible device)
int multi_devices(const int* devices, int ndev, std::vector<int>* devs) {
  const int count = ouro_device_count();
  if (devices) {
    if (ndev <= 0 || ndev > 64) return fail(OURO_EINVAL, "bad device count");
    devs->assign(devices, devices + ndev);
    for (int d : *devs)
      if (d < 0 || d >= count) return fail(OURO_ENODEV, "no such device " + std::to_string(d));
  } else {
    for (int d = 0; d < count; d++) devs->push_back(d);
    if (devs->empty()) return fail(OURO_ENODEV, "no device");
  }
  return OURO_OK;
}

// n items in contiguous shards of ceil(n / G) over the listed devices, shard
// k = job(k's first item, its count) on a borrowed worker of devices[k]; the
// first failing shard's code (its message prefixed with the device)
template <class Job>
int run_multi(const std::vector<int>& devs, size_t n, Job&& job) {
  const size_t g = std::min<size_t>(devs.size(), n);
  const size_t per = (n + g - 1) / g;
  // every shard's worker first, so a worker that cannot be started fails the
  // call before any shard runs
  std::vector<Worker*> used;
  for (size_t k = 0; k < g && k * per < n; k++) {
    Worker* w = borrow_worker(devs[k]);
    if (!w) {
      for (Worker* u : used) return_worker(u);
      return fail(OURO_EDEVICE, "cannot start a worker thread for device " +
                                    std::to_string(devs[k]));
    }
    used.push_back(w);
  }
  for (size_t k = 0; k < used.size(); k++) {
    const size_t lo = k * per;
    const size_t m = std::min(per, n - lo);
    Worker* w = used[k];
    {
      std::lock_guard<std::mutex> lk(w->mu);
      w->job = [&job, lo, m] { return job(lo, m); };
      w->done = false;
      w->has_job = true;
    }
    w->cv.notify_all();
  }
  int rc = OURO_OK;
  for (Worker* w : used) {  // wait for every shard, errors included
    {
      std::unique_lock<std::mutex> lk(w->mu);
      w->cv.wait(lk, [&] { return w->done; });
      if (w->rc && rc == OURO_OK) {
        rc = w->rc;
        t_last_error = "device " + std::to_string(w->dev) + ": " + w->err;
      }
    }
    return_worker(w);
  }
  return rc;
}

ouro_tpraos_batch shard_of(const ouro_tpraos_batch& b, size_t lo, size_t m) {
  ouro_tpraos_batch s = b;  // body + absolute offsets shared, epoch_nonce shared
  s.n = m;
  s.issuer_vk = b.issuer_vk + 32 * lo;
  s.vrf_vk = b.vrf_vk + 32 * lo;
  s.eta_proof = b.eta_proof + 80 * lo;
  s.leader_proof = b.leader_proof + 80 * lo;
  if (b.eta_alpha) s.eta_alpha = b.eta_alpha + 32 * lo;
  if (b.leader_alpha) s.leader_alpha = b.leader_alpha + 32 * lo;
  s.hot_vk = b.hot_vk + 32 * lo;
  s.ocert_counter = b.ocert_counter + lo;
  s.ocert_kes_period = b.ocert_kes_period + lo;
  s.ocert_sigma = b.ocert_sigma + 64 * lo;
  s.kes_t = b.kes_t + lo;
  s.kes_sig = b.kes_sig + 448 * lo;
  s.body_off = b.body_off + lo;
  s.body_len = b.body_len + lo;
  if (b.eta_output) s.eta_output = b.eta_output + 64 * lo;
  if (b.leader_output) s.leader_output = b.leader_output + 64 * lo;
  if (b.slot) s.slot = b.slot + lo;
  if (b.eta_nonce) s.eta_nonce = b.eta_nonce + 32 * lo;
  return s;
}

// shard [lo, lo + m) of a raw-CBOR call: the buffer and its offsets are
// shared (the offsets are absolute into raw), every per-header array offset
RawCall raw_shard(const RawCall& c, size_t lo, size_t m) {
  RawCall s = c;
  s.n = m;
  s.off = c.off + lo;
  s.len = c.len + lo;
  if (c.ea) s.ea = c.ea + 32 * lo;
  if (c.la) s.la = c.la + 32 * lo;
  s.status = c.status + lo;
  s.verdict = c.verdict + lo;
  if (c.be) s.be = c.be + 64 * lo;
  if (c.bl) s.bl = c.bl + 64 * lo;
  if (c.nonce) s.nonce = c.nonce + 32 * lo;
  if (c.proto) s.proto = c.proto + lo;  // (the epoch schedule is shared)
  return s;
}

// a raw-CBOR call over several devices: its argument checks once, then each
// shard through the one-device pipeline (raw_verify: chunks over the worker's
// slots, the host-path recompute of that shard after a device error)
int raw_verify_multi(const RawCall& c, const int* devices, int ndev) {
  if (c.n == 0) return OURO_OK;
  if (int rc0 = raw_check(c)) return rc0;
  // every span inside raw before any shard starts: the shards do not look again
  if (int rc = spans_check("header", "raw_bytes", c.raw_bytes, c.off, c.len, c.n)) return rc;
  std::vector<int> devs;
  int rc = multi_devices(devices, ndev, &devs);
  if (rc) return rc;
  RawCall checked = c;
  checked.spans_checked = true;
  return run_multi(devs, c.n, [&](size_t lo, size_t m) {
    return raw_verify(raw_shard(checked, lo, m));
  });
}
}  // namespace

extern "C" {

int ouro_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

int ouro_device_numa_node(int device) {
  const int count = ouro_device_count();
  if (device < 0 || device >= count) return fail(OURO_ENODEV, "no such device");
  return device_numa_node(device);
}

int ouro_bind_thread_to_device(int device) {
  const int node = ouro_device_numa_node(device);
  if (node >= 0) ouro_numa::bind_thread(node);
  return node;
}

int ouro_debug_multi_workers(int* devices, int* nodes, int* cpus, int max) {
  WorkerPool& P = worker_pool();
  std::lock_guard<std::mutex> guard(P.mu);
  int k = 0;
  for (Worker* w : P.all) {
    if (k < max) {
      if (devices) devices[k] = w->dev;
      if (nodes) nodes[k] = w->numa_node;
      if (cpus) cpus[k] = w->bound_cpus;
    }
    k++;
  }
  return k;
}

int ouro_tpraos_verify_batch_multi(const ouro_tpraos_batch* b, const int* devices, int ndev,
                                   uint8_t* verdict, uint8_t* beta_eta, uint8_t* beta_leader) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  if (b->n == 0) return OURO_OK;
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  std::vector<int> devs;
  if ((rc = multi_devices(devices, ndev, &devs))) return rc;
  return run_multi(devs, b->n, [&](size_t lo, size_t m) {
    const ouro_tpraos_batch s = shard_of(*b, lo, m);
    return ouro_tpraos_verify_batch(&s, verdict + lo, beta_eta ? beta_eta + 64 * lo : nullptr,
                                    beta_leader ? beta_leader + 64 * lo : nullptr);
  });
}

// The raw-CBOR entries over several devices of one process (SURVEY.md §8(e):
// static contiguous shards, one per listed device, each on that device's
// NUMA-bound worker with its own chunk pipeline and pinned staging; results
// straight into the caller's buffers).
int ouro_tpraos_verify_cbor_multi(const int* devices, int ndev, const uint8_t* raw,
                                  size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                                  size_t n, uint64_t slots_per_kes_period,
                                  const uint8_t* epoch_nonce, const uint8_t* eta_alpha,
                                  const uint8_t* leader_alpha, uint8_t* status, uint8_t* verdict,
                                  uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce) {
  if (n && slots_per_kes_period == 0) return fail(OURO_EINVAL, "zero slots per KES period");
  if ((eta_alpha == nullptr) != (leader_alpha == nullptr))
    return fail(OURO_EINVAL, "give both VRF input arrays or neither");
  RawCall c = RawCall::of(kRawHdr, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = slots_per_kes_period;
  c.eta0 = epoch_nonce;
  c.ea = eta_alpha;
  c.la = leader_alpha;
  c.be = beta_eta;
  c.bl = beta_leader;
  c.nonce = eta_nonce;
  return raw_verify_multi(c, devices, ndev);
}

int ouro_integrity_verify_cbor_multi(const int* devices, int ndev, const uint8_t* raw,
                                     size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                                     size_t n, uint64_t slots_per_kes_period, uint8_t* status,
                                     uint8_t* verdict) {
  if (n && slots_per_kes_period == 0) return fail(OURO_EINVAL, "zero slots per KES period");
  RawCall c = RawCall::of(kRawKes, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = slots_per_kes_period;
  return raw_verify_multi(c, devices, ndev);
}

// The combined entry (chain_api.cpp ouro_chain_verify_cbor) sharded like the
// others: each shard classifies and verifies its own headers; the epoch
// schedule is validated and packed once and shared by every shard.
int ouro_chain_verify_cbor_multi(const int* devices, int ndev, const uint8_t* raw,
                                 size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                                 size_t n, uint64_t slots_per_kes_period, int64_t protocol_magic,
                                 const ouro_epoch_nonces* epochs, const uint8_t* eta_alpha,
                                 const uint8_t* leader_alpha, uint8_t* proto, uint8_t* status,
                                 uint8_t* verdict, uint8_t* beta_eta, uint8_t* beta_leader,
                                 uint8_t* eta_nonce) {
  RawCall c = RawCall::of(kRawChain, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = slots_per_kes_period;
  c.ea = eta_alpha;
  c.la = leader_alpha;
  c.be = beta_eta;
  c.bl = beta_leader;
  c.nonce = eta_nonce;
  c.magic = protocol_magic;
  c.proto = proto;
  if (n == 0) return OURO_OK;
  std::vector<uint64_t> tab;
  if (epochs) {
    if (int rc = epoch_tab_build(epochs, &tab)) return rc;
    c.epochs = reinterpret_cast<const uint8_t*>(tab.data());
    c.epochs_bytes = 8 * tab.size();
  }
  return raw_verify_multi(c, devices, ndev);
}

int ouro_byron_verify_cbor_multi(const int* devices, int ndev, const uint8_t* raw,
                                 size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                                 size_t n, int64_t protocol_magic, uint8_t* status,
                                 uint8_t* verdict) {
  if (protocol_magic < -1 || protocol_magic > (int64_t)0xffffffffll)
    return fail(OURO_EINVAL, "protocol magic outside Word32 (or -1)");
  RawCall c = RawCall::of(kRawByron, raw, raw_bytes, off, len, n, status, verdict);
  c.magic = protocol_magic;
  return raw_verify_multi(c, devices, ndev);
}

}  // extern "C"
