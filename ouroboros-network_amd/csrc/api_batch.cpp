// api_batch.cpp -- the batch entries of the C ABI (include/ouro_verify.h):
// host-buffer batches and the two-slot header pipeline, single items, the
// nonce fold, the leader check, the device-pointer (*_batch_device) and
// explicit host-path (*_batch_host) entries.  Host code only: kernels are
// reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "host_path.h"
#include "host_util.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"
#include "tpraos.h"

using namespace ouro;
using namespace ouro_rt;

namespace ouro_rt {
// ouro_epoch_nonces (include/ouro_verify.h) checked and packed as the block
// the lane code reads (tpraos.h epoch_tab_*), 8-byte words for its alignment
int epoch_tab_build(const ouro_epoch_nonces* e, std::vector<uint64_t>* tab) {
  if (!e) return fail(OURO_EINVAL, "null epoch schedule");
  if (e->k < 1 || e->k > OURO_EPOCHS_MAX)
    return fail(OURO_EINVAL, "epoch schedule: k outside 1 .. OURO_EPOCHS_MAX");
  if (!e->first_slot || !e->nonce) return fail(OURO_EINVAL, "epoch schedule: null first_slot or nonce");
  if (e->first_slot[0] != 0) return fail(OURO_EINVAL, "epoch schedule: first_slot[0] must be 0");
  for (size_t j = 1; j < e->k; j++)
    if (e->first_slot[j] <= e->first_slot[j - 1])
      return fail(OURO_EINVAL, "epoch schedule: first_slot not strictly increasing at entry " +
                                   std::to_string(j));
  const size_t k = e->k;
  tab->assign(epoch_tab_bytes(k) / 8, 0);
  uint8_t* t = reinterpret_cast<uint8_t*>(tab->data());
  const uint32_t k32 = (uint32_t)k;
  memcpy(t, &k32, 4);
  memcpy(t + 16, e->first_slot, 8 * k);
  memcpy(t + epoch_tab_nonce_off(k), e->nonce, 32 * k);
  if (e->neutral)
    for (size_t j = 0; j < k; j++) t[epoch_tab_neutral_off(k) + j] = e->neutral[j] ? 1 : 0;
  return OURO_OK;
}
}  // namespace ouro_rt

namespace {
int ed_batch_host(size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                  const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* verdict,
                  uint32_t byron) {
  if (n == 0) return OURO_OK;
  if (!pk || !sig || !msg_off || !msg_len || !verdict) return fail(OURO_EINVAL, "null argument");
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, msg_off, msg_len, &w))) return rc;
  if (w.span() && !msg) return fail(OURO_EINVAL, "null message buffer");
  Stager sg{st};
  auto dpk = sg.up(pk, 32 * n);
  auto dsig = sg.up(sig, 64 * n);
  auto dmsg = sg.up(w.span() ? msg + w.lo : msg, w.span());
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(msg_len, n);
  auto dver = sg.out<uint8_t>(n);
  if (sg.rc) return sg.rc;
  if ((rc = launch_ed(st, n, dpk, dsig, dmsg, doff, dlen, dver, byron))) return rc;
  std::vector<uint8_t> tmp(n);
  if ((rc = download(st, tmp.data(), dver, n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(verdict, tmp.data(), n);
  return OURO_OK;
}
}  // namespace

extern "C" {

int ouro_ed25519_verify_batch(size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                              const uint64_t* msg_off, const uint32_t* msg_len, uint8_t* verdict) {
  return or_host(ed_batch_host(n, pk, sig, msg, msg_off, msg_len, verdict, 0), [&] {
    return ouro_host::ed_batch(n, pk, sig, msg, msg_off, msg_len, verdict, 0);
  });
}

int ouro_byron_ed25519_verify_batch(size_t n, const uint8_t* pk, const uint8_t* sig,
                                    const uint8_t* msg, const uint64_t* msg_off,
                                    const uint32_t* msg_len, uint8_t* verdict) {
  return or_host(ed_batch_host(n, pk, sig, msg, msg_off, msg_len, verdict, 1), [&] {
    return ouro_host::ed_batch(n, pk, sig, msg, msg_off, msg_len, verdict, 1);
  });
}


int ouro_vrf03_verify_batch(size_t n, const uint8_t* pk, const uint8_t* proof, const uint8_t* alpha,
                            const uint64_t* alpha_off, const uint32_t* alpha_len, uint8_t* beta,
                            uint8_t* verdict) {
  return ouro_vrf03_verify_batch_flags(n, pk, proof, alpha, alpha_off, alpha_len, beta, verdict, 0);
}

}  // extern "C"

namespace {
int vrf_batch_dev(size_t n, const uint8_t* pk, const uint8_t* proof, const uint8_t* alpha,
                  const uint64_t* alpha_off, const uint32_t* alpha_len, uint8_t* beta,
                  uint8_t* verdict, uint32_t flags) {
  if (n == 0) return OURO_OK;
  if (flags & ~OURO_VRF_STRICT_S) return fail(OURO_EINVAL, "unknown VRF flags");
  if (!pk || !proof || !alpha_off || !alpha_len || !verdict) return fail(OURO_EINVAL, "null argument");
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, alpha_off, alpha_len, &w))) return rc;
  if (w.span() && !alpha) return fail(OURO_EINVAL, "null alpha buffer");
  Stager sg{st};
  auto dpk = sg.up(pk, 32 * n);
  auto dpi = sg.up(proof, 80 * n);
  auto dal = sg.up(w.span() ? alpha + w.lo : alpha, w.span());
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(alpha_len, n);
  auto dbeta = sg.out<uint8_t>(64 * n);
  auto dver = sg.out<uint8_t>(n);
  if (sg.rc) return sg.rc;
  if ((rc = launch_vrf(st, n, dpk, dpi, dal, doff, dlen, dbeta, dver, flags))) return rc;
  std::vector<uint8_t> tv(n), tb(beta ? 64 * n : 0);
  if ((rc = download(st, tv.data(), dver, n))) return rc;
  if (beta && (rc = download(st, tb.data(), dbeta, 64 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(verdict, tv.data(), n);
  if (beta) memcpy(beta, tb.data(), 64 * n);
  return OURO_OK;
}

int kes_batch_dev(size_t n, const uint8_t* vk, const uint32_t* t, const uint8_t* msg,
                  const uint64_t* msg_off, const uint32_t* msg_len, const uint8_t* sig,
                  uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!vk || !t || !msg_off || !msg_len || !sig || !verdict) return fail(OURO_EINVAL, "null argument");
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, msg_off, msg_len, &w))) return rc;
  if (w.span() && !msg) return fail(OURO_EINVAL, "null message buffer");
  Stager sg{st};
  auto dvk = sg.up(vk, 32 * n);
  auto dt = sg.up(t, n);
  auto dmsg = sg.up(w.span() ? msg + w.lo : msg, w.span());
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(msg_len, n);
  auto dsig = sg.up(sig, 448 * n);
  auto dver = sg.out<uint8_t>(n);
  if (sg.rc) return sg.rc;
  if ((rc = launch_kes(st, n, dvk, dt, dmsg, doff, dlen, dsig, dver))) return rc;
  std::vector<uint8_t> tv(n);
  if ((rc = download(st, tv.data(), dver, n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(verdict, tv.data(), n);
  return OURO_OK;
}
}  // namespace

extern "C" {

int ouro_vrf03_verify_batch_flags(size_t n, const uint8_t* pk, const uint8_t* proof,
                                  const uint8_t* alpha, const uint64_t* alpha_off,
                                  const uint32_t* alpha_len, uint8_t* beta, uint8_t* verdict,
                                  uint32_t flags) {
  return or_host(vrf_batch_dev(n, pk, proof, alpha, alpha_off, alpha_len, beta, verdict, flags),
                 [&] {
                   return ouro_host::vrf_batch(n, pk, proof, alpha, alpha_off, alpha_len, beta,
                                               verdict, flags);
                 });
}

int ouro_sum6kes_verify_batch(size_t n, const uint8_t* vk, const uint32_t* t, const uint8_t* msg,
                              const uint64_t* msg_off, const uint32_t* msg_len, const uint8_t* sig,
                              uint8_t* verdict) {
  return or_host(kes_batch_dev(n, vk, t, msg, msg_off, msg_len, sig, verdict), [&] {
    return ouro_host::kes_batch(n, vk, t, msg, msg_off, msg_len, sig, verdict);
  });
}

}  // extern "C"

namespace {
// ---- pipelined host-buffer header batches (PipeSlot / Pipe above) ----
int pipe_of(int dev, Pipe** out) {
  Pipe& p = ctx_of(dev).pipe;
  if (!p.ready) {
    for (PipeSlot& q : p.s) {
      if (!q.st) OURO_HIP(hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking));
      if (!q.done) OURO_HIP(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
    }
    p.ready = true;
  }
  *out = &p;
  return OURO_OK;
}

struct HdrOut {
  uint8_t *verdict, *beta_eta, *beta_leader, *eta_nonce;
};

// the argument checks of the two epochs entries; the schedule packed into *tab
int check_epochs_batch(const ouro_tpraos_batch* b, const ouro_epoch_nonces* e,
                       const uint8_t* verdict, std::vector<uint64_t>* tab) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  int rc = epoch_tab_build(e, tab);
  if (rc || b->n == 0) return rc;
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  if (!b->slot) return fail(OURO_EINVAL, "an epoch schedule needs the headers' slots (slot is null)");
  if (b->epoch_nonce)
    return fail(OURO_EINVAL, "epoch_nonce must be null beside an epoch schedule");
  if (b->eta_alpha || b->leader_alpha)
    return fail(OURO_EINVAL, "eta_alpha / leader_alpha must be null beside an epoch schedule");
  return check_hdr_batch(b);
}

int pipe_drain(PipeSlot& p, const HdrOut& o) {
  if (!p.busy) return OURO_OK;
  p.busy = false;
  OURO_HIP(hipEventSynchronize(p.done));
  const size_t m = p.m;
  memcpy(o.verdict + p.lo, p.h_out, m);
  if (o.beta_eta) memcpy(o.beta_eta + 64 * p.lo, p.h_out + m, 64 * m);
  if (o.beta_leader) memcpy(o.beta_leader + 64 * p.lo, p.h_out + 65 * m, 64 * m);
  if (o.eta_nonce) memcpy(o.eta_nonce + 32 * p.lo, p.h_out + 129 * m, 32 * m);
  return OURO_OK;
}

// (tab: the call's epoch-nonce schedule block, or null; uploaded with every
// chunk on the chunk's own stream -- at most ~170 KB beside ~100 MB of rows)
int pipe_chunk(PipeSlot& p, const ouro_tpraos_batch* b, size_t lo, size_t m, const HdrOut& o,
               const std::vector<uint64_t>* tab) {
  Stager sg{p.st};
  sg.bufs = p.in;
  sg.nbufs = (int)(sizeof(p.in) / sizeof(p.in[0]));
  int rc = stage_hdr(sg, b, lo, m, &p.staged);
  if (rc) return rc;
  const uint64_t* dtab = tab ? sg.up(tab->data(), tab->size()) : nullptr;
  if (sg.rc) return sg.rc;
  const StagedHdr& s = p.staged;
  if ((rc = launch_hdr(p.st, s.d, s.ver, s.be, s.bl, reinterpret_cast<const uint8_t*>(dtab))))
    return rc;
  if (p.h_cap < kOutRow * m) {
    if (p.h_out) OURO_HIP(hipHostFree(p.h_out));
    p.h_out = nullptr;
    p.h_cap = 0;
    // (hipHostMallocNumaUser: on the calling thread's NUMA policy -- a
    // multi-device worker is bound to its GPU's node, numa.cpp)
    OURO_HIP(hipHostMalloc(reinterpret_cast<void**>(&p.h_out), kOutRow * m, hipHostMallocNumaUser));
    p.h_cap = kOutRow * m;
  }
  OURO_HIP(hipMemcpyAsync(p.h_out, s.ver, m, hipMemcpyDeviceToHost, p.st));
  if (o.beta_eta) OURO_HIP(hipMemcpyAsync(p.h_out + m, s.be, 64 * m, hipMemcpyDeviceToHost, p.st));
  if (o.beta_leader)
    OURO_HIP(hipMemcpyAsync(p.h_out + 65 * m, s.bl, 64 * m, hipMemcpyDeviceToHost, p.st));
  if (o.eta_nonce)
    OURO_HIP(hipMemcpyAsync(p.h_out + 129 * m, s.nonce, 32 * m, hipMemcpyDeviceToHost, p.st));
  OURO_HIP(hipEventRecord(p.done, p.st));
  p.lo = lo;
  p.m = m;
  p.busy = true;
  return OURO_OK;
}

// headers per chunk: one full grid of the header kernel (OURO_HOST_CHUNK
// overrides; 0 = the whole batch in one piece)
size_t host_chunk(DeviceState* ds) {
  const long long v = ouro_knobs::get().host_chunk.load(std::memory_order_relaxed);
  return v >= 0 ? (size_t)v : (size_t)ds->max_blocks[kHdr] * kBlock;
}

int hdr_batch_pipelined(const ouro_tpraos_batch* b, size_t chunk, const HdrOut& o,
                        const std::vector<uint64_t>* tab) {
  int dev, rc = current_device(&dev);
  if (rc) return rc;
  Pipe* pp;
  if ((rc = pipe_of(dev, &pp))) return rc;
  size_t c = 0;
  for (size_t lo = 0; lo < b->n && !rc; lo += chunk, c++) {
    PipeSlot& p = pp->s[c & 1];
    rc = pipe_drain(p, o);
    if (!rc) rc = pipe_chunk(p, b, lo, std::min(chunk, b->n - lo), o, tab);
  }
  // older chunk first; on an error, still wait for everything in flight
  for (int k = 0; k < 2; k++) {
    PipeSlot& p = pp->s[(c + k) & 1];
    if (rc) {
      (void)hipStreamSynchronize(p.st);
      p.busy = false;
    } else {
      rc = pipe_drain(p, o);
    }
  }
  return rc;
}

// one synchronous launch of the whole batch (throughput kernel, or the
// latency-mode kernels with lowlat), results copied out after the sync
int hdr_batch_once(const ouro_tpraos_batch* b, const HdrOut& o, bool lowlat,
                   const std::vector<uint64_t>* tab = nullptr) {
  const size_t n = b->n;
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  DeviceState* ds;
  if ((rc = device_state(&ds))) return rc;
  Stager sg{st};
  StagedHdr s;
  if ((rc = stage_hdr(sg, b, 0, n, &s))) return rc;
  const uint64_t* dtab = tab ? sg.up(tab->data(), tab->size()) : nullptr;
  if (sg.rc) return sg.rc;
  if (lowlat) {
    // {n, option bits, generation (arrive_last; res is zeroed below), 0}
    const uint32_t nw[4] = {(uint32_t)n, batch_opts(s.d), 1u, 0u};
    const uint32_t* d_n = sg.up(nw, 4);
    int32_t* res = sg.out<int32_t>(slot_region_words(n, kLatResWords));
    int32_t* scr = sg.out<int32_t>(lowlat_scratch_words(ds, n));
    if (sg.rc) return sg.rc;
    // the arrival records are generation-tagged (generation 1 here) and never
    // reset by the kernel: this one-shot buffer starts from zero
    OURO_HIP(hipMemsetAsync(res, 0, sizeof(int32_t) * slot_region_words(n, kLatResWords), st));
    // (nw is read by the H2D above; this frame outlives the sync below)
    if ((rc = launch_lowlat(st, s.d, d_n, n, res, scr, s.ver, s.be, s.bl))) return rc;
  } else if ((rc = launch_hdr(st, s.d, s.ver, s.be, s.bl,
                              reinterpret_cast<const uint8_t*>(dtab)))) {
    return rc;
  }
  std::vector<uint8_t> tv(n), te(o.beta_eta ? 64 * n : 0), tl(o.beta_leader ? 64 * n : 0),
      tn(o.eta_nonce ? 32 * n : 0);
  if ((rc = download(st, tv.data(), s.ver, n))) return rc;
  if (o.beta_eta && (rc = download(st, te.data(), s.be, 64 * n))) return rc;
  if (o.beta_leader && (rc = download(st, tl.data(), s.bl, 64 * n))) return rc;
  if (o.eta_nonce && (rc = download(st, tn.data(), s.nonce, 32 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(o.verdict, tv.data(), n);
  if (o.beta_eta) memcpy(o.beta_eta, te.data(), 64 * n);
  if (o.beta_leader) memcpy(o.beta_leader, tl.data(), 64 * n);
  if (o.eta_nonce) memcpy(o.eta_nonce, tn.data(), 32 * n);
  return OURO_OK;
}
}  // namespace

extern "C" {

int ouro_tpraos_verify_batch(const ouro_tpraos_batch* b, uint8_t* verdict, uint8_t* beta_eta,
                             uint8_t* beta_leader) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  if (b->n == 0) return OURO_OK;
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  DeviceState* ds;
  if ((rc = device_state(&ds))) return rc;
  const HdrOut o{verdict, beta_eta, beta_leader, b->eta_nonce};
  const size_t chunk = host_chunk(ds);
  rc = chunk && b->n > chunk ? hdr_batch_pipelined(b, chunk, o, nullptr)
                             : hdr_batch_once(b, o, false);
  return or_host(rc, [&] { return ouro_host::hdr_batch(b, verdict, beta_eta, beta_leader); });
}

// The same under an epoch-nonce schedule: mkSeed's eta0 looked up per header
// by its slot (tpraos.h hdr_mkseed, kOptEpochs), so one call verifies a batch
// that crosses epoch boundaries.  Every argument check runs before anything
// else does.
int ouro_tpraos_verify_batch_epochs(const ouro_tpraos_batch* b, const ouro_epoch_nonces* e,
                                    uint8_t* verdict, uint8_t* beta_eta, uint8_t* beta_leader) {
  std::vector<uint64_t> tab;
  int rc = check_epochs_batch(b, e, verdict, &tab);
  if (rc || b->n == 0) return rc;
  DeviceState* ds;
  if ((rc = device_state(&ds))) return rc;
  const HdrOut o{verdict, beta_eta, beta_leader, b->eta_nonce};
  const size_t chunk = host_chunk(ds);
  rc = chunk && b->n > chunk ? hdr_batch_pipelined(b, chunk, o, &tab)
                             : hdr_batch_once(b, o, false, &tab);
  return or_host(rc, [&] {
    return ouro_host::hdr_batch(b, verdict, beta_eta, beta_leader,
                                reinterpret_cast<const uint8_t*>(tab.data()));
  });
}

// ---- latency mode (ChainSync windows) ----
int ouro_tpraos_verify_batch_lowlat(const ouro_tpraos_batch* b, uint8_t* verdict,
                                    uint8_t* beta_eta, uint8_t* beta_leader) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  if (b->n == 0) return OURO_OK;
  if (b->n > 0xffffffffu) return fail(OURO_EINVAL, "batch too large");
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  return or_host(hdr_batch_once(b, HdrOut{verdict, beta_eta, beta_leader, b->eta_nonce}, true),
                 [&] { return ouro_host::hdr_batch(b, verdict, beta_eta, beta_leader); });
}

int ouro_nonce_fold(size_t n, const uint8_t* eta_nonce, const uint64_t* slot,
                    uint64_t first_slot_next_epoch, uint64_t stability_window, uint8_t* eta_v,
                    uint8_t* eta_c, int* is_neutral) {
  if (n == 0) return OURO_OK;
  if (!eta_nonce || !slot || !eta_v || !eta_c) return fail(OURO_EINVAL, "null argument");
  bool v_neutral = is_neutral && is_neutral[0], c_neutral = is_neutral && is_neutral[1];
  uint32_t v[8], c[8];
  memcpy(v, eta_v, 32);
  memcpy(c, eta_c, 32);
  for (size_t i = 0; i < n; i++) {
    // eta_v <- eta_v (*) eta, with NeutralNonce (*) x = x
    uint32_t in[16];
    memcpy(in + 8, eta_nonce + 32 * i, 32);
    if (v_neutral) {
      memcpy(v, in + 8, 32);
    } else {
      memcpy(in, v, 32);
      blake2b256_64(v, in);
    }
    v_neutral = false;
    // UPDN: s +* Duration sp < firstSlotNextEpoch (Word64 arithmetic, as SlotNo)
    if (slot[i] + stability_window < first_slot_next_epoch) {
      memcpy(c, v, 32);
      c_neutral = false;
    }
  }
  memcpy(eta_v, v, 32);
  memcpy(eta_c, c, 32);
  if (is_neutral) {
    is_neutral[0] = v_neutral;
    is_neutral[1] = c_neutral;
  }
  return OURO_OK;
}

int ouro_leader_check_batch(size_t n, const uint8_t* beta, const uint64_t* sigma_num,
                            const uint64_t* sigma_den, int64_t act_log_hi, uint64_t act_log_lo,
                            int f_is_one, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!beta || !sigma_num || !sigma_den || !verdict) return fail(OURO_EINVAL, "null argument");
  auto dev = [&]() -> int {
    hipStream_t st;
    int rc = thread_stream(&st);
    if (rc) return rc;
    Stager sg{st};
    auto dbeta = sg.up(beta, 64 * n);
    auto dnum = sg.up(sigma_num, n);
    auto dden = sg.up(sigma_den, n);
    auto dver = sg.out<uint8_t>(n);
    if (sg.rc) return sg.rc;
    if ((rc = launch_leader(st, n, dbeta, dnum, dden, act_log_hi, act_log_lo, f_is_one, dver)))
      return rc;
    std::vector<uint8_t> tv(n);
    if ((rc = download(st, tv.data(), dver, n))) return rc;
    if ((rc = finish(st))) return rc;
    memcpy(verdict, tv.data(), n);
    return OURO_OK;
  };
  return or_host(dev(), [&] {
    return ouro_host::leader_batch(n, beta, sigma_num, sigma_den, act_log_hi, act_log_lo, f_is_one,
                                   verdict);
  });
}

// ---- single item: a batch of one (ABI-identical to the symbols replaced) ----
int ouro_ed25519_verify(const unsigned char* sig, const unsigned char* m, unsigned long long mlen,
                        const unsigned char* pk) {
  if (!sig || !pk || (mlen && !m)) return OURO_INVALID;
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)mlen;
  if ((unsigned long long)len != mlen) return fail(OURO_EINVAL, "message too long");
  uint8_t v = 0;
  static const uint8_t empty[1] = {0};
  int rc;
  if (single_on_gpu()) {
    rc = ouro_ed25519_verify_batch(1, pk, sig, mlen ? m : empty, &off, &len, &v);
  } else {
    g_host_single++;
    rc = ouro_host::ed_batch(1, pk, sig, mlen ? m : empty, &off, &len, &v, 0);
  }
  if (rc) return rc;
  return v ? OURO_OK : OURO_INVALID;
}

int ouro_byron_ed25519_verify(const unsigned char* m, size_t mlen, const unsigned char* pk,
                              const unsigned char* sig) {
  if (!sig || !pk || (mlen && !m)) return OURO_INVALID;
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)mlen;
  if ((size_t)len != mlen) return fail(OURO_EINVAL, "message too long");
  uint8_t v = 0;
  static const uint8_t empty[1] = {0};
  int rc;
  if (single_on_gpu()) {
    rc = ouro_byron_ed25519_verify_batch(1, pk, sig, mlen ? m : empty, &off, &len, &v);
  } else {
    g_host_single++;
    rc = ouro_host::ed_batch(1, pk, sig, mlen ? m : empty, &off, &len, &v, 1);
  }
  if (rc) return rc;
  return v ? OURO_OK : OURO_INVALID;
}

int ouro_vrf03_verify(unsigned char* output, const unsigned char* pk, const unsigned char* proof,
                      const unsigned char* msg, unsigned long long msglen) {
  if (!pk || !proof || (msglen && !msg)) return OURO_INVALID;
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)msglen;
  if ((unsigned long long)len != msglen) return fail(OURO_EINVAL, "message too long");
  uint8_t v = 0, beta[64];
  static const uint8_t empty[1] = {0};
  int rc;
  if (single_on_gpu()) {
    rc = ouro_vrf03_verify_batch(1, pk, proof, msglen ? msg : empty, &off, &len, beta, &v);
  } else {
    g_host_single++;
    rc = ouro_host::vrf_batch(1, pk, proof, msglen ? msg : empty, &off, &len, beta, &v, 0);
  }
  if (rc) return rc;
  if (!v) return OURO_INVALID;
  if (output) memcpy(output, beta, 64);  // written only on success, like the original
  return OURO_OK;
}

int ouro_vrf03_proof_to_hash(unsigned char* output, const unsigned char* proof) {
  if (!output || !proof) return OURO_INVALID;
  if (!single_on_gpu()) {
    g_host_single++;
    return ouro_host::proof_to_hash(output, proof);
  }
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  DeviceState* ds;
  if ((rc = device_state(&ds))) return rc;
  Stager sg{st};
  auto dpi = sg.up(proof, 80);
  auto dbeta = sg.out<uint8_t>(64);
  auto dver = sg.out<uint8_t>(1);
  if (sg.rc) return sg.rc;
  launch_vrf03_proof_to_hash(st, 1, (size_t)1, dpi, dbeta, dver);
  if ((rc = launch_check())) return rc;
  uint8_t beta[64], v = 0;
  if ((rc = download(st, beta, dbeta, 64))) return rc;
  if ((rc = download(st, &v, dver, 1))) return rc;
  if ((rc = finish(st))) return rc;
  if (!v) return OURO_INVALID;
  memcpy(output, beta, 64);
  return OURO_OK;
}

// (The cardano-crypto-praos names are NOT exported here: the opt-in
// lib/libouro_vrf_shim.so, csrc/vrf_shim.cpp, provides them.)

int ouro_sum6kes_verify(const unsigned char* vk, unsigned int t, const unsigned char* m,
                        unsigned long long mlen, const unsigned char* sig) {
  if (!vk || !sig || (mlen && !m)) return OURO_INVALID;
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)mlen;
  if ((unsigned long long)len != mlen) return fail(OURO_EINVAL, "message too long");
  uint8_t v = 0;
  const uint32_t tt = t;
  static const uint8_t empty[1] = {0};
  int rc;
  if (single_on_gpu()) {
    rc = ouro_sum6kes_verify_batch(1, vk, &tt, mlen ? m : empty, &off, &len, sig, &v);
  } else {
    g_host_single++;
    rc = ouro_host::kes_batch(1, vk, &tt, mlen ? m : empty, &off, &len, sig, &v);
  }
  if (rc) return rc;
  return v ? OURO_OK : OURO_INVALID;
}

// ---- device-resident batches ----
int ouro_ed25519_verify_batch_device(void* stream, size_t n, const uint8_t* pk, const uint8_t* sig,
                                     const uint8_t* msg, const uint64_t* msg_off,
                                     const uint32_t* msg_len, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_ed(st, n, pk, sig, msg, msg_off, msg_len, verdict);
}

int ouro_byron_ed25519_verify_batch_device(void* stream, size_t n, const uint8_t* pk,
                                           const uint8_t* sig, const uint8_t* msg,
                                           const uint64_t* msg_off, const uint32_t* msg_len,
                                           uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_ed(st, n, pk, sig, msg, msg_off, msg_len, verdict, 1);
}

int ouro_vrf03_verify_batch_device(void* stream, size_t n, const uint8_t* pk, const uint8_t* proof,
                                   const uint8_t* alpha, const uint64_t* alpha_off,
                                   const uint32_t* alpha_len, uint8_t* beta, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_vrf(st, n, pk, proof, alpha, alpha_off, alpha_len, beta, verdict);
}

int ouro_vrf03_verify_batch_device_flags(void* stream, size_t n, const uint8_t* pk,
                                         const uint8_t* proof, const uint8_t* alpha,
                                         const uint64_t* alpha_off, const uint32_t* alpha_len,
                                         uint8_t* beta, uint8_t* verdict, uint32_t flags) {
  if (n == 0) return OURO_OK;
  if (flags & ~OURO_VRF_STRICT_S) return fail(OURO_EINVAL, "unknown VRF flags");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_vrf(st, n, pk, proof, alpha, alpha_off, alpha_len, beta, verdict, flags);
}

int ouro_sum6kes_verify_batch_device(void* stream, size_t n, const uint8_t* vk, const uint32_t* t,
                                     const uint8_t* msg, const uint64_t* msg_off,
                                     const uint32_t* msg_len, const uint8_t* sig,
                                     uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_kes(st, n, vk, t, msg, msg_off, msg_len, sig, verdict);
}

int ouro_tpraos_verify_batch_device(void* stream, const ouro_tpraos_batch* b, uint8_t* verdict,
                                    uint8_t* beta_eta, uint8_t* beta_leader) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  if (b->n == 0) return OURO_OK;
  if (!beta_eta || !beta_leader) return fail(OURO_EINVAL, "device API needs both beta buffers");
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  hipStream_t st;
  if ((rc = device_entry(stream, &st))) return rc;
  return launch_hdr(st, *b, verdict, beta_eta, beta_leader);
}

int ouro_tpraos_pack_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                 const uint64_t* off, const uint32_t* len, size_t n,
                                 uint64_t slots_per_kes_period, void* arena, size_t arena_bytes,
                                 ouro_tpraos_batch* out, uint64_t* slot, uint8_t* era,
                                 uint8_t* status) {
  if (!out || slots_per_kes_period == 0) return fail(OURO_EINVAL, "null batch / zero period");
  if (n > 0 && (!raw || !off || !len || !arena || !status)) return fail(OURO_EINVAL, "null buffer");
  if (arena_bytes < ouro_tpraos_pack_bytes(n)) return fail(OURO_EINVAL, "arena too small");
  const cbor::Out o = cbor::arena_out(cbor::arena_base(arena), n, slot, era);
  cbor::batch_from(out, o, raw, n);
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  const size_t blocks = std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  launch_tpraos_pack(st, (unsigned)blocks, raw, raw_bytes, off, len, n, slots_per_kes_period, o,
                     status);
  return launch_check();
}

}  // extern "C"

extern "C" {

int ouro_leader_check_batch_device(void* stream, size_t n, const uint8_t* beta,
                                   const uint64_t* sigma_num, const uint64_t* sigma_den,
                                   int64_t act_log_hi, uint64_t act_log_lo, int f_is_one,
                                   uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_leader(st, n, beta, sigma_num, sigma_den, act_log_hi, act_log_lo, f_is_one,
                       verdict);
}

}  // extern "C"

namespace {
// The (offset, length) spans of a host-path batch: the same argument checks
// as the device calls' window_of: an offset + length that wraps,
// or a null buffer with any nonzero length, is OURO_EINVAL -- never a read of
// invalid memory.
int check_spans(size_t n, const uint64_t* off, const uint32_t* len, const void* buf,
                const char* what) {
  for (size_t i = 0; i < n; i++) {
    if (!len[i]) continue;
    if (off[i] + len[i] < off[i]) return fail(OURO_EINVAL, "offset + length overflows");
    if (!buf) return fail(OURO_EINVAL, std::string("null ") + what + " buffer");
  }
  return OURO_OK;
}
}  // namespace

extern "C" {

// ---- the host path, called explicitly (host_path.h) ----
int ouro_ed25519_verify_batch_host(size_t n, const uint8_t* pk, const uint8_t* sig,
                                   const uint8_t* msg, const uint64_t* msg_off,
                                   const uint32_t* msg_len, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!pk || !sig || !msg_off || !msg_len || !verdict) return fail(OURO_EINVAL, "null argument");
  if (int rc = check_spans(n, msg_off, msg_len, msg, "message")) return rc;
  return ouro_host::ed_batch(n, pk, sig, msg, msg_off, msg_len, verdict, 0);
}
int ouro_byron_ed25519_verify_batch_host(size_t n, const uint8_t* pk, const uint8_t* sig,
                                         const uint8_t* msg, const uint64_t* msg_off,
                                         const uint32_t* msg_len, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!pk || !sig || !msg_off || !msg_len || !verdict) return fail(OURO_EINVAL, "null argument");
  if (int rc = check_spans(n, msg_off, msg_len, msg, "message")) return rc;
  return ouro_host::ed_batch(n, pk, sig, msg, msg_off, msg_len, verdict, 1);
}
int ouro_vrf03_verify_batch_host(size_t n, const uint8_t* pk, const uint8_t* proof,
                                 const uint8_t* alpha, const uint64_t* alpha_off,
                                 const uint32_t* alpha_len, uint8_t* beta, uint8_t* verdict,
                                 uint32_t flags) {
  if (n == 0) return OURO_OK;
  if (flags & ~OURO_VRF_STRICT_S) return fail(OURO_EINVAL, "unknown VRF flags");
  if (!pk || !proof || !alpha_off || !alpha_len || !verdict) return fail(OURO_EINVAL, "null argument");
  if (int rc = check_spans(n, alpha_off, alpha_len, alpha, "alpha")) return rc;
  return ouro_host::vrf_batch(n, pk, proof, alpha, alpha_off, alpha_len, beta, verdict, flags);
}
int ouro_sum6kes_verify_batch_host(size_t n, const uint8_t* vk, const uint32_t* t,
                                   const uint8_t* msg, const uint64_t* msg_off,
                                   const uint32_t* msg_len, const uint8_t* sig, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!vk || !t || !msg_off || !msg_len || !sig || !verdict) return fail(OURO_EINVAL, "null argument");
  if (int rc = check_spans(n, msg_off, msg_len, msg, "message")) return rc;
  return ouro_host::kes_batch(n, vk, t, msg, msg_off, msg_len, sig, verdict);
}
int ouro_tpraos_verify_batch_host(const ouro_tpraos_batch* b, uint8_t* verdict,
                                  uint8_t* beta_eta, uint8_t* beta_leader) {
  if (!b) return fail(OURO_EINVAL, "null batch");
  if (b->n == 0) return OURO_OK;
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  int rc = check_hdr_batch(b);
  if (rc) return rc;
  if ((rc = check_spans(b->n, b->body_off, b->body_len, b->body, "body"))) return rc;
  return ouro_host::hdr_batch(b, verdict, beta_eta, beta_leader);
}
int ouro_tpraos_verify_batch_epochs_host(const ouro_tpraos_batch* b, const ouro_epoch_nonces* e,
                                         uint8_t* verdict, uint8_t* beta_eta,
                                         uint8_t* beta_leader) {
  std::vector<uint64_t> tab;
  int rc = check_epochs_batch(b, e, verdict, &tab);
  if (rc || b->n == 0) return rc;
  if ((rc = check_spans(b->n, b->body_off, b->body_len, b->body, "body"))) return rc;
  return ouro_host::hdr_batch(b, verdict, beta_eta, beta_leader,
                              reinterpret_cast<const uint8_t*>(tab.data()));
}
int ouro_leader_check_batch_host(size_t n, const uint8_t* beta, const uint64_t* sigma_num,
                                 const uint64_t* sigma_den, int64_t act_log_hi,
                                 uint64_t act_log_lo, int f_is_one, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!beta || !sigma_num || !sigma_den || !verdict) return fail(OURO_EINVAL, "null argument");
  return ouro_host::leader_batch(n, beta, sigma_num, sigma_den, act_log_hi, act_log_lo, f_is_one,
                                 verdict);
}

}  // extern "C"
