// forge_api.cpp -- the forging-side entries of the C ABI (include/ouro_verify.h
// ouro_vrf03_prove*, ouro_tpraos_leader_schedule*, ouro_tpraos_leader_vrfs*):
// PraosVRF evalCertified in batches and checkIsLeader over a slot range
// (forge.h).  Every entry validates first; the device forms stage on the
// calling thread's stream and recompute on the host path after a device error.
// Host code only: kernels are reached through launches.h.
//
// Key hygiene: a signing key lives in the caller's memory, in call-local host
// memory here (zeroed before returning), in a launch's arguments, or in this
// call's staging buffer on the device (zeroed before returning, KeyWipe).
// Nothing of a key goes into an error text.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "host_path.h"
#include "host_util.h"
#include "launch.h"
#include "launches.h"
#include "leader.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

void wipe(void* p, size_t n) {
  volatile uint8_t* q = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) q[i] = 0;
}

// a key's staging buffer on the device, zeroed when the call leaves, whatever
// way it leaves; the stream is drained so the zeros are there on return
struct KeyWipe {
  hipStream_t st;
  void* p = nullptr;
  size_t bytes = 0;
  ~KeyWipe() {
    if (!p) return;
    (void)hipMemsetAsync(p, 0, bytes, st);
    (void)hipStreamSynchronize(st);
  }
};

// ---- ouro_vrf03_prove_batch ----
int prove_check(size_t n, const uint8_t* sk, size_t nkeys, const uint8_t* alpha, size_t alpha_bytes,
                const uint64_t* off, const uint32_t* len, const uint8_t* proof) {
  if (!sk || !off || !len || !proof || (!alpha && alpha_bytes))
    return fail(OURO_EINVAL, "null argument");
  if (nkeys != 1 && nkeys != n) return fail(OURO_EINVAL, "nkeys must be 1 or n");
  return spans_check("alpha", "alpha_bytes", alpha_bytes, off, len, n);
}

int prove_dev(size_t n, const uint8_t* sk, size_t nkeys, const uint8_t* alpha, const uint64_t* off,
              const uint32_t* len, uint8_t* proof, uint8_t* beta) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, off, len, &w))) return rc;
  Stager sg{st};
  KeyWipe kw{st};
  // (the kernel reads the aligned dwords a span touches: up to the next multiple of 4)
  auto dal = sg.out<uint8_t>(w.span() + 4);
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(len, n);
  auto dpi = sg.out<uint8_t>(80 * n);
  auto dbeta = sg.out<uint8_t>(64 * n);
  auto dsk = sg.up(sk, 64 * nkeys);
  kw.p = dsk;
  kw.bytes = 64 * nkeys;
  if (sg.rc) return sg.rc;
  if (w.span()) OURO_HIP(hipMemcpyAsync(dal, alpha + w.lo, w.span(), hipMemcpyHostToDevice, st));
  if ((rc = launch_vrf_prove(st, n, dsk, nkeys == 1, dal, doff, dlen, nullptr, nullptr, dpi,
                             beta ? dbeta : nullptr)))
    return rc;
  std::vector<uint8_t> tp(80 * n), tb(beta ? 64 * n : 0);
  if ((rc = download(st, tp.data(), dpi, 80 * n))) return rc;
  if (beta && (rc = download(st, tb.data(), dbeta, 64 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(proof, tp.data(), 80 * n);
  if (beta) memcpy(beta, tb.data(), 64 * n);
  return OURO_OK;
}

int prove_call(size_t n, const uint8_t* sk, size_t nkeys, const uint8_t* alpha, size_t alpha_bytes,
               const uint64_t* off, const uint32_t* len, uint8_t* proof, uint8_t* beta, bool host) {
  if (n == 0) return OURO_OK;
  if (int rc = prove_check(n, sk, nkeys, alpha, alpha_bytes, off, len, proof)) return rc;
  auto on_host = [&] {
    const int rc = ouro_host::prove_batch(n, sk, nkeys == 1, alpha, off, len, nullptr, nullptr,
                                          proof, beta);
    return rc ? fail(rc, "prover host path failed") : OURO_OK;
  };
  return host ? on_host() : or_host(prove_dev(n, sk, nkeys, alpha, off, len, proof, beta), on_host);
}

// ---- ouro_tpraos_leader_schedule ----
// sigma and act_log inside ouro_leader_check_batch's domain (leader.h): the
// routine itself says so, on an all-zero output
bool leader_domain(const ouro_leader_params& p) {
  if (p.sigma_den == 0 || p.sigma_num > p.sigma_den) return false;
  if (p.f_is_one) return true;
  const uint8_t zero[64] = {0};
  return leader_check_lane(zero, p.sigma_num, p.sigma_den, p.act_log_lo, p.act_log_hi) !=
         kLeaderBadArg;
}

int sched_check(const uint8_t* sk, const ouro_leader_params* p, uint64_t first_slot, size_t n,
                const uint8_t* cls) {
  if (!sk || !p || !cls) return fail(OURO_EINVAL, "null argument");
  if ((uint64_t)(n - 1) > ~(uint64_t)0 - first_slot)
    return fail(OURO_EINVAL, "first_slot + n_slots wraps");
  if (!leader_domain(*p)) return fail(OURO_EINVAL, "sigma or act_log outside the leader check's domain");
  if (p->d_den == 0 || p->d_num > p->d_den) return fail(OURO_EINVAL, "d outside [0, 1]");
  if (p->d_num) {
    if (p->asc_inv == 0 || p->ngen == 0)
      return fail(OURO_EINVAL, "an overlay schedule (d > 0) needs asc_inv and ngen");
    if (first_slot < p->epoch_first_slot)
      return fail(OURO_EINVAL, "first_slot before epoch_first_slot");
  }
  return OURO_OK;
}

void sched_arg(OuroForgeSched* s, const uint8_t* sk, const ouro_leader_params& p) {
  memset(s, 0, sizeof *s);
  ouro_host::sched_key(s, sk);
  if (p.epoch_nonce) {
    memcpy(s->eta0, p.epoch_nonce, 32);
    s->have_eta0 = 1;
  }
  s->f_is_one = p.f_is_one ? 1 : 0;
  s->ngen = p.d_num ? p.ngen : 0;
  s->epoch_first_slot = p.d_num ? p.epoch_first_slot : 0;
  s->sigma_num = p.sigma_num;
  s->sigma_den = p.sigma_den;
  s->act_log_lo = p.act_log_lo;
  s->act_log_hi = p.act_log_hi;
  s->d_num = p.d_num;
  s->d_den = p.d_den;
  s->asc_inv = p.d_num ? p.asc_inv : 1;
}

int sched_dev(const OuroForgeSched& s, uint64_t first_slot, size_t n, uint8_t* cls,
              uint32_t* gen_index, uint8_t* beta) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Stager sg{st};
  auto dcls = sg.out<uint8_t>(n);
  auto dgi = sg.out<uint32_t>(gen_index ? n : 0);
  auto dbeta = sg.out<uint8_t>(beta ? 64 * n : 0);
  if (sg.rc) return sg.rc;
  if ((rc = launch_leader_schedule(st, s, first_slot, n, dcls, gen_index ? dgi : nullptr,
                                   beta ? dbeta : nullptr)))
    return rc;
  std::vector<uint8_t> tc(n), tb(beta ? 64 * n : 0);
  std::vector<uint32_t> tg(gen_index ? n : 0);
  if ((rc = download(st, tc.data(), dcls, n))) return rc;
  if (gen_index && (rc = download(st, tg.data(), dgi, 4 * n))) return rc;
  if (beta && (rc = download(st, tb.data(), dbeta, 64 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(cls, tc.data(), n);
  if (gen_index) memcpy(gen_index, tg.data(), 4 * n);
  if (beta) memcpy(beta, tb.data(), 64 * n);
  return OURO_OK;
}

int sched_call(const uint8_t* sk, const ouro_leader_params* p, uint64_t first_slot, size_t n,
               uint8_t* cls, uint32_t* gen_index, uint8_t* beta, bool host) {
  if (n == 0) return OURO_OK;
  if (int rc = sched_check(sk, p, first_slot, n, cls)) return rc;
  OuroForgeSched s;
  sched_arg(&s, sk, *p);
  auto on_host = [&] {
    const int rc = ouro_host::sched_batch(s, first_slot, n, cls, gen_index, beta);
    return rc ? fail(rc, "leader schedule host path failed") : OURO_OK;
  };
  const int rc = host ? on_host()
                      : or_host(sched_dev(s, first_slot, n, cls, gen_index, beta), on_host);
  wipe(&s, sizeof s);
  return rc;
}

// ---- ouro_tpraos_leader_vrfs ----
// item 2 j: the eta VRF of slot[j]; item 2 j + 1: its leader VRF
void vrfs_split(size_t m, const uint8_t* pi, const uint8_t* be, uint8_t* eta_proof,
                uint8_t* eta_output, uint8_t* leader_proof, uint8_t* leader_output) {
  for (size_t j = 0; j < m; j++) {
    memcpy(eta_proof + 80 * j, pi + 160 * j, 80);
    memcpy(leader_proof + 80 * j, pi + 160 * j + 80, 80);
    if (eta_output) memcpy(eta_output + 64 * j, be + 128 * j, 64);
    if (leader_output) memcpy(leader_output + 64 * j, be + 128 * j + 64, 64);
  }
}

int vrfs_dev(const uint8_t* sk, const uint8_t* eta0, size_t m, const uint64_t* slot, uint8_t* pi,
             uint8_t* be) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Stager sg{st};
  KeyWipe kw{st};
  auto dslot = sg.up(slot, m);
  auto deta = sg.up(eta0, eta0 ? 32 : 0);
  auto dpi = sg.out<uint8_t>(160 * m);
  auto dbe = sg.out<uint8_t>(128 * m);
  auto dsk = sg.up(sk, 64);
  kw.p = dsk;
  kw.bytes = 64;
  if (sg.rc) return sg.rc;
  if ((rc = launch_vrf_prove(st, 2 * m, dsk, true, nullptr, nullptr, nullptr, dslot,
                             eta0 ? deta : nullptr, dpi, dbe)))
    return rc;
  if ((rc = download(st, pi, dpi, 160 * m)) || (rc = download(st, be, dbe, 128 * m))) return rc;
  return finish(st);
}

int vrfs_call(const uint8_t* sk, const uint8_t* eta0, size_t m, const uint64_t* slot,
              uint8_t* eta_proof, uint8_t* eta_output, uint8_t* leader_proof,
              uint8_t* leader_output, bool host) {
  if (m == 0) return OURO_OK;
  if (!sk || !slot || !eta_proof || !leader_proof) return fail(OURO_EINVAL, "null argument");
  if (m > ~(size_t)0 / 320) return fail(OURO_EINVAL, "too many slots");
  std::vector<uint8_t> pi(160 * m), be(128 * m);
  auto on_host = [&] {
    const int rc = ouro_host::prove_batch(2 * m, sk, true, nullptr, nullptr, nullptr, slot, eta0,
                                          pi.data(), be.data());
    return rc ? fail(rc, "prover host path failed") : OURO_OK;
  };
  const int rc = host ? on_host() : or_host(vrfs_dev(sk, eta0, m, slot, pi.data(), be.data()), on_host);
  if (rc) return rc;
  vrfs_split(m, pi.data(), be.data(), eta_proof, eta_output, leader_proof, leader_output);
  return OURO_OK;
}

}  // namespace

extern "C" {

int ouro_vrf03_prove_batch(size_t n, const uint8_t* sk, size_t nkeys, const uint8_t* alpha,
                           size_t alpha_bytes, const uint64_t* alpha_off,
                           const uint32_t* alpha_len, uint8_t* proof, uint8_t* beta) {
  return prove_call(n, sk, nkeys, alpha, alpha_bytes, alpha_off, alpha_len, proof, beta, false);
}

int ouro_vrf03_prove_batch_host(size_t n, const uint8_t* sk, size_t nkeys, const uint8_t* alpha,
                                size_t alpha_bytes, const uint64_t* alpha_off,
                                const uint32_t* alpha_len, uint8_t* proof, uint8_t* beta) {
  return prove_call(n, sk, nkeys, alpha, alpha_bytes, alpha_off, alpha_len, proof, beta, true);
}

int ouro_vrf03_prove(uint8_t proof[80], const uint8_t sk[64], const uint8_t* m, size_t mlen) {
  if (!proof || !sk || (mlen && !m)) return fail(OURO_EINVAL, "null argument");
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)mlen;
  if ((size_t)len != mlen) return fail(OURO_EINVAL, "message too long");
  g_host_single++;
  return prove_call(1, sk, 1, m, mlen, &off, &len, proof, nullptr, true);
}

int ouro_vrf03_keypair_from_seed(uint8_t pk[32], uint8_t sk[64], const uint8_t seed[32]) {
  if (!pk || !sk || !seed) return fail(OURO_EINVAL, "null argument");
  uint8_t t[32];
  ouro_host::vrf_public_key(t, seed);
  memmove(sk, seed, 32);
  memcpy(sk + 32, t, 32);
  memcpy(pk, t, 32);
  return OURO_OK;
}

int ouro_tpraos_leader_schedule(const uint8_t vrf_sk[64], const ouro_leader_params* p,
                                uint64_t first_slot, size_t n_slots, uint8_t* cls,
                                uint32_t* gen_index, uint8_t* beta_leader) {
  return sched_call(vrf_sk, p, first_slot, n_slots, cls, gen_index, beta_leader, false);
}

int ouro_tpraos_leader_schedule_host(const uint8_t vrf_sk[64], const ouro_leader_params* p,
                                     uint64_t first_slot, size_t n_slots, uint8_t* cls,
                                     uint32_t* gen_index, uint8_t* beta_leader) {
  return sched_call(vrf_sk, p, first_slot, n_slots, cls, gen_index, beta_leader, true);
}

int ouro_tpraos_leader_vrfs(const uint8_t vrf_sk[64], const uint8_t* epoch_nonce, size_t m,
                            const uint64_t* slot, uint8_t* eta_proof, uint8_t* eta_output,
                            uint8_t* leader_proof, uint8_t* leader_output) {
  return vrfs_call(vrf_sk, epoch_nonce, m, slot, eta_proof, eta_output, leader_proof,
                   leader_output, false);
}

int ouro_tpraos_leader_vrfs_host(const uint8_t vrf_sk[64], const uint8_t* epoch_nonce, size_t m,
                                 const uint64_t* slot, uint8_t* eta_proof, uint8_t* eta_output,
                                 uint8_t* leader_proof, uint8_t* leader_output) {
  return vrfs_call(vrf_sk, epoch_nonce, m, slot, eta_proof, eta_output, leader_proof,
                   leader_output, true);
}

}  // extern "C"
