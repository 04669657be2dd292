// envelope_api.cpp -- the header envelope of a raw chain and every header's
// hash (include/ouro_verify.h ouro_chain_envelope_cbor; envelope.h): the
// argument checks, the host path (both slicers without their rows, the host
// build of the prefixed Blake2b-256, envelope_link) and the C entries.  Host
// code only: kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor.h"
#include "cbor_byron.h"
#include "envelope.h"
#include "host_util.h"
#include "launch.h"
#include "launches.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

struct EnvCall {
  const uint8_t* raw;
  size_t raw_bytes;
  const uint64_t* off;
  const uint32_t* len;
  size_t n;
  ouro_envelope_cfg cfg;
  env::Rec tip;
  uint8_t *status, *hash, *envelope;
  ouro_chain_tip* tip_out;
};

// everything that is OURO_EINVAL, before anything runs (`host`: the buffers
// are host memory, so spans and eras can be looked at)
int env_check(EnvCall* c, const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in, bool host) {
  if (!c->raw || !c->off || !c->len) return fail(OURO_EINVAL, "null argument");
  if (!c->status || !c->hash || !c->envelope)
    return fail(OURO_EINVAL, "null status, header_hash or envelope");
  if (int rc = env_args(cfg, tip_in, &c->tip)) return rc;
  c->cfg = *cfg;
  if (!host) return OURO_OK;
  if (int rc = spans_check("header", "raw_bytes", c->raw_bytes, c->off, c->len, c->n)) return rc;
  if (cfg->byron_epoch_slots == 0) return env_needs_epoch_slots(c->raw, c->off, c->len, c->n);
  return OURO_OK;
}

// one header on the host: what k_envelope_slice and k_header_hash do for it
uint8_t env_host_one(const EnvCall& c, size_t i, env::Rec* r) {
  env::rec_clear(r);
  const uint64_t o0 = c.off[i];
  const uint32_t l0 = c.len[i];
  uint8_t st;
  if (cbor::era_class(c.raw + o0, l0) == OURO_PROTO_PBFT)
    st = cbor::byron_pack_one<false>(c.raw, o0, l0, -1, cbor::ByronOut{}, i, r,
                                     c.cfg.byron_epoch_slots);
  else
    st = cbor::pack_one<false>(c.raw, o0, l0, 1, cbor::Out{}, i, r);
  if (r->sliced) {
    uint32_t npre, d[8];
    const uint32_t pre = env::hash_prefix(*r, &npre);
    blake2b256_stream_prefixed(d, pre, npre, c.raw + r->hdr_off, r->hdr_len);
    digest_bytes(r->hash, d);
  }
  return st;
}

// the host path: chunks of 64 K records over the worker pool, then the links
// in order, the last record of a chunk carried to the next
int env_host(const EnvCall& c, env::Rec* last = nullptr) {
  const size_t C = 1 << 16;
  std::vector<env::Rec> rec;
  try {  // (no exception crosses the C ABI)
    rec.resize(std::min(C, c.n));
  } catch (const std::bad_alloc&) {
    return fail(OURO_EDEVICE, "envelope host path: out of host memory");
  }
  env::Rec prev = c.tip;
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    const int rc = host_rows(m, 256, [&](size_t r0, size_t r1) {
      for (size_t i = r0; i < r1; i++) {
        const uint8_t st = env_host_one(c, lo + i, &rec[i]);
        if (c.status) c.status[lo + i] = st;
      }
    });
    if (rc) return rc;
    for (size_t i = 0; i < m; i++) {
      c.envelope[lo + i] = env::envelope_link(prev, rec[i], c.cfg);
      memcpy(c.hash + 32 * (lo + i), rec[i].hash, 32);
      prev = rec[i];
    }
  }
  if (c.tip_out) env::tip_of_rec(c.tip_out, prev);
  if (last) *last = prev;
  return OURO_OK;
}

// one upload, the three kernels and one copy back on the calling thread's stream
int env_dev(const EnvCall& c) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(c.n, c.off, c.len, &w))) return rc;
  using cbor::a64;
  const size_t n = c.n;
  // the results as one block: hash | envelope | status | tip
  const size_t o_env = 32 * n, o_st = o_env + a64(n), o_tip = o_st + a64(n);
  const size_t out_bytes = o_tip + sizeof(ouro_chain_tip);
  Stager sg{st};
  auto draw = sg.up(w.span() ? c.raw + w.lo : c.raw, w.span());
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(c.len, n);
  auto drec = sg.out<env::Rec>(n);
  auto dout = sg.out<uint8_t>(out_bytes);
  if (sg.rc) return sg.rc;
  if ((rc = launch_envelope(st, draw, w.span(), doff, dlen, n, c.cfg, c.tip, drec, dout + o_st,
                            dout, dout + o_env, reinterpret_cast<ouro_chain_tip*>(dout + o_tip))))
    return rc;
  std::vector<uint8_t> tv(out_bytes);
  if ((rc = download(st, tv.data(), dout, out_bytes))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(c.hash, tv.data(), 32 * n);
  memcpy(c.envelope, tv.data() + o_env, n);
  memcpy(c.status, tv.data() + o_st, n);
  if (c.tip_out) memcpy(c.tip_out, tv.data() + o_tip, sizeof(ouro_chain_tip));
  return OURO_OK;
}

}  // namespace

namespace ouro_rt {
// cfg and tip_in checked (OURO_EINVAL), the tip as a record
int env_args(const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in, env::Rec* tip) {
  if (!cfg) return fail(OURO_EINVAL, "null envelope cfg");
  if (tip_in) {
    ouro_chain_tip o{};
    o.origin = 1;
    if (tip_in->origin > 1 || (tip_in->origin && memcmp(tip_in, &o, sizeof o) != 0))
      return fail(OURO_EINVAL, "tip_in: origin set and another field nonzero");
    if (!tip_in->origin && ((tip_in->proto > OURO_PROTO_TPRAOS && tip_in->proto != 0xff) ||
                            tip_in->is_ebb > 1 ||
                            (tip_in->is_ebb && tip_in->proto != OURO_PROTO_PBFT)))
      return fail(OURO_EINVAL, "tip_in: proto or is_ebb out of range");
  }
  *tip = env::rec_of_tip(tip_in);
  if (tip_in && !tip_in->origin && tip_in->proto == 0xff) tip->sliced = 0;  // links to nothing
  return OURO_OK;
}
// byron_epoch_slots is 0: OURO_EINVAL if a header is PBFT (spans checked before)
int env_needs_epoch_slots(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (cbor::era_class(raw + off[i], len[i]) == OURO_PROTO_PBFT)
      return fail(OURO_EINVAL,
                  "header " + std::to_string(i) + " is PBFT and byron_epoch_slots is 0");
  return OURO_OK;
}
int env_host_run(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                 const ouro_envelope_cfg& cfg, const env::Rec& tip, uint8_t* status, uint8_t* hash,
                 uint8_t* envelope, env::Rec* last) {
  const EnvCall c{raw, 0, off, len, n, cfg, tip, status, hash, envelope, nullptr};
  return env_host(c, last);
}
}  // namespace ouro_rt

extern "C" {

// validateEnvelope (ouroboros-consensus/src/Ouroboros/Consensus/
// HeaderValidation.hs:297-344) and the header hash over a raw chain
int ouro_chain_envelope_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                  const uint32_t* len, size_t n, const ouro_envelope_cfg* cfg,
                                  const ouro_chain_tip* tip_in, uint8_t* status,
                                  uint8_t* header_hash, uint8_t* envelope,
                                  ouro_chain_tip* tip_out) {
  EnvCall c{raw, raw_bytes, off, len, n, {}, {}, status, header_hash, envelope, tip_out};
  if (n == 0) {  // nothing to link: the checked tip passes through
    if (int rc = env_args(cfg, tip_in, &c.tip)) return rc;
    if (tip_out) env::tip_of_rec(tip_out, c.tip);
    return OURO_OK;
  }
  if (int rc = env_check(&c, cfg, tip_in, true)) return rc;
  return env_host(c);
}

int ouro_chain_envelope_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                             const uint32_t* len, size_t n, const ouro_envelope_cfg* cfg,
                             const ouro_chain_tip* tip_in, uint8_t* status, uint8_t* header_hash,
                             uint8_t* envelope, ouro_chain_tip* tip_out) {
  EnvCall c{raw, raw_bytes, off, len, n, {}, {}, status, header_hash, envelope, tip_out};
  if (n == 0) {  // nothing to link: the checked tip passes through
    if (int rc = env_args(cfg, tip_in, &c.tip)) return rc;
    if (tip_out) env::tip_of_rec(tip_out, c.tip);
    return OURO_OK;
  }
  if (int rc = env_check(&c, cfg, tip_in, true)) return rc;
  return or_host(env_dev(c), [&] { return env_host(c); });
}

size_t ouro_chain_envelope_work_bytes(size_t n) { return sizeof(env::Rec) * n + 64; }

int ouro_chain_envelope_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                    const uint64_t* off, const uint32_t* len, size_t n,
                                    const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in,
                                    void* work, size_t work_bytes, uint8_t* status,
                                    uint8_t* header_hash, uint8_t* envelope,
                                    ouro_chain_tip* tip_out) {
  EnvCall c{raw, raw_bytes, off, len, n, {}, {}, status, header_hash, envelope, tip_out};
  if (n == 0) return env_args(cfg, tip_in, &c.tip);  // (nothing is enqueued or written)
  if (int rc = env_check(&c, cfg, tip_in, false)) return rc;
  if (!work || work_bytes < ouro_chain_envelope_work_bytes(n))
    return fail(OURO_EINVAL, "work area too small");
  if (misaligned(raw, 4)) return fail(OURO_EINVAL, "raw must be 4-byte aligned");
  if (misaligned(header_hash, 16)) return fail(OURO_EINVAL, "header_hash must be 16-byte aligned");
  if (misaligned(tip_out, 8)) return fail(OURO_EINVAL, "tip_out must be 8-byte aligned");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_envelope(st, raw, raw_bytes, off, len, n, c.cfg, c.tip,
                         reinterpret_cast<env::Rec*>(cbor::arena_base(work)), status, header_hash,
                         envelope, tip_out);
}

}  // extern "C"
