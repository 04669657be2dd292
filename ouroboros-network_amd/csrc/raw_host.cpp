// raw_host.cpp -- the host path of a raw-CBOR call (raw_call.h raw_host): what
// raw_pipe.cpp's pipeline computes, recomputed after a device error or run
// alone by a *_host entry -- the host slicers and the host build of the lane
// routines (host_path.h), in chunks, results straight into the caller's
// buffers.  Host code only.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "cbor_byron.h"
#include "host_path.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

namespace {
// the host path over the same batch: host slicer + host verification, in
// chunks (no batch-sized arena), results straight into the caller's buffers
int raw_host_byron(const RawCall& c) {
  const size_t C = 1 << 16;
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    const size_t nb = ouro_byron_pack_bytes(m, c.len + lo);
    std::unique_ptr<uint8_t[]> arena(new (std::nothrow) uint8_t[nb]);  // every row written
    if (!arena) return fail(OURO_EDEVICE, "raw Byron host path: out of host memory");
    ouro_byron_batch b;
    int rc = ouro_byron_pack_cbor(c.raw, c.raw_bytes, c.off + lo, c.len + lo, m, c.magic,
                                  arena.get(), nb, &b, c.status + lo, 0);
    if (rc) return fail(rc, "ouro_byron_pack_cbor: bad arguments");
    if ((rc = ouro_host::ed_batch(m, b.pk, b.sig, b.msg, b.msg_off, b.msg_len, c.verdict + lo, 1)))
      return fail(rc, "raw Byron host path failed");
    for (size_t i = lo; i < lo + m; i++)
      c.verdict[i] = c.status[i] == OURO_PACK_EBB ? 1
                                                  : (c.status[i] == OURO_PACK_OK && c.verdict[i]);
  }
  return OURO_OK;
}

// a ledger call on the host path: the TPraos headers sliced again on the host
// in chunks, ledger_check_lane over their rows, the fold in stream order
// (c.proto and c.status are the chain kind's, already written)
int raw_host_ledger(const RawCall& c) {
  RawLedger& L = *c.ledger;
  L.fold_begin();
  const size_t C = 1 << 16;
  std::vector<uint32_t> ix, rows;
  std::vector<uint64_t> off, slots;
  std::vector<uint32_t> len;
  std::vector<uint8_t> st, bits, arena;
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    memset(L.ledger + lo, 0, m);
    ix.clear();
    for (size_t i = lo; i < lo + m; i++) {
      L.pool_row[i] = OURO_LV_NO_POOL;
      if (c.proto[i] == OURO_PROTO_TPRAOS) ix.push_back((uint32_t)(i - lo));
    }
    const size_t q = ix.size();
    if (!q) continue;
    off.resize(q), len.resize(q), slots.resize(q), st.resize(q), bits.resize(q), rows.resize(q);
    for (size_t j = 0; j < q; j++) {
      off[j] = c.off[lo + ix[j]];
      len[j] = c.len[lo + ix[j]];
    }
    arena.resize(ouro_tpraos_pack_bytes(q));
    ouro_tpraos_batch b{};
    int rc = ouro_tpraos_pack_cbor(c.raw, c.raw_bytes, off.data(), len.data(), q, c.spkp,
                                   arena.data(), arena.size(), &b, slots.data(), nullptr, st.data(),
                                   0);
    if (rc) return fail(rc, "ouro_tpraos_pack_cbor: bad arguments");
    if ((rc = lv_host_rows(q, b.issuer_vk, b.vrf_vk, slots.data(), b.leader_output,
                           b.ocert_kes_period, *L.views, L.g, L.genesis, bits.data(),
                           rows.data())))
      return rc;
    for (size_t j = 0; j < q; j++) {
      if (st[j] != OURO_PACK_OK) continue;
      const size_t i = lo + ix[j];
      L.ledger[i] = bits[j];
      L.pool_row[i] = rows[j];
      if (L.fold) lv_fold_run(L.fold, 1, &rows[j], &b.ocert_counter[j], &L.ledger[i]);
    }
  }
  return OURO_OK;
}

// a PBFT call on the host path: the Byron headers sliced again on the host in
// chunks (their slots from the envelope's record of the same header),
// pbft_check_lane over their rows, the window fold in stream order restarted
// from the state as the call found it (c.proto is the chain kind's, already
// written)
int raw_host_pbft(const RawCall& c) {
  RawPbft& B = *c.pbft;
  B.fold_begin();
  const size_t C = 1 << 16;
  std::vector<uint32_t> ix, rows;
  std::vector<uint64_t> off, slots;
  std::vector<uint32_t> len;
  std::vector<uint8_t> st, bits, arena;
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    memset(B.pbft + lo, 0, m);
    if (B.signed_count) memset(B.signed_count + lo, 0, 8 * m);
    ix.clear();
    for (size_t i = lo; i < lo + m; i++) {
      B.genesis_row[i] = OURO_LV_NO_POOL;
      if (c.proto[i] == OURO_PROTO_PBFT) ix.push_back((uint32_t)(i - lo));
    }
    const size_t q = ix.size();
    if (!q) continue;
    off.resize(q), len.resize(q), slots.resize(q), st.resize(q), bits.resize(q), rows.resize(q);
    for (size_t j = 0; j < q; j++) {
      off[j] = c.off[lo + ix[j]];
      len[j] = c.len[lo + ix[j]];
      env::Rec r;
      env::rec_clear(&r);
      cbor::byron_pack_one<false>(c.raw, off[j], len[j], -1, cbor::ByronOut{}, j, &r,
                                  c.env->cfg.byron_epoch_slots);
      slots[j] = r.slot;
    }
    arena.resize(ouro_byron_pack_bytes(q, len.data()));
    ouro_byron_batch b;
    int rc = ouro_byron_pack_cbor(c.raw, c.raw_bytes, off.data(), len.data(), q, c.magic,
                                  arena.data(), arena.size(), &b, st.data(), 0);
    if (rc) return fail(rc, "ouro_byron_pack_cbor: bad arguments");
    if ((rc = pbft_host_rows(q, b.delegate_vk, slots.data(), st.data(), *B.views, bits.data(),
                             rows.data())))
      return rc;
    for (size_t j = 0; j < q; j++) {
      if (st[j] != OURO_PACK_OK && st[j] != OURO_PACK_EBB) continue;
      const size_t i = lo + ix[j];
      B.pbft[i] = bits[j];
      B.genesis_row[i] = rows[j];
      if (B.fold)
        pbft_fold_run(B.fold, 1, &rows[j], &slots[j], &B.pbft[i],
                      B.signed_count ? &B.signed_count[i] : nullptr);
    }
  }
  return OURO_OK;
}

// The combined entry on the host path: per chunk of 64 K headers the same
// partition as a mixed device chunk -- each class's offset / length (and
// alpha) list through its own host slicer and verification, both result sets
// scattered back to the caller's order.
int raw_host_chain(const RawCall& c) {
  const size_t C = 1 << 16;
  std::vector<uint32_t> idx[2];
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<uint8_t> st, v, be, bl, en, ea, la;
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    idx[0].clear();
    idx[1].clear();
    for (size_t i = lo; i < lo + m; i++) {  // (every span was checked before any work)
      c.proto[i] = (uint8_t)cbor::era_class(c.raw + c.off[i], c.len[i]);
      idx[c.proto[i] == OURO_PROTO_TPRAOS ? 1 : 0].push_back((uint32_t)(i - lo));
    }
    for (int cls = 0; cls < 2; cls++) {
      const std::vector<uint32_t>& ix = idx[cls];
      const size_t q = ix.size();
      if (!q) continue;
      off.resize(q);
      len.resize(q);
      st.assign(q, 0);
      v.assign(q, 0);
      for (size_t j = 0; j < q; j++) {
        off[j] = c.off[lo + ix[j]];
        len[j] = c.len[lo + ix[j]];
      }
      RawCall sub = RawCall::of(cls ? kRawHdr : kRawByron, c.raw, c.raw_bytes, off.data(),
                                len.data(), q, st.data(), v.data());
      sub.spkp = c.spkp;
      sub.magic = c.magic;
      if (cls) {
        if (c.ea) {
          ea.resize(32 * q);
          la.resize(32 * q);
          for (size_t j = 0; j < q; j++) {
            memcpy(&ea[32 * j], c.ea + 32 * (lo + ix[j]), 32);
            memcpy(&la[32 * j], c.la + 32 * (lo + ix[j]), 32);
          }
          sub.ea = ea.data();
          sub.la = la.data();
        }
        sub.epochs = c.epochs;
        sub.epochs_bytes = c.epochs_bytes;
        if (c.be) be.assign(64 * q, 0), sub.be = be.data();
        if (c.bl) bl.assign(64 * q, 0), sub.bl = bl.data();
        if (c.nonce) en.assign(32 * q, 0), sub.nonce = en.data();
      }
      const int rc = raw_host(sub);
      if (rc) return rc;
      for (size_t j = 0; j < q; j++) {
        const size_t i = lo + ix[j];
        c.status[i] = st[j];
        c.verdict[i] = v[j];
        // (a PBFT header has no VRF outputs: zero rows)
        if (c.be) cls ? memcpy(c.be + 64 * i, &be[64 * j], 64) : memset(c.be + 64 * i, 0, 64);
        if (c.bl) cls ? memcpy(c.bl + 64 * i, &bl[64 * j], 64) : memset(c.bl + 64 * i, 0, 64);
        if (c.nonce) cls ? memcpy(c.nonce + 32 * i, &en[32 * j], 32) : memset(c.nonce + 32 * i, 0, 32);
      }
    }
  }
  return OURO_OK;
}

}  // namespace

namespace ouro_rt {
int raw_host(const RawCall& c) {
  if (c.kind == kRawByron) return raw_host_byron(c);
  if (c.kind == kRawBlock) return block_host(c);
  if (c.kind == kRawChain) {
    try {  // (its lists are vectors; no exception crosses the C ABI)
      if (int rc = raw_host_chain(c)) return rc;
      if (c.ledger)
        if (int rc = raw_host_ledger(c)) return rc;
      if (c.pbft)
        if (int rc = raw_host_pbft(c)) return rc;
      if (!c.env) return OURO_OK;
      // a validating call: the envelope with the host build of the same routines
      if (int rc = env_host_run(c.raw, c.off, c.len, c.n, c.env->cfg, c.env->tip, nullptr,
                                c.env->hash, c.env->envelope, &c.env->prev))
        return rc;
      if (c.env->tip_out) env::tip_of_rec(c.env->tip_out, c.env->prev);
      return OURO_OK;
    } catch (const std::bad_alloc&) {
      return fail(OURO_EDEVICE, "raw CBOR host path: out of host memory");
    }
  }
  const size_t C = 1 << 16;
  const size_t cap = std::min(C, c.n);
  const size_t nb = ouro_tpraos_pack_bytes(cap);
  std::unique_ptr<uint8_t[]> arena(new (std::nothrow) uint8_t[nb]);
  std::unique_ptr<uint64_t[]> slots(new (std::nothrow) uint64_t[cap]);
  if (!arena || !slots) return fail(OURO_EDEVICE, "raw CBOR host path: out of host memory");
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    ouro_tpraos_batch b{};  // (the slicer sets the required members only)
    int rc = ouro_tpraos_pack_cbor(c.raw, c.raw_bytes, c.off + lo, c.len + lo, m, c.spkp,
                                   arena.get(), nb, &b, slots.get(), nullptr, c.status + lo, 0);
    if (rc) return fail(rc, "ouro_tpraos_pack_cbor: bad arguments");
    if (c.kind == kRawKes) {
      rc = ouro_host::kes_batch(m, b.hot_vk, b.kes_t, b.body, b.body_off, b.body_len, b.kes_sig,
                                c.verdict + lo);
    } else {
      if (c.ea) {
        b.eta_alpha = c.ea + 32 * lo;
        b.leader_alpha = c.la + 32 * lo;
      } else {
        b.slot = slots.get();
        b.epoch_nonce = c.eta0;
      }
      if (c.nonce) b.eta_nonce = c.nonce + 32 * lo;
      rc = ouro_host::hdr_batch(&b, c.verdict + lo, c.be ? c.be + 64 * lo : nullptr,
                                c.bl ? c.bl + 64 * lo : nullptr, c.ea ? nullptr : c.epochs);
    }
    if (rc) return fail(rc, "raw CBOR host path failed");
    for (size_t i = lo; i < lo + m; i++)
      if (c.status[i] != OURO_PACK_OK) c.verdict[i] = 0;
  }
  return OURO_OK;
}
}  // namespace ouro_rt
