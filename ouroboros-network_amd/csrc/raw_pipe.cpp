// raw_pipe.cpp -- raw header CBOR in host memory -> verdicts in one call: the
// engine, a chunked multi-slot pipeline (raw_run) behind raw_verify.  Its
// host-path recompute is raw_host.cpp, the *_verify_cbor entries over it are
// chain_api.cpp.  Host code only: kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "cbor_byron.h"
#include "host_util.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

// ---- raw header CBOR in host memory -> verdicts in one call -----------------
// The reference's bulk callers hold raw header bytes in host memory: ChainDB's
// re-validation of a chain suffix (ouroboros-consensus/src/Ouroboros/Consensus/
// Storage/ChainDB/Impl/LgrDB.hs:350-368), ChainSync windows
// (.../MiniProtocol/ChainSync/Client.hs:792), and storage integrity on every
// block (.../Storage/VolatileDB/Impl/Parser.hs:66-85,
// .../Storage/ImmutableDB/Impl/Validation.hs:358-365).  raw_run takes such a
// batch straight through the device:
//   * the batch is cut into chunks of whole headers (OURO_CBOR_CHUNK headers,
//     default 65,536, and at most kRawChunkBytes of raw bytes each);
//   * chunk c runs on slot c % S (S = OURO_CBOR_SLOTS streams, default 6 for
//     headers, 4 for integrity):
//     the library's worker pool gathers its header spans from the caller's
//     pageable buffer into the slot's pinned, NUMA-local staging (runs of
//     adjacent spans as one memcpy; offsets rebased by a prefix sum), the
//     slot's stream uploads that block -- the raw bytes, ~1 KB per header,
//     not the 1.4 KB SoA --, runs the device slicer (k_tpraos_pack) into the
//     slot's arena, then the header kernel with mkSeed from (slot, eta0) on
//     the device (or the Sum6KES kernel, for integrity), and copies status,
//     verdicts and outputs back into pinned memory;
//   * before reusing a slot the host harvests its previous chunk into the
//     caller's buffers, so up to S chunks are in flight: the host's gathers,
//     the uploads and the other slots' kernels overlap, and the kernels of
//     neighbouring chunks share the CUs as each one's waves retire.
// A device error stops the pipeline (everything in flight is waited for) and
// the whole batch is recomputed on the host path (raw_host.cpp raw_host).
// The combined entry (kRawChain, ouro_chain_verify_cbor) classifies every
// header while it is gathered (cbor.h era_class): a chunk of one era runs that
// era's path above, a mixed chunk both slicers and both kernels on its one
// upload, each over its own offset / length list (raw_stage, raw_launch), and
// raw_drain scatters the two result sets back to the caller's order.
// A validating call (ouro_chain_validate_cbor) is the chain kind with
// RawCall::env set: behind each chunk's work, on the same stream, the envelope
// kernels (launches.h launch_envelope) over the chunk in the caller's order;
// raw_drain links each chunk's first header to the chunk before it.
// A ledger call (ouro_chain_validate_ledger_cbor) is a validating call with
// RawCall::ledger set: the views uploaded once, k_ledger_checks behind each
// chunk's header kernel over the rows in the slot's arena (launches.h
// launch_ledger), the OCERT counter fold in stream order as chunks drain.
// With a genesis-delegation schedule (RawLedger::genesis) it rides in the
// views' block and the kernel is k_ledger_checks_overlay (raw_call.h lv_launch).
namespace {
constexpr size_t kRawChunkBytes = (size_t)96 << 20;

// (RawKind, RawCall: raw_call.h)
struct RawChunk {
  size_t lo, m, bytes;
};

// the pinned / device input block of a chunk of m headers and `bytes` raw bytes
// (tab: the call's epoch-nonce schedule block, uploaded with every chunk)
// (eoff / elen, behind everything else: a validating call's mixed chunk keeps
// the caller-order offset and length lists for the envelope kernels, which
// link each header to its neighbour in the stream; total_env includes them)
struct RawIn {
  size_t off, len, eta0, alpha, tab, raw, total, eoff, elen, total_env;
};
RawIn raw_in(size_t m, size_t bytes, bool alphas, size_t tab_bytes) {
  RawIn l;
  l.off = 0;
  l.len = a16(8 * m);
  l.eta0 = l.len + a16(4 * m);
  l.alpha = l.eta0 + 32;
  l.tab = a16(l.alpha + (alphas ? 64 * m : 0));
  l.raw = l.tab + a16(tab_bytes);
  l.total = l.raw + a16(std::max<size_t>(bytes, 16));
  l.eoff = l.total;
  l.elen = l.eoff + a16(8 * m);
  l.total_env = l.elen + a16(4 * m);
  return l;
}
// the Byron results of a mixed chunk (mb PBFT headers), behind the TPraos block
struct RawOutB {
  size_t status, verdict, total;
};
RawOutB raw_out_b(size_t mb) { return RawOutB{0, a16(mb), a16(mb) + a16(mb)}; }
// its result block: status | verdict | beta_eta | beta_leader | eta_nonce | slot
struct RawOut {
  size_t status, verdict, be, bl, nonce, slot, total;
};
RawOut raw_out(size_t m) {
  RawOut o;
  o.status = 0;
  o.verdict = a16(m);
  o.be = o.verdict + a16(m);
  o.bl = o.be + 64 * m;
  o.nonce = o.bl + 64 * m;
  o.slot = o.nonce + 32 * m;  // device only: the slicer's slots for mkSeed
  o.total = o.slot + 8 * m;
  return o;
}
// bytes of the result block copied back
size_t raw_out_bytes(const RawCall& c, const RawOut& o, size_t m) {
  // (the block kind: its body hashes, 32 B each, where beta_eta would start)
  if (c.kind == kRawBlock) return c.body_hash ? o.be + 32 * m : o.verdict + m;
  if (c.kind != kRawHdr && c.kind != kRawChain) return o.verdict + m;
  if (c.nonce) return o.slot;
  if (c.bl) return o.nonce;
  if (c.be) return o.bl;
  return o.verdict + m;
}

// a validating call's envelope block of a chunk: on the device the records,
// then what is copied back -- hash | bits | the first and the last record --
// then the envelope slicer's status (not copied: the chain kind's is the same)
struct RawEnvOut {
  size_t rec, hash, bits, ends, back, status, total;
};
RawEnvOut raw_env_out(size_t m) {
  RawEnvOut e;
  e.rec = 0;
  e.hash = (sizeof(env::Rec) * m + 63) & ~(size_t)63;
  e.bits = e.hash + 32 * m;
  e.ends = e.bits + a16(m);
  e.back = e.ends + 2 * sizeof(env::Rec) - e.hash;
  e.status = e.ends + 2 * sizeof(env::Rec);
  e.total = e.status + a16(m);
  return e;
}

// a ledger call's block of a chunk's mt TPraos rows: bits | view rows on the
// device and in pinned memory, where the rows' counter column follows
struct RawLvOut {
  size_t bits, rows, ctr, total;
};
RawLvOut raw_lv_out(size_t mt) {
  RawLvOut l;
  l.bits = 0;
  l.rows = a16(mt);
  l.ctr = l.rows + a16(4 * mt);
  l.total = l.ctr + 8 * mt;
  return l;
}

// a PBFT call's block of a chunk's mb PBFT rows: bits | schedule rows | slots,
// on the device (where a mixed chunk's index list follows) and in pinned memory
struct RawPbOut {
  size_t bits, rows, slot, back, idx, total;
};
RawPbOut raw_pb_out(size_t mb) {
  RawPbOut l;
  l.bits = 0;
  l.rows = a16(mb);
  l.slot = l.rows + a16(4 * mb);
  l.back = l.slot + 8 * mb;
  l.idx = a16(l.back);
  l.total = l.idx + a16(4 * mb);
  return l;
}

// a raw-CBOR knob (knobs.h; 0 = unset) if inside [lo, hi], else the default
size_t knob_size(const std::atomic<size_t>& k, size_t dflt, size_t lo, size_t hi) {
  const size_t v = k.load(std::memory_order_relaxed);
  return v && v >= lo && v <= hi ? v : dflt;
}

// Headers in chunk j when `left` headers (this chunk's included) remain.
// ramp (OURO_CBOR_RAMP=1, A/B): the first chunks a quarter and a half of
// `per`, so the first kernel starts after a short gather and upload, and the
// last ones halving down to a quarter, so the chip is not left running one
// full chunk's kernel alone at the end.  It lost: 77.5 -> 85.3 ms per 1M
// headers (profiles/r05o/cbor_ramp_ab.jsonl) -- a small chunk's kernel runs
// at a fraction of the chip with nothing beside it; off by default.
size_t raw_chunk_target(size_t j, size_t left, size_t per, bool ramp) {
  if (!ramp) return per;
  size_t t = j == 0 ? per / 4 : (j == 1 ? per / 2 : per);
  if (left <= per + per / 2) t = std::min(t, std::max(per / 4, left / 2));
  return std::max<size_t>(t, 256);
}

// The chunks of a call, and on the way every span inside raw (as
// ouro_tpraos_pack_cbor demands) unless the entry has checked them: one pass
// over off / len per call either way.
int raw_chunks(const RawCall& c, size_t per, std::vector<RawChunk>* out) {
  out->clear();
  const bool ramp = ouro_knobs::get().cbor_ramp.load(std::memory_order_relaxed) == 1;
  // (locals: the loop runs once per header, and *out growing may not alias them)
  const bool check = !c.spans_checked;
  const size_t n = c.n, raw_bytes = c.raw_bytes;
  const uint64_t* off = c.off;
  const uint32_t* len = c.len;
  RawChunk k{0, 0, 0};
  size_t target = raw_chunk_target(0, n, per, ramp);
  for (size_t i = 0; i < n; i++) {
    if (check && !span_inside(raw_bytes, off[i], len[i])) return span_fail("header", "raw_bytes", i);
    if (k.m && (k.m >= target || k.bytes + len[i] > kRawChunkBytes)) {
      out->push_back(k);
      k = RawChunk{i, 0, 0};
      target = raw_chunk_target(out->size(), n - i, per, ramp);
    }
    k.m++;
    k.bytes += len[i];
  }
  if (k.m) out->push_back(k);
  return OURO_OK;
}


// last call's phases on this thread (ouro_debug_cbor_stats)
thread_local double t_raw_stats[6] = {-1, -1, -1, -1, -1, -1};

int pinned_at_least(uint8_t** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return OURO_OK;
  if (*p) OURO_HIP(hipHostFree(*p));
  *p = nullptr;
  *cap = 0;
  // (hipHostMallocNumaUser: the calling thread's NUMA policy -- a bench rank
  // or multi-device worker is bound to its GPU's node, numa.cpp)
  OURO_HIP(hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocNumaUser));
  *cap = bytes;
  return OURO_OK;
}

// the chunk's header spans from the caller's buffer into the slot's pinned block
int raw_stage(RawSlot& s, const RawCall& c, const RawChunk& k, int width) {
  const bool alphas = c.ea != nullptr;
  const bool chain = c.kind == kRawChain;
  const RawIn L = raw_in(k.m, k.bytes, alphas, c.epochs_bytes);
  const size_t in_bytes = c.env ? L.total_env : L.total;
  int rc = pinned_at_least(&s.h_in, &s.h_in_cap, in_bytes + in_bytes / 8);
  if (rc) return rc;
  uint64_t* noff = reinterpret_cast<uint64_t*>(s.h_in + L.off);
  uint64_t at = 0;
  for (size_t i = 0; i < k.m; i++) {
    noff[i] = at;
    at += c.len[k.lo + i];
  }
  memcpy(s.h_in + L.len, c.len + k.lo, 4 * k.m);
  if (c.eta0) memcpy(s.h_in + L.eta0, c.eta0, 32);
  if (c.epochs) memcpy(s.h_in + L.tab, c.epochs, c.epochs_bytes);
  if (alphas) {
    memcpy(s.h_in + L.alpha, c.ea + 32 * k.lo, 32 * k.m);
    memcpy(s.h_in + L.alpha + 32 * k.m, c.la + 32 * k.lo, 32 * k.m);
  }
  uint8_t* dst = s.h_in + L.raw;
  // tasks of ~1 MB: enough to balance, few enough to keep each memcpy long
  const size_t ntasks = std::max<size_t>(1, std::min<size_t>(k.m, k.bytes >> 20));
  const int r = ouro_pool::parallel_for(ntasks, width, [&](size_t t) {
    const size_t a = k.m * t / ntasks, b = k.m * (t + 1) / ntasks;
    for (size_t i = a; i < b;) {
      // a run of headers adjacent in the caller's buffer: one memcpy
      const uint64_t src = c.off[k.lo + i];
      uint64_t bytes = c.len[k.lo + i];
      size_t j = i + 1;
      while (j < b && c.off[k.lo + j] == src + bytes) bytes += c.len[k.lo + j++];
      memcpy(dst + noff[i], c.raw + src, bytes);
      // the combined entry: each header's era from the bytes just copied
      // (in cache; no pass of its own over the caller's buffer)
      if (chain)
        for (size_t q = i; q < j; q++)
          c.proto[k.lo + q] = (uint8_t)cbor::era_class(dst + noff[q], c.len[k.lo + q]);
      i = j;
    }
  });
  if (r) return fail(OURO_EDEVICE, "raw CBOR gather failed");
  s.mode = c.kind == kRawByron ? kModeByron : kModeTpraos;
  s.mt = k.m;
  if (!chain) return OURO_OK;
  const uint8_t* pr = c.proto + k.lo;
  size_t mt = 0;
  for (size_t i = 0; i < k.m; i++) mt += pr[i] == OURO_PROTO_TPRAOS;
  s.mt = mt;
  if (mt == k.m) return OURO_OK;  // one era: that era's path, unchanged
  if (mt == 0) {
    s.mode = kModeByron;
    return OURO_OK;
  }
  // A mixed chunk.  The bytes stay where the gather put them; the offset and
  // length lists are reordered by class -- the TPraos headers' entries first,
  // then the PBFT headers', each class in the caller's order -- so each
  // slicer runs over one contiguous list, and idx says where a class's row
  // belongs in the caller's arrays.
  s.mode = kModeMixed;
  std::vector<uint64_t> o2;
  try {  // (no exception crosses the C ABI)
    s.idx.resize(k.m);
    o2.resize(k.m);
  } catch (const std::bad_alloc&) {
    return fail(OURO_EDEVICE, "raw CBOR gather: out of host memory");
  }
  if (c.env) {  // the caller's order, before the lists are reordered
    memcpy(s.h_in + L.eoff, noff, 8 * k.m);
    memcpy(s.h_in + L.elen, c.len + k.lo, 4 * k.m);
  }
  size_t at_t = 0, at_b = mt;
  for (size_t i = 0; i < k.m; i++) {
    const size_t j = pr[i] == OURO_PROTO_TPRAOS ? at_t++ : at_b++;
    s.idx[j] = (uint32_t)i;
    o2[j] = noff[i];
  }
  memcpy(noff, o2.data(), 8 * k.m);
  uint32_t* nlen = reinterpret_cast<uint32_t*>(s.h_in + L.len);
  for (size_t j = 0; j < k.m; j++) nlen[j] = c.len[k.lo + s.idx[j]];
  if (alphas)
    for (size_t j = 0; j < mt; j++) {
      memcpy(s.h_in + L.alpha + 32 * j, c.ea + 32 * (k.lo + s.idx[j]), 32);
      memcpy(s.h_in + L.alpha + 32 * k.m + 32 * j, c.la + 32 * (k.lo + s.idx[j]), 32);
    }
  return OURO_OK;
}

// the Byron slicer into `arena`, then the Ed25519 kernel with ByronDSIGN
// acceptance (cardano-crypto: SURVEY.md App. B.5), over the mb headers the
// lists doff / dlen address inside the chunk's raw bytes
int raw_launch_byron(RawSlot& s, const RawCall& c, const uint8_t* draw, size_t raw_bytes,
                     const uint64_t* doff, const uint32_t* dlen, size_t mb, uint8_t* arena,
                     uint8_t* dstatus, uint8_t* dverdict) {
  const size_t blocks = std::min<size_t>((mb + kBlock - 1) / kBlock, 4096);
  const cbor::ByronLayout bl = cbor::byron_layout(mb, raw_bytes + cbor::kByronMsgExtra * mb);
  const cbor::ByronOut o = cbor::byron_arena_out(arena, bl);
  launch_byron_pack(s.st, (unsigned)blocks, draw, raw_bytes, doff, dlen, mb, c.magic, o, dstatus);
  int rc;
  if ((rc = launch_check())) return rc;
  return launch_ed(s.st, mb, o.pk, o.sig, o.msg, o.msg_off, o.msg_len, dverdict, 1);
}

// the TPraos slicer into `arena`, then the header kernel (or the Sum6KES
// kernel, for integrity) over the mt headers of the lists doff / dlen;
// results into the RawOut block at dout.  dea / dla: the explicit VRF inputs
// of those headers, or null: mkSeed from the sliced slots under the epoch
// schedule dtab, else under deta0 (null: NeutralNonce)
int raw_launch_tpraos(RawSlot& s, const RawCall& c, const uint8_t* draw, size_t raw_bytes,
                      const uint64_t* doff, const uint32_t* dlen, size_t mt, uint8_t* arena,
                      uint8_t* dout, const uint8_t* dea, const uint8_t* dla,
                      const uint8_t* deta0, const uint8_t* dtab) {
  const RawOut O = raw_out(mt);
  const size_t blocks = std::min<size_t>((mt + kBlock - 1) / kBlock, 4096);
  uint64_t* dslot = reinterpret_cast<uint64_t*>(dout + O.slot);
  const bool seeds = c.kind != kRawKes && !dea;
  // (a ledger call needs the slots whatever seeds the VRF inputs)
  const cbor::Out o = cbor::arena_out(arena, mt, seeds || c.ledger ? dslot : nullptr, nullptr);
  launch_tpraos_pack(s.st, (unsigned)blocks, draw, raw_bytes, doff, dlen, mt, c.spkp, o,
                     dout + O.status);
  int rc;
  if ((rc = launch_check())) return rc;
  ouro_tpraos_batch b{};
  cbor::batch_from(&b, o, draw, mt);
  if (c.kind == kRawKes)
    return launch_kes(s.st, mt, b.hot_vk, b.kes_t, b.body, b.body_off, b.body_len, b.kes_sig,
                      dout + O.verdict);
  if (dea) {
    b.eta_alpha = dea;
    b.leader_alpha = dla;
  } else {
    b.slot = dslot;
    b.epoch_nonce = deta0;
  }
  if (c.nonce) b.eta_nonce = dout + O.nonce;
  if ((rc = launch_hdr(s.st, b, dout + O.verdict, dout + O.be, dout + O.bl, dea ? nullptr : dtab)) ||
      !c.ledger)
    return rc;
  // the ledger-view checks behind the header kernel, on the same stream, over
  // the rows already in the arena; the views were uploaded once for the call
  const RawLvOut LO = raw_lv_out(mt);
  if ((rc = ensure(s.d_lv, LO.ctr)) || (rc = pinned_at_least(&s.h_lv, &s.h_lv_cap, LO.total)))
    return rc;
  uint8_t* dlv = static_cast<uint8_t*>(s.d_lv.p);
  OURO_HIP(hipStreamWaitEvent(s.st, c.ledger->uploaded, 0));
  if ((rc = lv_launch(s.st, mt, b.issuer_vk, b.vrf_vk, dslot, b.leader_output, b.ocert_kes_period,
                      c.ledger->dviews, c.ledger->g,
                      c.ledger->genesis ? &c.ledger->dgenesis : nullptr, dlv + LO.bits,
                      reinterpret_cast<uint32_t*>(dlv + LO.rows))))
    return rc;
  OURO_HIP(hipMemcpyAsync(s.h_lv, dlv, LO.ctr, hipMemcpyDeviceToHost, s.st));
  OURO_HIP(hipMemcpyAsync(s.h_lv + LO.ctr, b.ocert_counter, 8 * mt, hipMemcpyDeviceToHost, s.st));
  return OURO_OK;
}

// a drained chunk's ledger results into the caller's order, then the counter
// fold over them in that order (idx: a mixed chunk's TPraos rows' indices,
// ascending, or null: row j is header j)
void raw_drain_ledger(const RawSlot& s, const RawCall& c, size_t mt, const uint32_t* idx,
                      const uint8_t* status) {
  RawLedger& L = *c.ledger;
  memset(L.ledger + s.lo, 0, s.m);
  for (size_t i = 0; i < s.m; i++) L.pool_row[s.lo + i] = OURO_LV_NO_POOL;
  const RawLvOut LO = raw_lv_out(mt);
  const uint8_t* bits = s.h_lv + LO.bits;
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(s.h_lv + LO.rows);
  const uint64_t* ctr = reinterpret_cast<const uint64_t*>(s.h_lv + LO.ctr);
  for (size_t j = 0; j < mt; j++) {
    if (status[j] != OURO_PACK_OK) continue;  // (its zeroed row says nothing)
    const size_t i = s.lo + (idx ? idx[j] : j);
    L.ledger[i] = bits[j];
    L.pool_row[i] = rows[j];
    if (L.fold) lv_fold_run(L.fold, 1, &rows[j], &ctr[j], &L.ledger[i]);
  }
}

// a drained chunk's PBFT results into the caller's order, then the window fold
// over them in that order (idx: a mixed chunk's PBFT rows' indices, ascending,
// or null: row j is header j); status: the Byron slicer's, per row
void raw_drain_pbft(const RawSlot& s, const RawCall& c, size_t mb, const uint32_t* idx,
                    const uint8_t* status) {
  RawPbft& B = *c.pbft;
  memset(B.pbft + s.lo, 0, s.m);
  for (size_t i = 0; i < s.m; i++) B.genesis_row[s.lo + i] = OURO_LV_NO_POOL;
  if (B.signed_count) memset(B.signed_count + s.lo, 0, 8 * s.m);
  const RawPbOut PO = raw_pb_out(mb);
  const uint8_t* bits = s.h_pb + PO.bits;
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(s.h_pb + PO.rows);
  const uint64_t* slot = reinterpret_cast<const uint64_t*>(s.h_pb + PO.slot);
  for (size_t j = 0; j < mb; j++) {
    if (status[j] != OURO_PACK_OK && status[j] != OURO_PACK_EBB) continue;
    const size_t i = s.lo + (idx ? idx[j] : j);
    B.pbft[i] = bits[j];
    B.genesis_row[i] = rows[j];
    if (B.fold)
      pbft_fold_run(B.fold, 1, &rows[j], &slot[j], &B.pbft[i],
                    B.signed_count ? &B.signed_count[i] : nullptr);
  }
}

// the slot's stream: upload, device slicer(s), kernel(s), results back
int raw_launch(RawSlot& s, const RawCall& c, const RawChunk& k) {
  const bool alphas = c.ea != nullptr;
  const RawIn L = raw_in(k.m, k.bytes, alphas, c.epochs_bytes);
  const size_t mt = s.mode == kModeByron ? 0 : s.mt, mb = k.m - mt;
  const RawOut O = raw_out(mt ? mt : k.m);
  const RawOutB OB = raw_out_b(mb);
  // bytes copied back: one era's block, or a mixed chunk's two
  const size_t back = mt ? raw_out_bytes(c, O, mt) : O.verdict + k.m;
  const size_t back_b = s.mode == kModeMixed ? OB.verdict + mb : 0;
  const size_t arena_t = !mt ? 0
                         : c.kind == kRawBlock ? a16(ouro_block_pack_bytes(mt)) + 64
                                               : a16(ouro_tpraos_pack_bytes(mt)) + 64;
  const cbor::ByronLayout bl = cbor::byron_layout(mb, k.bytes + cbor::kByronMsgExtra * mb);
  const bool env_lists = c.env && s.mode == kModeMixed;
  const size_t up = env_lists ? L.total_env : L.total;
  const RawEnvOut EO = raw_env_out(k.m);
  int rc;
  if (c.env && ((rc = ensure(s.d_env, EO.total + 64)) ||
                (rc = pinned_at_least(&s.h_env, &s.h_env_cap, EO.back))))
    return rc;
  if ((rc = ensure(s.d_in, up)) ||
      (rc = ensure(s.d_arena, arena_t + (mb ? bl.total + 64 : 0))) ||
      (rc = ensure(s.d_out, a16(O.total) + (back_b ? OB.total : 0))) ||
      (rc = pinned_at_least(&s.h_out, &s.h_out_cap, a16(back) + back_b)))
    return rc;
  uint8_t* din = static_cast<uint8_t*>(s.d_in.p);
  uint8_t* dout = static_cast<uint8_t*>(s.d_out.p);
  uint8_t* darena = static_cast<uint8_t*>(s.d_arena.p);
  OURO_HIP(hipMemcpyAsync(din, s.h_in, up, hipMemcpyHostToDevice, s.st));
  const uint8_t* draw = din + L.raw;
  const uint64_t* doff = reinterpret_cast<const uint64_t*>(din + L.off);
  const uint32_t* dlen = reinterpret_cast<const uint32_t*>(din + L.len);
  if (s.mode == kModeByron) {
    // (a one-era chunk: status | verdict where the TPraos block has them)
    if ((rc = raw_launch_byron(s, c, draw, k.bytes, doff, dlen, k.m, cbor::arena_base(darena),
                               dout + O.status, dout + O.verdict)))
      return rc;
  } else if (c.kind == kRawBlock) {
    // whole blocks: slicer, segment hashes, Sum6KES and the finish (block_api.cpp)
    if ((rc = block_launch(s.st, draw, k.bytes, doff, dlen, mt, c.spkp, cbor::arena_base(darena),
                           dout + O.status, dout + O.verdict,
                           c.body_hash ? dout + O.be : nullptr)))
      return rc;
  } else {
    if ((rc = raw_launch_tpraos(s, c, draw, k.bytes, doff, dlen, mt, cbor::arena_base(darena),
                                dout, alphas ? din + L.alpha : nullptr,
                                alphas ? din + L.alpha + 32 * k.m : nullptr,
                                c.eta0 ? din + L.eta0 : nullptr,
                                c.epochs ? din + L.tab : nullptr)))
      return rc;
    // a mixed chunk: its PBFT headers from the same uploaded bytes, through
    // the tail of the lists, on the same stream
    if (mb && (rc = raw_launch_byron(s, c, draw, k.bytes, doff + mt, dlen + mt, mb,
                                     cbor::arena_base(darena + arena_t), dout + a16(O.total),
                                     dout + a16(O.total) + OB.verdict)))
      return rc;
  }
  if (c.env) {
    // the envelope on the same stream over the bytes already uploaded, in the
    // caller's order whatever the chunk's era make-up; its first header is
    // linked on the host when the chunk before it has drained (raw_drain)
    uint8_t* de = cbor::arena_base(s.d_env.p);
    const uint64_t* eoff = env_lists ? reinterpret_cast<const uint64_t*>(din + L.eoff) : doff;
    const uint32_t* elen = env_lists ? reinterpret_cast<const uint32_t*>(din + L.elen) : dlen;
    if ((rc = launch_envelope(s.st, draw, k.bytes, eoff, elen, k.m, c.env->cfg, c.env->tip,
                              reinterpret_cast<env::Rec*>(de + EO.rec), de + EO.status,
                              de + EO.hash, de + EO.bits, nullptr,
                              reinterpret_cast<env::Rec*>(de + EO.ends))))
      return rc;
    OURO_HIP(hipMemcpyAsync(s.h_env, de + EO.hash, EO.back, hipMemcpyDeviceToHost, s.st));
    // the Byron ledger-view checks behind the Byron slicer and the envelope
    // slicer, on the same stream: the rows' delegate keys and statuses lie in
    // the slot's arena and result block, their slots in the envelope records
    // (a mixed chunk's through the index list of its PBFT rows)
    if (c.pbft && mb) {
      const RawPbOut PO = raw_pb_out(mb);
      if ((rc = ensure(s.d_pb, PO.total)) || (rc = pinned_at_least(&s.h_pb, &s.h_pb_cap, PO.back)))
        return rc;
      uint8_t* dpb = static_cast<uint8_t*>(s.d_pb.p);
      const bool mixed = s.mode == kModeMixed;
      uint8_t* barena = cbor::arena_base(mixed ? darena + arena_t : darena);
      const cbor::ByronOut bo = cbor::byron_arena_out(barena, bl);
      const uint8_t* bstatus = mixed ? dout + a16(O.total) : dout + O.status;
      const uint32_t* didx = nullptr;
      if (mixed) {
        OURO_HIP(hipMemcpyAsync(dpb + PO.idx, s.idx.data() + mt, 4 * mb, hipMemcpyHostToDevice,
                                s.st));
        didx = reinterpret_cast<const uint32_t*>(dpb + PO.idx);
      }
      OURO_HIP(hipStreamWaitEvent(s.st, c.ledger->uploaded, 0));
      if ((rc = launch_pbft_chain(s.st, mb, bo.delegate_vk, bstatus, de + EO.rec, didx,
                                  c.pbft->dviews, dpb + PO.bits,
                                  reinterpret_cast<uint32_t*>(dpb + PO.rows),
                                  reinterpret_cast<uint64_t*>(dpb + PO.slot))))
        return rc;
      OURO_HIP(hipMemcpyAsync(s.h_pb, dpb, PO.back, hipMemcpyDeviceToHost, s.st));
    }
  }
  OURO_HIP(hipMemcpyAsync(s.h_out, dout, back, hipMemcpyDeviceToHost, s.st));
  if (back_b)
    OURO_HIP(hipMemcpyAsync(s.h_out + a16(back), dout + a16(O.total), back_b,
                            hipMemcpyDeviceToHost, s.st));
  OURO_HIP(hipEventRecord(s.done, s.st));
  s.lo = k.lo;
  s.m = k.m;
  s.busy = true;
  return OURO_OK;
}

// the slot's finished chunk into the caller's buffers
int raw_drain(RawSlot& s, const RawCall& c) {
  if (!s.busy) return OURO_OK;
  s.busy = false;
  OURO_HIP(hipEventSynchronize(s.done));
  if (c.env) {
    // chunks drain in order: this chunk's first header on top of the last
    // record of the one before it (or the tip), with the kernels' own rule
    const RawEnvOut EO = raw_env_out(s.m);
    const uint8_t* h = s.h_env;  // (the block from its hashes on)
    memcpy(c.env->hash + 32 * s.lo, h, 32 * s.m);
    memcpy(c.env->envelope + s.lo, h + (EO.bits - EO.hash), s.m);
    env::Rec ends[2];
    memcpy(ends, h + (EO.ends - EO.hash), sizeof ends);
    c.env->envelope[s.lo] = env::envelope_link(c.env->prev, ends[0], c.env->cfg);
    c.env->prev = ends[1];
  }
  const bool hdr = c.kind == kRawHdr || c.kind == kRawChain;
  if (s.mode == kModeMixed) {
    // both result sets back to the caller's order (RawSlot idx: the TPraos
    // rows' indices, then the PBFT rows')
    const size_t mt = s.mt, mb = s.m - mt;
    const RawOut O = raw_out(mt);
    const RawOutB OB = raw_out_b(mb);
    const uint8_t* h = s.h_out;
    if (c.ledger) raw_drain_ledger(s, c, mt, s.idx.data(), h + O.status);
    for (size_t j = 0; j < mt; j++) {
      const size_t i = s.lo + s.idx[j];
      const uint8_t st = h[O.status + j];
      c.status[i] = st;
      c.verdict[i] = st == OURO_PACK_OK ? h[O.verdict + j] : 0;
      if (c.be) memcpy(c.be + 64 * i, h + O.be + 64 * j, 64);
      if (c.bl) memcpy(c.bl + 64 * i, h + O.bl + 64 * j, 64);
      if (c.nonce) memcpy(c.nonce + 32 * i, h + O.nonce + 32 * j, 32);
    }
    const uint8_t* hb = s.h_out + a16(raw_out_bytes(c, O, mt));
    if (c.pbft) raw_drain_pbft(s, c, mb, s.idx.data() + mt, hb + OB.status);
    for (size_t j = 0; j < mb; j++) {
      const size_t i = s.lo + s.idx[mt + j];
      const uint8_t st = hb[OB.status + j];
      c.status[i] = st;
      c.verdict[i] = st == OURO_PACK_EBB ? 1 : (st == OURO_PACK_OK && hb[OB.verdict + j] ? 1 : 0);
      if (c.be) memset(c.be + 64 * i, 0, 64);
      if (c.bl) memset(c.bl + 64 * i, 0, 64);
      if (c.nonce) memset(c.nonce + 32 * i, 0, 32);
    }
    return OURO_OK;
  }
  const RawOut O = raw_out(s.m);
  const uint8_t* st = s.h_out + O.status;
  const uint8_t* v = s.h_out + O.verdict;
  memcpy(c.status + s.lo, st, s.m);
  if (s.mode == kModeByron) {
    // PBFT accepts an epoch-boundary header without a signature
    // (ouroboros-consensus/src/Ouroboros/Consensus/Protocol/PBFT.hs:327-328)
    for (size_t i = 0; i < s.m; i++)
      c.verdict[s.lo + i] = st[i] == OURO_PACK_EBB ? 1 : (st[i] == OURO_PACK_OK && v[i] ? 1 : 0);
    if (c.ledger) raw_drain_ledger(s, c, 0, nullptr, st);
    if (c.pbft) raw_drain_pbft(s, c, s.m, nullptr, st);
    if (hdr) {  // the combined entry: a PBFT header has no VRF outputs
      if (c.be) memset(c.be + 64 * s.lo, 0, 64 * s.m);
      if (c.bl) memset(c.bl + 64 * s.lo, 0, 64 * s.m);
      if (c.nonce) memset(c.nonce + 32 * s.lo, 0, 32 * s.m);
    }
    return OURO_OK;
  }
  // a header the slicer rejected is invalid (its zeroed row cannot verify;
  // masked so that no bit at all is set for it)
  for (size_t i = 0; i < s.m; i++) c.verdict[s.lo + i] = st[i] == OURO_PACK_OK ? v[i] : 0;
  if (c.kind == kRawBlock && c.body_hash) memcpy(c.body_hash + 32 * s.lo, s.h_out + O.be, 32 * s.m);
  if (c.ledger) raw_drain_ledger(s, c, s.m, nullptr, st);
  if (c.pbft) raw_drain_pbft(s, c, 0, nullptr, st);
  if (hdr) {
    if (c.be) memcpy(c.be + 64 * s.lo, s.h_out + O.be, 64 * s.m);
    if (c.bl) memcpy(c.bl + 64 * s.lo, s.h_out + O.bl, 64 * s.m);
    if (c.nonce) memcpy(c.nonce + 32 * s.lo, s.h_out + O.nonce, 32 * s.m);
  }
  return OURO_OK;
}

int raw_run(const RawCall& c, const std::vector<RawChunk>& chunks) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  double gather_ms = 0, wait_ms = 0;
  DeviceState* ds;
  int dev, rc = device_state(&ds);
  if (rc || (rc = current_device(&dev))) return rc;
  RawPipe& p = ctx_of(dev).raw;
  // chunks in flight: the header kernel wants ~3 grids of work queued (6 x
  // 64 K headers); the Sum6KES kernel is PCIe-bound, 4 suffice
  // (profiles/r05a/cbor_sweep.jsonl); Byron's Ed25519 runs best with 5
  // (66.7--67.1 M headers/s against ~61 with 4 and 60--68 with 6, interleaved
  // on one box: profiles/r06k/byron_ab.jsonl)
  // (the combined entry: the header kernel's count)
  const bool hdr_kind = c.kind == kRawHdr || c.kind == kRawChain;
  const int S = (int)knob_size(ouro_knobs::get().cbor_slots, hdr_kind ? 6 : (c.kind == kRawByron ? 5 : 4), 1,
                                kRawMaxSlots);
  for (int k = 0; k < S; k++) {
    RawSlot& s = p.s[k];
    if (!s.st) OURO_HIP(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
    if (!s.done) OURO_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  const int width = (int)knob_size(ouro_knobs::get().cbor_copy_threads, 8, 1, 64);
  if (c.env) c.env->prev = c.env->tip;
  if (c.ledger) {
    c.ledger->fold_begin();
    // the views (and the genesis delegations, in the same block) once per
    // call, on the first slot's stream; every chunk's stream waits on the
    // upload before its ledger kernel
    if (!p.views_up) OURO_HIP(hipEventCreateWithFlags(&p.views_up, hipEventDisableTiming));
    if ((rc = lv_upload(p.s[0].st, *c.ledger->views, c.ledger->genesis, &p.d_views,
                        &c.ledger->packed, &c.ledger->dviews, &c.ledger->dgenesis)))
      return rc;
    // (the delegation schedule of a PBFT call on the same stream, before the event)
    if (c.pbft) {
      c.pbft->fold_begin();
      if ((rc = pbft_upload(p.s[0].st, *c.pbft->views, &p.d_pviews, &c.pbft->packed,
                            &c.pbft->dviews)))
        return rc;
    }
    OURO_HIP(hipEventRecord(p.views_up, p.s[0].st));
    c.ledger->uploaded = p.views_up;
  }
  size_t ci = 0;
  for (; ci < chunks.size() && !rc; ci++) {
    RawSlot& s = p.s[ci % S];
    const auto a = clk::now();
    rc = raw_drain(s, c);
    const auto b = clk::now();
    if (!rc) rc = raw_stage(s, c, chunks[ci], width);
    const auto d = clk::now();
    if (!rc) rc = raw_launch(s, c, chunks[ci]);
    wait_ms += std::chrono::duration<double, std::milli>(b - a).count();
    gather_ms += std::chrono::duration<double, std::milli>(d - b).count();
  }
  // the rest in chunk order; after an error, wait for everything in flight
  for (int k = 0; k < S; k++) {
    RawSlot& s = p.s[(ci + k) % S];
    if (rc) {
      (void)hipStreamSynchronize(s.st);
      s.busy = false;
    } else {
      const auto a = clk::now();
      rc = raw_drain(s, c);
      wait_ms += std::chrono::duration<double, std::milli>(clk::now() - a).count();
    }
  }
  const double total = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  const double st[6] = {total, gather_ms, wait_ms, (double)chunks.size(), (double)S, (double)width};
  memcpy(t_raw_stats, st, sizeof st);
  if (!rc && c.env && c.env->tip_out) env::tip_of_rec(c.env->tip_out, c.env->prev);
  return rc;
}

}  // namespace

namespace ouro_rt {
int raw_check(const RawCall& c) {
  if (!c.raw || !c.off || !c.len || !c.status || !c.verdict)
    return fail(OURO_EINVAL, "null argument");
  if (c.kind == kRawChain && !c.proto) return fail(OURO_EINVAL, "null proto");
  if (c.kind != kRawByron && c.spkp == 0) return fail(OURO_EINVAL, "zero slots per KES period");
  if ((c.kind == kRawByron || c.kind == kRawChain) &&
      (c.magic < -1 || c.magic > (int64_t)0xffffffffll))
    return fail(OURO_EINVAL, "protocol magic outside Word32 (or -1)");
  if ((c.ea == nullptr) != (c.la == nullptr))
    return fail(OURO_EINVAL, "give both VRF input arrays or neither");
  if (c.ea && c.epochs)
    return fail(OURO_EINVAL, "give an epoch schedule or the VRF input arrays, not both");
  return OURO_OK;
}

int raw_verify_host(const RawCall& c) {
  if (c.n == 0) return OURO_OK;
  if (int rc = raw_check(c)) return rc;
  // every span before any output is written
  if (!c.spans_checked)
    if (int rc = spans_check("header", "raw_bytes", c.raw_bytes, c.off, c.len, c.n)) return rc;
  return raw_host(c);
}

int raw_verify(const RawCall& c) {
  if (c.n == 0) return OURO_OK;
  if (int rc0 = raw_check(c)) return rc0;
  std::vector<RawChunk> chunks;
  const size_t per = knob_size(ouro_knobs::get().cbor_chunk, 65536, 256, (size_t)1 << 24);
  int rc = raw_chunks(c, per, &chunks);
  if (rc) return rc;
  return or_host(raw_run(c, chunks), [&] { return raw_host(c); });
}
}  // namespace ouro_rt

extern "C" {
// DIAGNOSTIC: the calling thread's last raw-CBOR call (ms and counts)
int ouro_debug_cbor_stats(double* out6) {
  if (!out6) return fail(OURO_EINVAL, "null buffer");
  memcpy(out6, t_raw_stats, sizeof t_raw_stats);
  return OURO_OK;
}
}  // extern "C"
