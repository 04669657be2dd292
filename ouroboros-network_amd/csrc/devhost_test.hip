// devhost_test.hip -- TEST-ONLY host build of the kernels' lane routines.
//
// hipcc compiles the __host__ __device__ bodies in verify.h for x86 too; this
// library exports them so tests/test_devcode_host.py can check the exact
// arithmetic the gfx950 kernels run against the oracle and libsodium in a
// container with no GPU.  It is never linked into, or loaded by, the product
// library (lib/libouro_verify.so) and launches nothing.
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <vector>

#include "blake2b_stream.h"
#include "lane_items.h"
#include "leader.h"
#include "ledger_view.h"
#include "pbft_view.h"
#include "prove.h"
#include "tpraos.h"
#include "wide_cores.h"

using namespace ouro;

#if defined(OURO_COUNT_OPS)
thread_local unsigned long long g_ouro_nmul = 0, g_ouro_nsq = 0, g_ouro_bound_violations = 0;

// bound tracker hooks (fe25519.h): shadow bounds of elements stored in memory
#include <array>
#include <unordered_map>
namespace {
thread_local std::unordered_map<const void*, std::array<uint64_t, 10>> g_shadow;
thread_local unsigned long long g_untracked_loads = 0;
}
void ouro_trk_violation() {
  ++g_ouro_bound_violations;
  static const bool do_abort = getenv("OURO_TRK_ABORT") != nullptr;
  if (do_abort) abort();
}
void ouro_trk_store(const void* p, const uint64_t b[10]) {
  std::array<uint64_t, 10> a;
  for (int i = 0; i < 10; i++) a[i] = b[i];
  g_shadow[p] = a;
}
void ouro_trk_load(const void* p, uint64_t b[10]) {
  auto it = g_shadow.find(p);
  if (it == g_shadow.end()) {
    // never stored through st_fe/st_cached: only possible for memory the
    // tracker did not see being written -- assume the worst 32-bit value
    ++g_untracked_loads;
    for (int i = 0; i < 10; i++) b[i] = 0xffffffffu;
    return;
  }
  for (int i = 0; i < 10; i++) b[i] = it->second[i];
}
#endif

namespace {
const int32_t* host_btab() {
  static std::vector<int32_t> tab = [] {
    std::vector<int32_t> t(kBTabWords);
    build_btab(t.data());
    return t;
  }();
  return tab.data();
}
// one slot (column 0) of a kSlotGroup-slot region, laid out as on the device
struct SlotRegion {
  std::vector<int32_t> buf;
  Slot s;
  explicit SlotRegion(int slot_words) : buf(slot_region_words(1, slot_words) + 4, 0) {
    s = Slot{reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~uintptr_t(15))};
  }
};
struct Lane : SlotRegion {
  Lane() : SlotRegion(kLaneWords) {}
};
fe fe_from_bytes(const uint8_t* b) {
  uint32_t w[8];
  bytes_to_words8(w, b);
  return fe_from_words(w);
}
void fe_to_bytes(uint8_t* out, const fe& f) {
  uint32_t w[8];
  fe_to_words(w, f);
  memcpy(out, w, 32);
}
// the fixed-record items of lane_items.h in a host loop
template <int kOp>
int lt_host_op(int op, int n, const uint32_t* in, uint32_t* out, int param) {
  if (op == kOp) {
    for (int i = 0; i < n; i++) lt::item<kOp>(in + (size_t)i * lt::kIn, out + (size_t)i * lt::kOut, param);
    return 0;
  }
  if constexpr (kOp + 1 < lt::kOps) return lt_host_op<kOp + 1>(op, n, in, out, param);
  return -1;
}
}  // namespace

extern "C" {

// field-operation counters (valid when built with -DOURO_COUNT_OPS)
void dh_count_reset(void) {
#if defined(OURO_COUNT_OPS)
  g_ouro_nmul = g_ouro_nsq = 0;
#endif
}
unsigned long long dh_bound_violations(void) {
#if defined(OURO_COUNT_OPS)
  return g_ouro_bound_violations;
#else
  return ~0ull;
#endif
}
void dh_count_get(unsigned long long* nmul, unsigned long long* nsq) {
#if defined(OURO_COUNT_OPS)
  *nmul = g_ouro_nmul;
  *nsq = g_ouro_nsq;
#else
  *nmul = *nsq = 0;
#endif
}

// field ops on canonical 32-byte encodings
void dh_fe_mul(uint8_t* out, const uint8_t* a, const uint8_t* b) {
  fe_to_bytes(out, fe_mul(fe_from_bytes(a), fe_from_bytes(b)));
}
void dh_fe_sq(uint8_t* out, const uint8_t* a) { fe_to_bytes(out, fe_sq(fe_from_bytes(a))); }
void dh_fe_sub(uint8_t* out, const uint8_t* a, const uint8_t* b) {
  fe_to_bytes(out, fe_sub(fe_from_bytes(a), fe_from_bytes(b)));
}
void dh_fe_invert(uint8_t* out, const uint8_t* a) {
  fe_to_bytes(out, fe_invert(fe_from_bytes(a)));
}
void dh_fe_invert_vartime(uint8_t* out, const uint8_t* a) {
  fe_to_bytes(out, fe_invert_vartime(fe_from_bytes(a)));
}
// the same with at most 10 bits cancelled per divstep step (the latency
// mode's wave inversion, wide_inv.h OURO_INV_CAP)
void dh_fe_invert_vartime_cap10(uint8_t* out, const uint8_t* a) {
  fe_to_bytes(out, fe_invert_vartime<10>(fe_from_bytes(a)));
}
void dh_fe_invert_vartime_sel(uint8_t* out, const uint8_t* a) {
  fe_to_bytes(out, fe_invert_vartime<10, true>(fe_from_bytes(a)));
}
void dh_fe_invert_vartime_spec(uint8_t* out, const uint8_t* a) {
  fe_to_bytes(out, fe_invert_vartime<30, true, true>(fe_from_bytes(a)));
}
// the same from raw limbs (< 2^31 each: unreduced representations)
void dh_fe_invert_vartime_limbs(uint8_t* out, const uint32_t* limbs) {
  fe f = fe_make(limbs[0], limbs[1], limbs[2], limbs[3], limbs[4], limbs[5], limbs[6], limbs[7],
                 limbs[8], limbs[9]);
  fe_to_bytes(out, fe_invert_vartime(f));
}
// raw-limb round trip: limbs given as 10 uint32 (< 2^31), canonical encoding out
void dh_fe_limbs_tobytes(uint8_t* out, const uint32_t* limbs) {
  fe f = fe_make(limbs[0], limbs[1], limbs[2], limbs[3], limbs[4], limbs[5], limbs[6], limbs[7],
                 limbs[8], limbs[9]);
  fe_to_bytes(out, f);
}
// a per-lane table coordinate's 256-bit packing (verify.h fe_pack256, limbs
// < 2^28 in) and the limbs its unpacking yields
void dh_fe_pack256(uint32_t* words8, uint32_t* limbs_out, const uint32_t* limbs) {
  fe f = fe_make(limbs[0], limbs[1], limbs[2], limbs[3], limbs[4], limbs[5], limbs[6], limbs[7],
                 limbs[8], limbs[9]);
  fe_pack256(words8, f);
  const fe g = fe_unpack256(words8);
  for (int i = 0; i < 10; i++) limbs_out[i] = g.v[i];
}
unsigned long long dh_untracked_loads(void) {
#if defined(OURO_COUNT_OPS)
  return g_untracked_loads;
#else
  return 0;
#endif
}
void dh_sc_reduce64(uint8_t* out, const uint8_t* in64) {
  uint32_t w[16], r[8];
  for (int i = 0; i < 16; i++) w[i] = ld_le32(in64 + 4 * i);
  sc_reduce512(r, w);
  memcpy(out, r, 32);
}
void dh_sha512_prefixed64(uint8_t* out, const uint8_t* prefix64, const uint8_t* msg,
                          uint32_t mlen) {
  uint32_t pre[16];
  for (int i = 0; i < 16; i++) pre[i] = ld_le32(prefix64 + 4 * i);
  uint64_t H[8];
  sha512_prefixed<64>(H, pre, ShaGlobalTail{msg}, mlen);
  uint32_t w[16];
  sha512_digest_words(w, H);
  memcpy(out, w, 64);
}
void dh_blake2b256_64(uint8_t* out, const uint8_t* in64) {
  uint32_t w[16], h[8];
  for (int i = 0; i < 16; i++) w[i] = ld_le32(in64 + 4 * i);
  blake2b256_64(h, w);
  memcpy(out, h, 32);
}
// the streaming Blake2b-256 (blake2b_stream.h): the host build's memcpy loads
void dh_blake2b256_stream(uint8_t* out, const uint8_t* msg, uint32_t len) {
  uint32_t h[8];
  blake2b256_stream(h, msg, len);
  memcpy(out, h, 32);
}
void dh_blake2b256_96(uint8_t* out, const uint8_t* in96) {
  uint32_t w[24], h[8];
  for (int i = 0; i < 24; i++) w[i] = ld_le32(in96 + 4 * i);
  blake2b256_96(h, w);
  memcpy(out, h, 32);
}
// ... and the same hash through the DEVICE's block loads (b2b_load_dwords:
// aligned dwords funnel-shifted by the span's misalignment) with a loader
// that checks the load rule: every dword read is aligned and holds at least
// one byte of the span msg[0 .. len).  Returns the number of dwords read, or
// -1 on the first read that breaks the rule.
int dh_blake2b256_dwords(uint8_t* out, const uint8_t* msg, uint32_t len) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(msg), e0 = a0 + len;
  int loads = 0;
  bool bad = false;
  auto ld = [&](uintptr_t x) -> uint32_t {
    if ((x & 3) || len == 0 || x + 4 <= a0 || x >= e0) {
      bad = true;
      return 0xdeadbeefu;
    }
    loads++;
    // (only the bytes of the span are the caller's: the rest of the dword
    // comes back as set bits, which the routine must shift or mask away)
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) {
      const uintptr_t b = x + (uintptr_t)k;
      const uint32_t byte = (b >= a0 && b < e0) ? *reinterpret_cast<const uint8_t*>(b) : 0xffu;
      v |= byte << (8 * k);
    }
    return v;
  };
  uint64_t h[8];
  for (int i = 0; i < 8; i++) h[i] = kB2bIV[i];
  h[0] ^= 0x01010000ULL ^ 32;
  uintptr_t p = a0;
  uint32_t left = len;
  uint64_t t = 0;
  for (;;) {
    const bool last = left <= 128;
    const uint32_t take = last ? left : 128u;
    uint64_t m[16];
    b2b_load_dwords(m, p, take, ld);
    t += take;
    b2b_compress(h, m, t, last);
    if (last) break;
    p += take;
    left -= take;
  }
  memcpy(out, h, 32);
  return bad ? -1 : loads;
}
// Blake2b-256 of npre <= 2 prefix bytes (pre: the first in bits 0..7) and a
// span (blake2b_stream.h blake2b256_stream_prefixed): the host build ...
void dh_blake2b256_prefixed(uint8_t* out, uint32_t pre, uint32_t npre, const uint8_t* msg,
                            uint32_t len) {
  uint32_t h[8];
  blake2b256_stream_prefixed(h, pre, npre, msg, len);
  memcpy(out, h, 32);
}
// ... and the same routine (b2b_prefixed_with) through the DEVICE's block
// loads with the rule-checking loader of dh_blake2b256_dwords: the number of
// dwords read, or -1 on the first read that is unaligned or holds no byte of
// msg[0 .. len).
int dh_blake2b256_prefixed_dwords(uint8_t* out, uint32_t pre, uint32_t npre, const uint8_t* msg,
                                  uint32_t len) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(msg), e0 = a0 + len;
  int loads = 0;
  bool bad = false;
  auto ld = [&](uintptr_t x) -> uint32_t {
    if ((x & 3) || len == 0 || x + 4 <= a0 || x >= e0) {
      bad = true;
      return 0xdeadbeefu;
    }
    loads++;
    uint32_t v = 0;  // (bytes outside the span come back as set bits)
    for (int k = 0; k < 4; k++) {
      const uintptr_t b = x + (uintptr_t)k;
      const uint32_t byte = (b >= a0 && b < e0) ? *reinterpret_cast<const uint8_t*>(b) : 0xffu;
      v |= byte << (8 * k);
    }
    return v;
  };
  uint32_t h[8];
  b2b_prefixed_with(h, pre, npre, msg, len, [&](uint64_t m[16], const uint8_t* p, uint32_t take) {
    b2b_load_dwords(m, reinterpret_cast<uintptr_t>(p), take, ld);
  });
  memcpy(out, h, 32);
  return bad ? -1 : loads;
}
void dh_elligator2(uint8_t* out, const uint8_t* r32) {
  uint32_t r[8];
  bytes_to_words8(r, r32);
  r[7] &= 0x7fffffffu;
  ge_p3 H = elligator2_h(r);
  uint32_t enc[8];
  ge_encode_with_inv(enc, H.X, H.Y, fe_invert(H.Z));
  memcpy(out, enc, 32);
}
void dh_elligator2_ref(uint8_t* out, const uint8_t* r32) {
  uint32_t r[8];
  bytes_to_words8(r, r32);
  r[7] &= 0x7fffffffu;
  ge_p3 H = elligator2_h_ref(r);
  uint32_t enc[8];
  ge_encode_with_inv(enc, H.X, H.Y, fe_invert(H.Z));
  memcpy(out, enc, 32);
}
// leader.h: 1 leader, 0 not, -1 outside the supported domain
int dh_leader_check(const uint8_t* beta64, uint64_t num, uint64_t den, uint64_t act_log_lo,
                    int64_t act_log_hi) {
  return leader_check_lane(beta64, num, den, act_log_lo, act_log_hi);
}
// ledger_view.h: the OURO_LV_* bits (COUNTER_OK excepted) of one header row and
// its view row; blake2b.h: Blake2b-224 of 32 bytes
int dh_ledger_check(const ouro_ledger_views* v, const ouro_ledger_globals* g,
                    const uint8_t* issuer_vk, const uint8_t* vrf_vk, uint64_t slot,
                    const uint8_t* leader_output, uint64_t c0, uint32_t* pool_row) {
  return lv::ledger_check_lane(*v, *g, issuer_vk, vrf_vk, slot, leader_output, c0, pool_row);
}
// the same with a genesis-delegation schedule: overlay rows take the delegate
// branch
int dh_ledger_check_overlay(const ouro_ledger_views* v, const ouro_ledger_globals* g,
                            const ouro_genesis_delegs* gd, const uint8_t* issuer_vk,
                            const uint8_t* vrf_vk, uint64_t slot, const uint8_t* leader_output,
                            uint64_t c0, uint32_t* pool_row) {
  return lv::ledger_check_lane<true>(*v, *g, *gd, issuer_vk, vrf_vk, slot, leader_output, c0,
                                     pool_row);
}
// classifyOverlaySlot: -1 not an overlay slot, -2 inactive, else the index of
// the scheduled genesis key
int64_t dh_classify_overlay_slot(uint64_t s, uint64_t num, uint64_t den, uint64_t asc_inv,
                                 uint32_t ngen) {
  uint64_t position;
  if (!lv::overlay_position(s, num, den, &position)) return -1;
  const uint32_t ix = lv::overlay_index(position, asc_inv, ngen);
  return ix == OURO_LV_NO_POOL ? -2 : (int64_t)ix;
}
int dh_is_overlay_slot(uint64_t s, uint64_t num, uint64_t den) {
  return lv::is_overlay_slot(s, num, den) ? 1 : 0;
}
void dh_blake2b224_32(const uint8_t* in32, uint8_t* out28) {
  uint32_t in[16], o[7];
  for (int w = 0; w < 16; w++) in[w] = w < 8 ? ld_le32(in32 + 4 * w) : 0u;
  blake2b224_short(o, in, 32);
  for (int k = 0; k < 28; k++) out28[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
}
// sha3.h: SHA3-256 of a message of len <= 135 bytes (one block); Byron's
// hashKey of a 64-byte XPub; pbft_view.h: the OURO_PBFT_* bits of one row
// (SLOT_OK and WINDOW_OK excepted) and its schedule row
int dh_sha3_256_short(uint8_t* out32, const uint8_t* msg, uint32_t len) {
  if (len > 135) return -1;
  uint8_t blk[136] = {0};
  if (len) memcpy(blk, msg, len);
  uint32_t in[34], o[8];
  for (int w = 0; w < 34; w++) in[w] = ld_le32(blk + 4 * w);
  sha3_256_short(o, in, len);
  for (int k = 0; k < 32; k++) out32[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  return 0;
}
void dh_byron_key_hash(uint8_t* out28, const uint8_t* xpub64) { pbft::key_hash_lane(out28, xpub64); }
int dh_pbft_check(const ouro_pbft_views* v, const uint8_t* delegate_vk, uint64_t slot,
                  uint32_t status, uint32_t* genesis_row) {
  return pbft::pbft_check_lane(*v, delegate_vk, slot, status, genesis_row);
}
// lattice.h: (|c0|, c1, sign of c0) for h (32 bytes, < 2^253); returns the bit size
int dh_half_scalars(const uint8_t* h32, uint8_t* c0, uint8_t* c1, int* c0_neg) {
  uint32_t h[8];
  bytes_to_words8(h, h32);
  HalfScalars hs;
  ed25519_half_scalars(hs, h);
  memcpy(c0, hs.c0, 32);
  memcpy(c1, hs.c1, 32);
  *c0_neg = hs.c0_neg ? 1 : 0;
  return hs.bits;
}
// the round-1 reduction (lattice.h ed25519_half_scalars_v1), for the
// equivalence test of the round-6 step
int dh_half_scalars_v1(const uint8_t* h32, uint8_t* c0, uint8_t* c1, int* c0_neg) {
  uint32_t h[8];
  bytes_to_words8(h, h32);
  HalfScalars hs;
  ed25519_half_scalars_v1(hs, h);
  memcpy(c0, hs.c0, 32);
  memcpy(c1, hs.c1, 32);
  *c0_neg = hs.c0_neg ? 1 : 0;
  return hs.bits;
}
int dh_ed25519_verify(const uint8_t* sig, const uint8_t* m, uint32_t mlen, const uint8_t* pk) {
  uint32_t s[16], p[8];
  for (int i = 0; i < 16; i++) s[i] = ld_le32(sig + 4 * i);
  bytes_to_words8(p, pk);
  Lane lane;
  return ed25519_verify_lane(s, p, ShaGlobalTail{m}, mlen, lane.s, host_btab()) ? 0 : -1;
}
int dh_vrf03_verify(uint8_t* beta, const uint8_t* pk, const uint8_t* proof, const uint8_t* alpha,
                    uint32_t alen) {
  uint32_t p[8], pi[20], b[16];
  bytes_to_words8(p, pk);
  for (int i = 0; i < 20; i++) pi[i] = ld_le32(proof + 4 * i);
  Lane lane;
  bool ok = vrf03_verify_lane(b, p, pi, ShaGlobalTail{alpha}, alen, lane.s, host_btab());
  memcpy(beta, b, 64);
  return ok ? 0 : -1;
}
int dh_sum6kes_verify(const uint8_t* vk, uint32_t t, const uint8_t* m, uint32_t mlen,
                      const uint8_t* sig) {
  uint32_t v[8];
  bytes_to_words8(v, vk);
  alignas(16) uint32_t sw[112];
  memcpy(sw, sig, 448);
  Lane lane;
  return sum6kes_verify_lane(v, t, sw, ShaGlobalTail{m}, mlen, lane.s, host_btab()) ? 0 : -1;
}
// mkSeed through the header kernels' own path (tpraos.h hdr_seed: blake2b.h
// mkseed_hash and the seedEta / seedL constants); eta0 = NULL: NeutralNonce.
void dh_mk_seed(uint8_t* out, int leader, uint64_t slot, const uint8_t* eta0) {
  alignas(16) uint8_t e0[32];
  if (eta0) memcpy(e0, eta0, 32);
  ouro_tpraos_batch b{};
  b.n = 1;
  b.slot = &slot;
  b.epoch_nonce = eta0 ? e0 : nullptr;
  SeedMsg a;
  hdr_seed(a, b, 0, leader != 0, batch_opts(b));
  memcpy(out, a.w, 32);
}
// The OCERT sharing key of tpraos.h (kernels.hip k_ocert_group) on a host SoA
// batch: the hash of header i's 144 key bytes, and whether headers i and j
// have the same ones.
unsigned long long dh_ocert_key_hash(const ouro_tpraos_batch* b, size_t i) {
  return ocert_key_hash(*b, i);
}
int dh_ocert_key_equal(const ouro_tpraos_batch* b, size_t i, size_t j) {
  return ocert_key_equal(*b, i, j) ? 1 : 0;
}
// The header drivers of tpraos.h for every header of a host SoA batch.
// mode 0 = throughput (one lane, key table shared), 1 = latency (a fresh lane
// per core, no sharing), 2 = latency on lane quads (the four products of each
// group operation emulated in sequence, with the merged operand bounds; the
// finish VRF by VRF as the lane pairs run it).  Pointers must be 16-B aligned like device buffers.
int dh_tpraos_verify(const ouro_tpraos_batch* b, int mode, uint8_t* verdict, uint8_t* beta_eta,
                     uint8_t* beta_leader) {
  std::vector<Lane> lanes(kLatCores);
  SlotRegion rr(kLatResWords);
  const Slot r = rr.s;
  const uint32_t opts = batch_opts(*b);
  for (size_t i = 0; i < b->n; i++) {
    std::fill(rr.buf.begin(), rr.buf.end(), 0);
    if (mode == 3) {
      // the split header kernel's phases (k_hdr_pre / k_hdr_dsm / k_hdr_post):
      // each core in its own task slot, the dsm from the cfg word the pre
      // phase left there
      for (int core = 0; core < kHdrCores; core++)
        hdr_core(*b, i, opts, core, lanes[core].s, r, host_btab(), true, false, false, kPhasePre,
                 lanes[kCoreUe].s);
      for (int core = 0; core < kHdrCores; core++)
        dsm_lane(lanes[core].s, host_btab(), (uint32_t)*lanes[core].s.word(kSlotCfg));
      for (int core = 0; core < kHdrCores; core++)
        hdr_core(*b, i, opts, core, lanes[core].s, r, nullptr, true, false, false, kPhasePost);
      hdr_finish_item(*b, i, opts, r, lanes[0].s, verdict, beta_eta, beta_leader);
      continue;
    }
    const int cores = mode ? kLatCores : kHdrCores;
    for (int core = 0; core < cores; core++)
      hdr_core(*b, i, opts, core, lanes[mode ? core : 0].s, r, host_btab(), mode == 0, mode != 0,
               mode == 2);
    if (mode == 2) {
      hdr_finish_item_split(*b, i, opts, r, verdict, beta_eta, beta_leader);
      continue;
    }
    if (mode) hdr_combine_split(r);
    hdr_finish_item(*b, i, opts, r, lanes[0].s, verdict, beta_eta, beta_leader);
  }
  return 0;
}

// ---- lane_items.h on the host: the entries of csrc/lane_test.hip (lt_*), same
// records, same items, run in a loop (tests/test_lane_exact.py, backend
// "host").  0, or -1 on bad arguments.  `stride` places items on the device's
// threads and means nothing here: wave_max_small is the identity on the host.
int dh_lt_op(int op, int n, const uint32_t* in, uint32_t* out, int param) {
  if (n <= 0 || !in || !out) return -1;
  return lt_host_op<0>(op, n, in, out, param);
}
int dh_lt_sha512(int n, const uint8_t* pre, const uint8_t* buf, size_t buflen, const uint32_t* off,
                 const uint32_t* len, uint8_t* out) {
  if (n <= 0 || !pre || !buf || !off || !len || !out) return -1;
  for (int i = 0; i < n; i++) {
    if ((size_t)off[i] + len[i] > buflen) return -1;
    uint32_t p[16], w[16];
    for (int k = 0; k < 16; k++) p[k] = ld_le32(pre + 64 * (size_t)i + 4 * k);
    lt::sha512_item(p, buf + off[i], len[i], w);
    memcpy(out + 64 * (size_t)i, w, 64);
  }
  return 0;
}
// variant 1: the pre phase, the chain from the cfg word it left, the finish --
// the split header kernel's schedule (the host has one dsm_lane)
int dh_lt_ed(int n, int stride, int variant, const uint32_t* in, uint32_t* out) {
  if (n <= 0 || stride <= 0 || !in || !out) return -1;
  for (int i = 0; i < n; i++) {
    Lane lane;
    uint32_t* o = out + (size_t)i * lt::kChainOut;
    lt::ed_setup(in + (size_t)i * lt::kEdIn, o, lane.s, host_btab(), variant ? kPhasePre : kPhaseAll);
    if (variant) dsm_lane(lane.s, host_btab(), (uint32_t)*lane.s.word(kSlotCfg));
    lt::chain_finish(o, lane.s);
  }
  return 0;
}
int dh_lt_u(int n, int stride, const uint32_t* in, uint32_t* out) {
  if (n <= 0 || stride <= 0 || !in || !out) return -1;
  for (int i = 0; i < n; i++) {
    Lane lane;
    lt::u_item(in + (size_t)i * lt::kUIn, out + (size_t)i * lt::kChainOut, lane.s, host_btab());
  }
  return 0;
}
int dh_lt_v(int n, int stride, const uint32_t* in, uint32_t* out) {
  if (n <= 0 || stride <= 0 || !in || !out) return -1;
  for (int i = 0; i < n; i++) {
    Lane lane;
    lt::v_item(in + (size_t)i * lt::kVIn, out + (size_t)i * lt::kChainOut, lane.s, host_btab());
  }
  return 0;
}

// ---- the latency mode's split helpers and wide B table (wide_cores.h, verify.h)
// the signed width-4 digits of s as pw_dsm forms them (sc_recode_carries<4, 64>,
// sc_digit_from<4>), and the carry mask
unsigned long long dh_wide_recode4(const uint32_t s[8], int32_t digits[64]) {
  const uint64_t c = sc_recode_carries<4, 64>(s);
  for (int j = 0; j < 64; j++)
    digits[j] = sc_digit_from<4>((s[j >> 3] >> (4 * (j & 7))) & 15u, c, j, 64);
  return c;
}
void dh_wide_high_half(uint32_t hh[8], const uint32_t h[8]) { wide::sc_high_half_with_carry(hh, h); }
// the cuts the host build instantiates: the product's V / V2 window, the V2 /
// V3 one relative to it (used with OURO_LAT_V3), and one more each with 4 K a
// multiple of 32 and not
#define DH_WIDE_KS OURO_LAT_VWIN, (OURO_LAT_VWIN2 - OURO_LAT_VWIN) & 63, 16, 29
int dh_wide_split_ks(int ks[4], int* v3) {
  const int k[4] = {DH_WIDE_KS};
  for (int i = 0; i < 4; i++) ks[i] = k[i];
  *v3 = OURO_LAT_V3;
  return 4;
}
int dh_wide_high_from_window(int which, uint32_t hh[8], const uint32_t s[8]) {
  constexpr int k[4] = {DH_WIDE_KS};
  switch (which) {
    case 0: wide::sc_high_from_window<k[0]>(hh, s); return k[0];
    case 1: wide::sc_high_from_window<k[1]>(hh, s); return k[1];
    case 2: wide::sc_high_from_window<k[2]>(hh, s); return k[2];
    case 3: wide::sc_high_from_window<k[3]>(hh, s); return k[3];
  }
  return -1;
}
// entry idx (= k - 1) of half `half` of the wide B table, built as runtime.cpp
// builds it (build_btab_wide over the niels tables), once per process
int dh_btab_wide_entry(int half, int idx, uint16_t out[kBWideU16]) {
  if (half < 0 || half > 1 || idx < 0 || idx >= kBTabEntries) return -1;
  static const std::vector<uint16_t> tab = [] {
    std::vector<uint16_t> t(2 * kBTabWideWords);
    build_btab_wide(t.data(), host_btab());
    return t;
  }();
  memcpy(out, tab.data() + ((size_t)half * kBTabEntries + idx) * kBWideU16, sizeof(uint16_t) * kBWideU16);
  return 0;
}

// [k]P through the prover's scalar chain (prove.h var_mul): P from its
// encoding; reduce != 0: k is a clamped scalar, reduced mod L first as the
// prover does (expand_seed_scalar).  -1 when P does not decode.
int dh_var_mul(uint8_t* out, const uint8_t* k, const uint8_t* point, int reduce) {
  uint32_t kw[8], kr[8], pw[8], enc[8];
  bytes_to_words8(kw, k);
  bytes_to_words8(pw, point);
  ge_p3 P;
  if (!ge_decode(&P, pw, false)) return -1;
  if (reduce) sc_reduce256(kr, kw);
  Lane lane;
  encode_p2(enc, var_mul(reduce ? kr : kw, P, lane.s, host_btab()));
  memcpy(out, enc, 32);
  return 0;
}
}
