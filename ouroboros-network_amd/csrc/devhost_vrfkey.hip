// devhost_vrfkey.hip -- TEST-ONLY host build of the per-key VRF tables
// (verify.h vrfkey_base / vrfkey_fill / vrf_u_fixed_lane, tpraos.h
// hdr_u_shared), a second unit of lib/libouro_devhost_test.so.  The counters
// and the bound tracker's hooks are devhost_test.hip's.
#define OURO_NI_LINKAGE static  // this unit's own copies of the out-of-line routines
#include <algorithm>
#include <cstring>
#include <vector>

#include "lane_items.h"
#include "tpraos.h"
#include "vrfkey_ws.h"

using namespace ouro;

namespace {
const int32_t* host_btab() {
  static std::vector<int32_t> tab = [] {
    std::vector<int32_t> t(kBTabWords);
    build_btab(t.data());
    return t;
  }();
  return tab.data();
}
const int32_t* host_ubtab() {
  static std::vector<int32_t> tab = [] {
    std::vector<int32_t> t(kUBTabWords);
    build_ubtab(t.data());
    return t;
  }();
  return tab.data();
}
struct Lane {
  std::vector<int32_t> buf;
  Slot s;
  Lane() : buf(slot_region_words(1, kLaneWords) + 4, 0) {
    s = Slot{reinterpret_cast<int32_t*>((reinterpret_cast<uintptr_t>(buf.data()) + 15) & ~uintptr_t(15))};
  }
};
void encode_result(uint8_t* out, Slot lane) {
  const ge_p2 U = dsm_result(lane);
  uint32_t enc[8];
  ge_encode_with_inv(enc, U.X, U.Y, fe_invert(U.Z));
  memcpy(out, enc, 32);
}
}  // namespace

extern "C" {

// the compiled width, windows, entries and int32 words per key (table, base
// points), and the minimum headers per key
void dh_vrfkey_params(int* width, int* windows, int* entries, size_t* tab_words,
                      size_t* base_words, size_t* min_per_key) {
  *width = kYW;
  *windows = kYWindows;
  *entries = kYKeyEntries;
  *tab_words = kYKeyWords;
  *base_words = kYBaseWords;
  *min_per_key = kVrfKeyMinPerKey;
}
// the per-key pass and the fill of every window, as k_vrfkey_base and
// k_vrfkey_fill run them; returns the key's flag
int dh_vrfkey_build(const uint8_t* pk, int32_t* tab, int32_t* base) {
  uint32_t p[8];
  bytes_to_words8(p, pk);
  const bool ok = vrfkey_base(p, base);
  for (int j = 0; j < kYWindows; j++) vrfkey_fill(base, tab, j);
  return ok ? 1 : 0;
}
// U = [s]B - [c]Y, encoded, through the header's shared core (the table chain)
void dh_vrfkey_u(uint8_t* out, const int32_t* tab, const uint8_t* c16, const uint8_t* s32) {
  alignas(16) uint8_t proof[80] = {0};
  memcpy(proof + 32, c16, 16);
  memcpy(proof + 48, s32, 32);
  ouro_tpraos_batch b{};
  b.n = 1;
  b.eta_proof = proof;
  Lane lane;
  std::vector<int32_t> res(kResWords + 4, 0);
  hdr_u_shared(b, 0, false, true, lane.s, Slot{res.data()}, host_ubtab(), tab);
  encode_result(out, lane.s);
}
// ... and through today's core (vrf_u_core: the key's [1..8](-Y) table and
// dsm_lane's doubling chain); returns the key's flag
int dh_vrfkey_u_inline(uint8_t* out, const uint8_t* pk, const uint8_t* c16, const uint8_t* s32) {
  uint32_t p[8], pi[20] = {0};
  bytes_to_words8(p, pk);
  memcpy(pi + 8, c16, 16);
  memcpy(pi + 12, s32, 32);
  Lane lane;
  const bool ok = vrf_u_core(p, pi, true, 2, lane.s, host_btab());
  encode_result(out, lane.s);
  return ok ? 1 : 0;
}
// The throughput header schedule with both U cores from the key's table, for
// a host SoA batch whose headers all carry the key `tab` was built from
// (key_ok: that key's flag); dh_tpraos_verify mode 0 with the sharing on.
int dh_tpraos_verify_shared(const ouro_tpraos_batch* b, const int32_t* tab, int key_ok,
                            uint8_t* verdict, uint8_t* beta_eta, uint8_t* beta_leader) {
  Lane lane;
  std::vector<int32_t> rr(kResWords + 4, 0);
  const Slot r{rr.data()};
  const uint32_t opts = batch_opts(*b);
  for (size_t i = 0; i < b->n; i++) {
    std::fill(rr.begin(), rr.end(), 0);
    for (int core = 0; core < kHdrCores; core++) {
      if (core == kCoreUe || core == kCoreUl)
        hdr_u_shared(*b, i, core == kCoreUl, key_ok != 0, lane.s, r, host_ubtab(), tab);
      else
        hdr_core(*b, i, opts, core, lane.s, r, host_btab());
    }
    hdr_finish_item(*b, i, opts, r, lane.s, verdict, beta_eta, beta_leader);
  }
  return 0;
}
// the workspace arithmetic of the launch (vrfkey_ws.h): out7 = {kmax, cap,
// off_rep, off_uniq, off_kidx, off_flag, group_bytes}; returns table_bytes
size_t dh_vrfkey_layout(size_t n, size_t budget, size_t* out7) {
  const VrfKeyLayout L = vrfkey_layout(n, kYKeyBytes, budget);
  const size_t v[7] = {L.kmax, L.cap, L.off_rep, L.off_uniq, L.off_kidx, L.off_flag, L.group_bytes};
  memcpy(out7, v, sizeof v);
  return L.table_bytes;
}

// lane_items.h's table U on the host (csrc/lane_test.hip lt_u_table): the
// per-key pass and the fill of every window for each of nkeys keys, then item
// i from the table of key kidx[i] with the c and s of its 80-byte proof.
// 0, or -1 on bad arguments.
int dh_lt_u_table(int nkeys, const uint8_t* keys, int n, const uint32_t* kidx,
                  const uint8_t* proofs, int stride, uint32_t* out) {
  if (nkeys <= 0 || n <= 0 || stride <= 0 || !keys || !kidx || !proofs || !out) return -1;
  std::vector<int32_t> tabs((size_t)nkeys * kYKeyWords), base(kYBaseWords);
  std::vector<uint8_t> flag(nkeys);
  for (int k = 0; k < nkeys; k++)
    flag[k] = (uint8_t)dh_vrfkey_build(keys + 32 * (size_t)k, tabs.data() + (size_t)k * kYKeyWords,
                                       base.data());
  ouro_tpraos_batch b{};
  b.n = (size_t)n;
  b.eta_proof = proofs;
  for (int i = 0; i < n; i++) {
    if (kidx[i] >= (uint32_t)nkeys) return -1;
    Lane lane;
    std::vector<int32_t> res(kResWords + 4, 0);
    lt::u_table_item(b, (size_t)i, flag[kidx[i]] != 0, out + (size_t)i * lt::kChainOut, lane.s,
                     Slot{res.data()}, host_ubtab(), tabs.data() + (size_t)kidx[i] * kYKeyWords);
  }
  return 0;
}
}
