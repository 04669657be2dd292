// Stand-alone AddressSanitizer + UBSan run of the per-key VRF tables
// (csrc/verify.h vrfkey_base / vrfkey_fill / vrf_u_fixed_lane, csrc/tpraos.h
// hdr_u_shared) and of the workspace arithmetic of their launch
// (csrc/vrfkey_ws.h), compiled here for the host with
// -fsanitize=address,undefined and called from this program's own main
// (tests/test_vrfkey_asan.py builds and runs it; nothing is loaded into
// Python).
//
// Every buffer is a heap block of exactly the size the kernels are given, so
// an access past a table, a window or a workspace region is a
// heap-buffer-overflow.  For a few keys -- valid ones, the small-order ones, a
// non-canonical one and one that does not decode -- the table is built and U
// is computed from it for directed and pseudo-random c; for the keys that are
// points of the curve it must equal the doubling chain's U (vrf_u_core).
// Output: "keys N chains M mismatches K layouts L".
#define OURO_NI_LINKAGE static
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "tpraos.h"
#include "vrfkey_ws.h"

using namespace ouro;

namespace {
struct Buf32 {
  std::unique_ptr<int32_t[]> p;
  explicit Buf32(size_t words) : p(new int32_t[words]()) {}
};
uint64_t g_rng = 0x243f6a8885a308d3ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}
void encode(uint8_t* out, Slot lane) {
  const ge_p2 U = dsm_result(lane);
  uint32_t enc[8];
  ge_encode_with_inv(enc, U.X, U.Y, fe_invert(U.Z));
  memcpy(out, enc, 32);
}
}  // namespace

int main() {
  Buf32 btab(kBTabWords), ubtab(kUBTabWords);
  build_btab(btab.p.get());
  build_ubtab(ubtab.p.get());

  std::vector<std::vector<uint8_t>> keys;
  std::vector<bool> on_curve;
  auto add = [&](const uint8_t* k, bool curve) {
    keys.emplace_back(k, k + 32);
    on_curve.push_back(curve);
  };
  uint8_t k[32];
  for (int y = 3, found = 0; found < 2; y++) {  // two valid keys: small y that decode
    memset(k, 0, 32);
    k[0] = (uint8_t)y;
    uint32_t w[8];
    bytes_to_words8(w, k);
    ge_p3 P;
    if (ge_decode(&P, w, false) && !ge_has_small_order(w)) {
      add(k, true);
      found++;
    }
  }
  memset(k, 0, 32);
  k[0] = 1;
  add(k, true);  // the identity
  memset(k, 0, 32);
  add(k, true);  // y = 0, order 4
  k[31] = 0x80;
  add(k, true);
  memset(k, 0xff, 32);
  k[0] = 0xec;
  k[31] = 0x7f;
  add(k, true);  // y = p - 1, order 2
  memset(k, 0xff, 32);
  k[31] = 0x7f;
  add(k, false);  // y = 2^255 - 1, not canonical
  memset(k, 0, 32);
  k[0] = 2;
  add(k, false);  // does not decode

  const uint32_t pat[] = {0u, 1u, 0xffffffffu, 0x80808080u, 0x7f7f7f7fu, 0x81818181u, 0xff00ff00u,
                          0x20820820u, 0xdf7df7dfu, 0x61861861u};
  size_t chains = 0, mismatches = 0;
  for (size_t ki = 0; ki < keys.size(); ki++) {
    uint32_t pk[8];
    bytes_to_words8(pk, keys[ki].data());
    Buf32 tab(kYKeyWords), base(kYBaseWords);
    const bool flag = vrfkey_base(pk, base.p.get());
    for (int j = 0; j < kYWindows; j++) vrfkey_fill(base.p.get(), tab.p.get(), j);
    for (int t = 0; t < 16; t++) {
      alignas(16) uint8_t proof[80];
      uint32_t pi[20];
      for (int i = 0; i < 20; i++) pi[i] = rnd();
      for (int i = 0; i < 4; i++)
        if (t < 10) pi[8 + i] = t == 1 && i ? 0u : pat[t];
      if (t & 1) pi[19] = 0xffffffffu;  // s above L: reduced on the way in
      memcpy(proof, pi, 80);
      ouro_tpraos_batch b{};
      b.n = 1;
      b.eta_proof = proof;
      Buf32 lane1(kLaneWords), lane2(kLaneWords), res(kResWords);
      hdr_u_shared(b, 0, false, flag, Slot{lane1.p.get()}, Slot{res.p.get()}, ubtab.p.get(),
                   tab.p.get());
      const bool flag2 = vrf_u_core(pk, pi, true, 2, Slot{lane2.p.get()}, btab.p.get());
      uint8_t u1[32], u2[32];
      encode(u1, Slot{lane1.p.get()});
      encode(u2, Slot{lane2.p.get()});
      chains++;
      if (flag != flag2 || (on_curve[ki] && memcmp(u1, u2, 32) != 0)) mismatches++;
    }
  }

  // the workspace: every region inside the block, in order, the flags last
  size_t layouts = 0;
  const size_t ns[] = {1, 15, 16, 17, 65, 1000, 2048, 65536, 1u << 20};
  const size_t budgets[] = {0, kYKeyBytes - 1, kYKeyBytes, 3 * kYKeyBytes, (size_t)512 << 20};
  for (size_t n : ns)
    for (size_t budget : budgets) {
      const VrfKeyLayout L = vrfkey_layout(n, kYKeyBytes, budget);
      layouts++;
      if (!L.kmax) continue;
      std::unique_ptr<uint8_t[]> g(new uint8_t[L.group_bytes]);
      memset(g.get(), 0, L.off_rep);                 // the launch's clear
      memset(g.get() + L.off_desc, 1, 64);           // the header kernel's record
      memset(g.get() + L.off_rep, 2, 4 * n);
      memset(g.get() + L.off_uniq, 3, 4 * n);
      memset(g.get() + L.off_kidx, 4, 4 * n);
      memset(g.get() + L.off_flag, 5, L.kmax);
      if (L.off_table != L.off_desc + 64 || L.off_rep != L.off_table + 4 * L.cap ||
          L.table_bytes > budget || L.kmax > n / kVrfKeyMinPerKey || L.cap < 2 * n)
        mismatches++;
    }
  printf("keys %zu chains %zu mismatches %zu layouts %zu\n", keys.size(), chains, mismatches,
         layouts);
  return mismatches ? 1 : 0;
}
