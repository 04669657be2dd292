// Stand-alone AddressSanitizer + UBSan run of the host prover and the host
// leader schedule (csrc/forge.h, csrc/prove.h): the item routines
// ouro_vrf03_prove_batch_host and ouro_tpraos_leader_schedule_host run per
// item, compiled here with -fsanitize=address,undefined and called from this
// program's own main (tests/test_prove_asan.py builds and runs it; nothing is
// loaded into Python).
//
// Input: a file of records.
//   'P' sk[64] len:u32 alpha[len]   one certified VRF; alpha is copied into a
//       heap buffer of exactly its length, so it ends at the last byte of its
//       allocation and any read past the span is a heap-buffer-overflow
//   'S' sk[64] have_eta0:u32 eta0[32] f_is_one:u32 ngen:u32 epoch_first_slot
//       sigma_num sigma_den act_log_lo act_log_hi d_num d_den asc_inv
//       first_slot (u64 each) n:u32   a schedule of n slots; cls, gen_index and
//       beta go to heap rows of exactly n items
// The lane's scratch slot is a heap buffer of exactly one slot.
// Output: one line "records N digest <hex>" where digest folds every proof,
// output, class and index (the test compares it with the oracle's).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "forge.h"

using namespace ouro;

static uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: prove_asan RECORDS\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int32_t* btab = static_cast<int32_t*>(malloc(sizeof(int32_t) * kBTabWords));
  int32_t* slot = static_cast<int32_t*>(malloc(sizeof(int32_t) * kLaneWords));
  if (!btab || !slot) return 2;
  build_btab(btab);
  memset(slot, 0, sizeof(int32_t) * kLaneWords);
  const Slot lane{slot};
  size_t records = 0;
  uint32_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (;;) {
    uint8_t kind, skb[64], b4[4];
    if (fread(&kind, 1, 1, f) != 1) break;
    if (!rd(f, skb, 64)) return 2;
    uint32_t x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (kind == 'P') {
      if (!rd(f, b4, 4)) return 2;
      const uint32_t len = le32(b4);
      uint8_t* alpha = static_cast<uint8_t*>(malloc(len ? len : 1));
      if (!alpha || !rd(f, alpha, len)) return 2;
      uint32_t sk[16], pi[20], beta[16];
      for (int k = 0; k < 16; k++) sk[k] = le32(skb + 4 * k);
      forge_prove_item(pi, beta, sk, ShaGlobalTail{alpha}, len, lane, btab);
      prove_wipe_lane(lane);
      for (int k = 0; k < 20; k++) x[k & 7] ^= pi[k];
      for (int k = 0; k < 16; k++) x[k & 7] += beta[k];
      free(alpha);
    } else if (kind == 'S') {
      uint8_t h[44 + 72 + 4];
      if (!rd(f, h, sizeof h)) return 2;
      OuroForgeSched s;
      memset(&s, 0, sizeof s);
      {
        uint32_t sk[16];
        ExpandedKey k;
        for (int i = 0; i < 16; i++) sk[i] = le32(skb + 4 * i);
        expand_vrf_sk(k, sk);
        for (int i = 0; i < 8; i++) {
          s.x[i] = k.a[i];
          s.pk[i] = k.pk[i];
        }
      }
      s.have_eta0 = le32(h);
      for (int i = 0; i < 8; i++) s.eta0[i] = le32(h + 4 + 4 * i);
      s.f_is_one = le32(h + 36);
      s.ngen = le32(h + 40);
      const uint8_t* q = h + 44;
      s.epoch_first_slot = le64(q);
      s.sigma_num = le64(q + 8);
      s.sigma_den = le64(q + 16);
      s.act_log_lo = le64(q + 24);
      s.act_log_hi = (int64_t)le64(q + 32);
      s.d_num = le64(q + 40);
      s.d_den = le64(q + 48);
      s.asc_inv = le64(q + 56);
      const uint64_t first_slot = le64(q + 64);
      const uint32_t n = le32(q + 72);
      uint8_t* cls = static_cast<uint8_t*>(malloc(n ? n : 1));
      uint32_t* gen = static_cast<uint32_t*>(malloc(n ? 4 * (size_t)n : 1));
      uint8_t* beta = static_cast<uint8_t*>(malloc(n ? 64 * (size_t)n : 1));
      if (!cls || !gen || !beta) return 2;
      for (uint32_t i = 0; i < n; i++) {
        uint32_t b[16];
        cls[i] = forge_schedule_item(s, first_slot + i, b, &gen[i], lane, btab);
        memcpy(beta + 64 * (size_t)i, b, 64);
        prove_wipe_lane(lane);
      }
      for (uint32_t i = 0; i < n; i++) {
        x[i & 7] += (uint32_t)cls[i] * 0x9e3779b1u + gen[i];
        for (int k = 0; k < 16; k++) x[k & 7] ^= le32(beta + 64 * (size_t)i + 4 * k) + i;
      }
      free(cls);
      free(gen);
      free(beta);
    } else {
      fprintf(stderr, "unknown record\n");
      return 2;
    }
    for (int k = 0; k < 8; k++) fold[k] = fold[k] * 1000003u + x[k];
    records++;
  }
  fclose(f);
  free(btab);
  free(slot);
  printf("records %zu digest", records);
  for (int k = 0; k < 8; k++) printf(" %08x", fold[k]);
  printf("\n");
  return 0;
}
