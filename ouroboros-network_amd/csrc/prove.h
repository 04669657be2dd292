// prove.h -- the signing-side lane routines of the draft-03 VRF (PraosVRF
// evalCertified; cardano-crypto-praos crypto_vrf_ietfdraft03_prove) and the
// scalar multiplications under them.  Product code: kernels_forge.hip runs
// them on the device and host_path.hip on the host (include/ouro_verify.h
// ouro_vrf03_prove_batch, ouro_tpraos_leader_schedule, ouro_tpraos_leader_vrfs);
// synth.h includes this header for its input synthesis, so there is one copy.
// Deterministic, and pinned byte for byte against the oracle's prover, the
// IETF draft-03 vectors and a prover built from libsodium's primitives
// (tests/test_prove_rule.py).
//
// NO constant-time or side-channel claim: var_mul indexes a per-lane table of
// multiples by digits of the secret scalar, and the doubling chain skips
// leading zero windows.  These routines are for a machine that already holds
// the key.  A lane's scratch slot holds the scalar and its recoding while a
// multiplication runs; prove_wipe_lane clears them afterwards.  On the host
// every named local that held the key, its expansion, the nonce or an
// unreduced product of them is zeroed before its routine returns (prove_wipe);
// on the device such locals are registers, and neither they nor what the
// compiler spills or copies on either side is within the code's reach.
#pragma once
#include "verify.h"

namespace ouro {

// Zero n bytes of a local that held secret material, through a volatile
// pointer so that the stores stay.  Host only: a device local is a register
// allocation, and forcing it to memory to clear it would put it there first.
OURO_FI void prove_wipe(void* p, size_t n) {
#if !defined(__HIP_DEVICE_COMPILE__)
  volatile unsigned char* q = static_cast<volatile unsigned char*>(p);
  for (size_t i = 0; i < n; i++) q[i] = 0;
#else
  (void)p;
  (void)n;
#endif
}

// a*b + c mod L (all 8-word little-endian)
OURO_FI void sc_muladd(uint32_t out[8], const uint32_t a[8], const uint32_t b[8],
                       const uint32_t c[8]) {
  uint32_t p[16];
#pragma unroll
  for (int i = 0; i < 16; i++) p[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      uint64_t t = (uint64_t)a[i] * b[j] + p[i + j] + carry;
      p[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    p[i + 8] = (uint32_t)carry;
  }
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    uint64_t t = (uint64_t)p[i] + (i < 8 ? c[i] : 0u) + carry;
    p[i] = (uint32_t)t;
    carry = t >> 32;
  }
  sc_reduce512(out, p);
  prove_wipe(p, sizeof p);  // (k + c x before its reduction)
}

// [k]B for k < L, through the shared multiplication routine (B table only)
OURO_FI ge_p2 base_mul(const uint32_t k[8], Slot lane, const int32_t* btab) {
  st_words8(lane + kSlotB, k);
  st_carry(lane, 2, sc_recode_b(k));
  dsm(lane, btab, dsm_cfg(0, 0, true));
  return dsm_result(lane);
}

// [k]P for k < L
OURO_FI ge_p2 var_mul(const uint32_t k[8], const ge_p3& P, Slot lane, const int32_t* btab) {
  build_table(lane + kSlotTab1, P);
  st_words8(lane + kSlotA1, k);
  st_carry(lane, 0, sc_recode_carries<4, 64>(k));
  dsm(lane, btab, dsm_cfg(64, 0, false));
  return dsm_result(lane);
}

OURO_FI void encode_p2(uint32_t out[8], const ge_p2& p) { ge_p2_encode(out, p); }

// the scalars and their recoding carries out of a lane's scratch slot (the
// tables and the result slot hold public points only: multiples of H and of
// B, Gamma, kB, kH)
OURO_FI void prove_wipe_lane(Slot lane) {
  const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  st_words8(lane + kSlotA1, z);
  st_words8(lane + kSlotA2, z);
  st_words8(lane + kSlotB, z);
#pragma unroll
  for (int k = 0; k < 3; k++) st_carry(lane, k, 0);
}

// SHA-512 of a 32-byte register message
OURO_FI void sha512_32(uint32_t out[16], const uint32_t m[8]) {
  uint64_t H[8];
  sha512_prefixed<32>(H, m, ShaNoTail{}, 0);
  sha512_digest_words(out, H);
}

// az = SHA-512(seed) with the Ed25519 clamp; a = az[0:32] mod L
struct ExpandedKey {
  uint32_t a[8];       // clamped scalar reduced mod L
  uint32_t a_raw[8];   // clamped scalar as used for s = k + c x (reduced by muladd)
  uint32_t prefix[8];  // az[32:64]
  uint32_t pk[8];
};

// the scalar and the nonce prefix of a seed; pk is left to the caller
OURO_FI void expand_seed_scalar(ExpandedKey& k, const uint32_t seed[8]) {
  uint32_t az[16];
  sha512_32(az, seed);
  az[0] &= 0xfffffff8u;
  az[7] &= 0x7fffffffu;
  az[7] |= 0x40000000u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k.a_raw[i] = az[i];
    k.prefix[i] = az[8 + i];
  }
  sc_reduce256(k.a, k.a_raw);
  prove_wipe(az, sizeof az);
}

OURO_FI void expand_seed(ExpandedKey& k, const uint32_t seed[8], Slot lane,
                         const int32_t* btab) {
  expand_seed_scalar(k, seed);
  encode_p2(k.pk, base_mul(k.a, lane, btab));
}

// a VRF signing key sk = seed(32) || pk(32) as libsodium lays it out: the
// scalar from the seed, the public key bytes AS GIVEN (crypto_vrf_ietfdraft03_
// prove hashes sk + 32 into H; it never recomputes the key)
OURO_FI void expand_vrf_sk(ExpandedKey& k, const uint32_t sk[16]) {
  expand_seed_scalar(k, sk);
#pragma unroll
  for (int i = 0; i < 8; i++) k.pk[i] = sk[8 + i];
}

// a 32-byte message in registers as a SHA tail source
struct ProveRegTail {
  uint32_t w[8];
  OURO_FI uint32_t tail(uint32_t q) const { return byte_of(w, (int)q); }
};

// H = hash_to_curve(pk, alpha) = Elligator2(SHA-512(0x04 || 0x01 || pk || alpha)[0:32])
template <class Tail>
OURO_FI ge_p3 vrf03_hash_to_curve(const uint32_t pk[8], const Tail& alpha, uint32_t alen) {
  uint32_t pre[9];
  pre[0] = 0x04u | (0x01u << 8) | (pk[0] << 16);
#pragma unroll
  for (int i = 1; i < 8; i++) pre[i] = (pk[i - 1] >> 16) | (pk[i] << 16);
  pre[8] = pk[7] >> 16;
  uint64_t Hs[8];
  sha512_prefixed<34>(Hs, pre, alpha, alen);
  uint32_t rw[16];
  sha512_digest_words(rw, Hs);
  rw[7] &= 0x7fffffffu;
  return elligator2_h(rw);
}

// draft-03 prove (SURVEY.md App. B.3'): pi = Gamma (8 words) || c (4) || s (8),
// alpha of any length from a SHA tail source; beta (optional, 16 words): the
// output, SHA-512(0x04 || 0x03 || encode([8]Gamma))
OURO_HD inline void vrf03_beta_of_gamma(uint32_t beta[16], const ge_p2& Gamma);
template <class Tail>
OURO_HD inline void vrf03_prove_lane(uint32_t pi[20], const ExpandedKey& k, const Tail& alpha,
                                     uint32_t alen, Slot lane, const int32_t* btab,
                                     uint32_t* beta = nullptr) {
  ge_p3 Hp = vrf03_hash_to_curve(k.pk, alpha, alen);
  uint32_t Henc[8];
  ge_encode_with_inv(Henc, Hp.X, Hp.Y, fe_invert(Hp.Z));
  // Gamma = [x]H
  uint32_t G[8];
  {
    const ge_p2 Gp = var_mul(k.a, Hp, lane, btab);
    encode_p2(G, Gp);
    if (beta) vrf03_beta_of_gamma(beta, Gp);
  }
  // nonce k = SHA-512(prefix || H) mod L
  uint32_t nm[16], nw[16], kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    nm[i] = k.prefix[i];
    nm[8 + i] = Henc[i];
  }
  uint64_t Hn[8];
  sha512_prefixed<64>(Hn, nm, ShaNoTail{}, 0);
  sha512_digest_words(nw, Hn);
  sc_reduce512(kk, nw);
  uint32_t KB[8], KH[8];
  encode_p2(KB, base_mul(kk, lane, btab));
  encode_p2(KH, var_mul(kk, Hp, lane, btab));
  // c = SHA-512(4 || 2 || H || Gamma || kB || kH)[0:16]
  uint32_t hp[33];
  const uint32_t* pts[4] = {Henc, G, KB, KH};
  hp[0] = 0x04u | (0x02u << 8) | (Henc[0] << 16);
#pragma unroll
  for (int q = 0; q < 4; q++) {
#pragma unroll
    for (int i = 1; i < 8; i++) hp[8 * q + i] = (pts[q][i - 1] >> 16) | (pts[q][i] << 16);
    if (q < 3) hp[8 * q + 8] = (pts[q][7] >> 16) | (pts[q + 1][0] << 16);
  }
  hp[32] = KH[7] >> 16;
  uint64_t Hc[8];
  sha512_prefixed<130>(Hc, hp, ShaNoTail{}, 0);
  uint32_t cw[16], c[8], s[8];
  sha512_digest_words(cw, Hc);
#pragma unroll
  for (int i = 0; i < 8; i++) c[i] = i < 4 ? cw[i] : 0u;
  sc_muladd(s, c, k.a, kk);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    pi[i] = G[i];
    pi[12 + i] = s[i];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) pi[8 + i] = c[i];
  // the nonce, and what it was made from: with the proof it gives the key
  prove_wipe(kk, sizeof kk);
  prove_wipe(nw, sizeof nw);
  prove_wipe(nm, sizeof nm);
  prove_wipe(Hn, sizeof Hn);
}

// ... the 32-byte register form (the seeds)
OURO_FI void vrf03_prove_lane(uint32_t pi[20], const ExpandedKey& k, const uint32_t alpha[8],
                              Slot lane, const int32_t* btab) {
  ProveRegTail at;
#pragma unroll
  for (int i = 0; i < 8; i++) at.w[i] = alpha[i];
  vrf03_prove_lane(pi, k, at, 32, lane, btab);
}

// beta = SHA-512(0x04 || 0x03 || encode([8]Gamma)), as proof_to_hash computes
// it from the proof
OURO_HD inline void vrf03_beta_of_gamma(uint32_t beta[16], const ge_p2& Gamma) {
  ge_p2 t = ge_p1p1_to_p2(ge_p2_dbl(Gamma));
  t = ge_p1p1_to_p2(ge_p2_dbl(t));
  t = ge_p1p1_to_p2(ge_p2_dbl(t));
  uint32_t G8enc[8];
  encode_p2(G8enc, t);
  uint32_t bp[9];
  bp[0] = 0x04u | (0x03u << 8) | (G8enc[0] << 16);
#pragma unroll
  for (int i = 1; i < 8; i++) bp[i] = (G8enc[i - 1] >> 16) | (G8enc[i] << 16);
  bp[8] = G8enc[7] >> 16;
  uint64_t Hb[8];
  sha512_prefixed<34>(Hb, bp, ShaNoTail{}, 0);
  sha512_digest_words(beta, Hb);
}

// The output alone, all a slot that does not win needs: H, Gamma = [x]H and
// beta = SHA-512(0x04 || 0x03 || encode([8]Gamma)); no nonce, no c, no s.
// x: the clamped scalar reduced mod L (ExpandedKey a).
template <class Tail>
OURO_HD inline void vrf03_gamma_lane(uint32_t beta[16], const uint32_t x[8], const uint32_t pk[8],
                                     const Tail& alpha, uint32_t alen, Slot lane,
                                     const int32_t* btab) {
  const ge_p3 Hp = vrf03_hash_to_curve(pk, alpha, alen);
  vrf03_beta_of_gamma(beta, var_mul(x, Hp, lane, btab));
}

}  // namespace ouro
