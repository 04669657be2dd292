// lane_items.h -- TEST-ONLY: the lane routines as batch items, written once.
//
// One item = one call of a lane routine (fe25519.h, sc25519.h, lattice.h,
// modinv.h, sha512.h, blake2b.h, ge25519.h, verify.h, tpraos.h) with plain
// words in and plain words out.  Two callers run the same items over the same
// records: csrc/lane_test.hip from kernels, one item per lane, and
// csrc/devhost_test.hip / devhost_vrfkey.hip in a host loop.
// tests/test_lane_exact.py compares every output word with exact integer
// arithmetic.  The product library does not include this file.
#pragma once
#include "tpraos.h"

namespace ouro {
namespace lt {

// ---- items with a fixed record: kIn words in, kOut words out ----------------
constexpr int kIn = 20, kOut = 20;
enum Op {
  // two canonical 32-byte inputs a (words 0..7), b (8..15) through
  // fe_from_words; the result's canonical words (fe_to_words) at out 0..7
  kOpMul = 0, kOpSq, kOpAdd, kOpSub, kOpSub4, kOpNeg, kOpInvert, kOpPow22523,
  kOpInvVt, kOpInvVt10, kOpInvVt10Sel, kOpInvVt30Spec,
  kOpSqChain,  // `param` squarings of a, nothing canonicalised in between
  // raw limbs f (words 0..9), g (10..19) through fe_make; canonical words at
  // out 0..7, the result's limbs at out 8..17 where the item has some
  kOpRawWords, kOpRawCarry, kOpRawInvVt, kOpRawPack, kOpRawMul, kOpRawSq,
  kOpReduce512,  // words 0..15 -> 8 words
  kOpReduce256,  // words 0..7 -> 8 words
  // h (words 0..7) -> |c0| (out 0..7), c1 (8..15), c0's sign (16), bits (17)
  kOpHalfV2, kOpHalfV1,
  kOpBlake2b256_64,  // words 0..15 -> 8 words
  // an encoding (words 0..7) -> ok (out 0), ge_is_canonical (1),
  // ge_has_small_order (2), affine x (4..11) and y (12..19)
  kOpDecode, kOpDecodeNegate,
  kOpElligator2,  // r (words 0..7, bit 255 cleared) -> the encoding of [8]H
  kOps
};

OURO_FI fe raw_fe(const uint32_t* l) {
  return fe_make(l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8], l[9]);
}
OURO_FI void put_limbs(uint32_t* o, const fe& f) {
#pragma unroll
  for (int i = 0; i < 10; i++) o[i] = f.v[i];
}

template <int kOp>
OURO_HD inline void item(const uint32_t* in, uint32_t* out, int param) {
  uint32_t r[kIn], o[kOut];
#pragma unroll
  for (int k = 0; k < kIn; k++) r[k] = in[k];
#pragma unroll
  for (int k = 0; k < kOut; k++) o[k] = 0;
  if constexpr (kOp <= kOpSqChain) {
    const fe a = fe_from_words(r), b = fe_from_words(r + 8);
    fe h = a;
    if constexpr (kOp == kOpMul) h = fe_mul(a, b);
    else if constexpr (kOp == kOpSq) h = fe_sq(a);
    else if constexpr (kOp == kOpAdd) h = fe_add(a, b);
    else if constexpr (kOp == kOpSub) h = fe_sub(a, b);
    else if constexpr (kOp == kOpSub4) h = fe_sub4(a, b);
    else if constexpr (kOp == kOpNeg) h = fe_neg(a);
    else if constexpr (kOp == kOpInvert) h = fe_invert(a);
    else if constexpr (kOp == kOpPow22523) h = fe_pow22523(a);
    else if constexpr (kOp == kOpInvVt) h = fe_invert_vartime(a);
    else if constexpr (kOp == kOpInvVt10) h = fe_invert_vartime<10>(a);
    else if constexpr (kOp == kOpInvVt10Sel) h = fe_invert_vartime<10, true>(a);
    else if constexpr (kOp == kOpInvVt30Spec) h = fe_invert_vartime<30, true, true>(a);
    else {
#pragma unroll 1
      for (int k = 0; k < param; k++) h = fe_sq(h);
    }
    fe_to_words(o, h);
  } else if constexpr (kOp <= kOpRawSq) {
    const fe f = raw_fe(r), g = raw_fe(r + 10);
    if constexpr (kOp == kOpRawWords) {
      fe_to_words(o, f);
    } else if constexpr (kOp == kOpRawInvVt) {
      fe_to_words(o, fe_invert_vartime(f));
    } else if constexpr (kOp == kOpRawPack) {
      fe_pack256(o, f);
      put_limbs(o + 8, fe_unpack256(o));
    } else {
      const fe h = kOp == kOpRawCarry ? fe_carry(f) : kOp == kOpRawMul ? fe_mul(f, g) : fe_sq(f);
      fe_to_words(o, h);
      put_limbs(o + 8, h);
    }
  } else if constexpr (kOp == kOpReduce512) {
    sc_reduce512(o, r);
  } else if constexpr (kOp == kOpReduce256) {
    sc_reduce256(o, r);
  } else if constexpr (kOp == kOpHalfV2 || kOp == kOpHalfV1) {
    HalfScalars hs;
    if constexpr (kOp == kOpHalfV2) ed25519_half_scalars_v2(hs, r);
    else ed25519_half_scalars_v1(hs, r);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      o[k] = hs.c0[k];
      o[8 + k] = hs.c1[k];
    }
    o[16] = hs.c0_neg ? 1u : 0u;
    o[17] = (uint32_t)hs.bits;
  } else if constexpr (kOp == kOpBlake2b256_64) {
    blake2b256_64(o, r);
  } else if constexpr (kOp == kOpDecode || kOp == kOpDecodeNegate) {
    ge_p3 P;
    o[0] = ge_decode(&P, r, kOp == kOpDecodeNegate) ? 1u : 0u;
    o[1] = ge_is_canonical(r) ? 1u : 0u;
    o[2] = ge_has_small_order(r) ? 1u : 0u;
    const fe zi = fe_invert(P.Z);
    fe_to_words(o + 4, fe_mul(P.X, zi));
    fe_to_words(o + 12, fe_mul(P.Y, zi));
  } else {
    static_assert(kOp == kOpElligator2, "an item for every Op");
    r[7] &= 0x7fffffffu;
    const ge_p3 H = elligator2_h(r);
    ge_encode_with_inv(o, H.X, H.Y, fe_invert(H.Z));
  }
#pragma unroll
  for (int k = 0; k < kOut; k++) out[k] = o[k];
}

// SHA-512(pre || msg[0 .. len)): the 64-byte prefix in registers, the tail
// from memory at any alignment (ShaGlobalTail), the digest's 16 words out
OURO_HD inline void sha512_item(const uint32_t* pre16, const uint8_t* msg, uint32_t len,
                                uint32_t* out16) {
  uint32_t pre[16], w[16];
#pragma unroll
  for (int k = 0; k < 16; k++) pre[k] = pre16[k];
  uint64_t H[8];
  sha512_prefixed<64>(H, pre, ShaGlobalTail{msg}, len);
  sha512_digest_words(w, H);
#pragma unroll
  for (int k = 0; k < 16; k++) out16[k] = w[k];
}

// ---- the chain in its product configurations ---------------------------------
// Every chain item writes kChainOut words: the encoding of the chain's result
// (0..7), dsm_result_is_identity (8), and flags of its own (9..11).
constexpr int kChainOut = 12;
OURO_HD inline void chain_finish(uint32_t* out, Slot lane) {
  const ge_p2 Q = dsm_result(lane);
  uint32_t e[8];
  ge_encode_with_inv(e, Q.X, Q.Y, fe_invert(Q.Z));
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = e[k];
  out[8] = dsm_result_is_identity(lane) ? 1u : 0u;
}

// ED, as ed25519_verify_lane sets it up: [b]B + [+-|c0|](-A) + [c1](-R).
// in: A (0..7), R (8..15), |c0| (16..23), c1 (24..31), b (32..39), c0's sign
// (40), bits (41).  out 9 / 10: A / R decoded, 11: the window count the chain
// ran with.  phase as in ed25519_verify_lane: kPhasePre leaves the cfg word in
// the slot for a dsm launch of its own.
constexpr int kEdIn = 44;
OURO_HD inline void ed_setup(const uint32_t* in, uint32_t* out, Slot lane, const int32_t* btab,
                             int phase) {
  uint32_t A[8], R[8], b[8];
  HalfScalars hs;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    A[k] = in[k];
    R[k] = in[8 + k];
    hs.c0[k] = in[16 + k];
    hs.c1[k] = in[24 + k];
    b[k] = in[32 + k];
  }
  hs.c0_neg = in[40] != 0;
  hs.bits = (int)in[41];
  ge_p3 negA, negR;
  bool okA, okR;
  ge_decode_pair(&negA, &okA, &negR, &okR, A, R, true);
  build_table(lane + kSlotTab1, hs.c0_neg ? ge_p3_neg(negA) : negA);
  build_table(lane + kSlotTab2, negR);
  st_words8(lane + kSlotA1, hs.c0);
  st_words8(lane + kSlotA2, hs.c1);
  st_words8(lane + kSlotB, b);
  st_carry(lane, 0, sc_recode_carries<4, 64>(hs.c0));
  st_carry(lane, 1, sc_recode_carries<4, 64>(hs.c1));
  st_carry(lane, 2, sc_recode_b(b));
  int nw = wave_max_small((hs.bits + 4) >> 2);
  nw = nw < 1 ? 1 : (nw > 64 ? 64 : nw);
  dsm_or_defer(lane, btab, dsm_cfg(nw, nw, true, 0, 1), false, phase);
  out[9] = okA ? 1u : 0u;
  out[10] = okR ? 1u : 0u;
  out[11] = (uint32_t)nw;
}

// U = [s]B - [c]Y through vrf_u_core (the key's table in slot 2, as the header
// cores place it).  in: the key (0..7), then a proof's 20 words (c at 16..19,
// s at 20..27).  out 9: the key's flag.
constexpr int kUIn = 28;
OURO_HD inline void u_item(const uint32_t* in, uint32_t* out, Slot lane, const int32_t* btab) {
  uint32_t pk[8], pi[20];
#pragma unroll
  for (int k = 0; k < 8; k++) pk[k] = in[k];
#pragma unroll
  for (int k = 0; k < 20; k++) pi[k] = in[8 + k];
  const bool ok = vrf_u_core(pk, pi, true, 2, lane, btab);
  chain_finish(out, lane);
  out[9] = ok ? 1u : 0u;
}

// V = [s]H - [c]Gamma, as vrf03_verify_lane sets it up, H given as an
// encoding.  in: H (0..7), Gamma (8..15), c (16..19), s (20..27).  out 9 / 10:
// H / Gamma decoded.
constexpr int kVIn = 28;
OURO_HD inline void v_item(const uint32_t* in, uint32_t* out, Slot lane, const int32_t* btab) {
  uint32_t He[8], G[8], c[8], s_raw[8], s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    He[k] = in[k];
    G[k] = in[8 + k];
    c[k] = k < 4 ? in[16 + k] : 0u;
    s_raw[k] = in[20 + k];
  }
  ge_p3 Hp, Gamma;
  bool okH, okG;
  ge_decode_pair(&Hp, &okH, &Gamma, &okG, He, G, false);
  sc_reduce256(s, s_raw);
  build_table(lane + kSlotTab1, Hp);
  build_table(lane + kSlotTab2, ge_p3_neg(Gamma));
  st_words8(lane + kSlotA1, s);
  st_words8(lane + kSlotA2, c);
  st_carry(lane, 0, sc_recode_carries<4, 64>(s));
  st_carry(lane, 1, sc_recode_carries<4, 33>(c));
  dsm(lane, btab, dsm_cfg(64, 33, false));
  chain_finish(out, lane);
  out[9] = okH ? 1u : 0u;
  out[10] = okG ? 1u : 0u;
}

// U from the key's table: the header's shared core on item i of a batch whose
// eta proofs carry c and s.  out 9: the key's flag, as the per-key pass left it.
OURO_HD inline void u_table_item(const ouro_tpraos_batch& b, size_t i, bool key_ok, uint32_t* out,
                                 Slot lane, Slot res, const int32_t* ubtab, const int32_t* ytab) {
  hdr_u_shared(b, i, false, key_ok, lane, res, ubtab, ytab);
  chain_finish(out, lane);
  out[9] = key_ok ? 1u : 0u;
}

}  // namespace lt
}  // namespace ouro
