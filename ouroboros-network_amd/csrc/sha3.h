// sha3.h -- per-lane SHA3-256 of one short message (FIPS 202) and Byron's key
// hash over it.
//
// Byron's hashVerKey is CC.Common.hashKey (ouroboros-consensus-byron/src/
// Ouroboros/Consensus/Byron/Protocol.hs:35): cardano-crypto-wrapper's
// AbstractHash Blake2b_224 over the SHA3-256 of the key's CBOR encoding, i.e.
//   KH(k) = Blake2b-224(SHA3-256(0x58 0x40 || k))       k: the 64 XPub bytes.
// Pinned end to end by the reference's golden files (tests/test_pbft_rule.py).
// A message of at most 135 bytes is one absorbed block of the 136-byte rate, so
// the sponge is one Keccak-f[1600] permutation.  The 25 state words are only
// ever indexed by literals: on the device they are 50 VGPRs and nothing goes to
// scratch.  Host and device; no allocation.
#pragma once
#include "blake2b.h"
#include "common.h"

namespace ouro {

// rotate left by a compile-time amount (b2b_rotr: two v_alignbit_b32)
template <int N>
OURO_FI uint64_t kk_rotl(uint64_t x) {
  if (N == 0) return x;
  return b2b_rotr(x, 64 - N);
}

// One round on a[0..24] (lane (x, y) is a[x + 5 y]): theta, rho and pi into
// b, chi back into a, iota.
#define OURO_KK_CHI(y)                              \
  a[y + 0] = b[y + 0] ^ (~b[y + 1] & b[y + 2]);     \
  a[y + 1] = b[y + 1] ^ (~b[y + 2] & b[y + 3]);     \
  a[y + 2] = b[y + 2] ^ (~b[y + 3] & b[y + 4]);     \
  a[y + 3] = b[y + 3] ^ (~b[y + 4] & b[y + 0]);     \
  a[y + 4] = b[y + 4] ^ (~b[y + 0] & b[y + 1]);
#define OURO_KK_ROUND(rc)                                        \
  {                                                              \
    const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20];     \
    const uint64_t c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21];     \
    const uint64_t c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22];     \
    const uint64_t c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23];     \
    const uint64_t c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];     \
    const uint64_t d0 = c4 ^ kk_rotl<1>(c1);                     \
    const uint64_t d1 = c0 ^ kk_rotl<1>(c2);                     \
    const uint64_t d2 = c1 ^ kk_rotl<1>(c3);                     \
    const uint64_t d3 = c2 ^ kk_rotl<1>(c4);                     \
    const uint64_t d4 = c3 ^ kk_rotl<1>(c0);                     \
    uint64_t b[25];                                              \
    b[0] = a[0] ^ d0;                                            \
    b[10] = kk_rotl<1>(a[1] ^ d1);                               \
    b[20] = kk_rotl<62>(a[2] ^ d2);                              \
    b[5] = kk_rotl<28>(a[3] ^ d3);                               \
    b[15] = kk_rotl<27>(a[4] ^ d4);                              \
    b[16] = kk_rotl<36>(a[5] ^ d0);                              \
    b[1] = kk_rotl<44>(a[6] ^ d1);                               \
    b[11] = kk_rotl<6>(a[7] ^ d2);                               \
    b[21] = kk_rotl<55>(a[8] ^ d3);                              \
    b[6] = kk_rotl<20>(a[9] ^ d4);                               \
    b[7] = kk_rotl<3>(a[10] ^ d0);                               \
    b[17] = kk_rotl<10>(a[11] ^ d1);                             \
    b[2] = kk_rotl<43>(a[12] ^ d2);                              \
    b[12] = kk_rotl<25>(a[13] ^ d3);                             \
    b[22] = kk_rotl<39>(a[14] ^ d4);                             \
    b[23] = kk_rotl<41>(a[15] ^ d0);                             \
    b[8] = kk_rotl<45>(a[16] ^ d1);                              \
    b[18] = kk_rotl<15>(a[17] ^ d2);                             \
    b[3] = kk_rotl<21>(a[18] ^ d3);                              \
    b[13] = kk_rotl<8>(a[19] ^ d4);                              \
    b[14] = kk_rotl<18>(a[20] ^ d0);                             \
    b[24] = kk_rotl<2>(a[21] ^ d1);                              \
    b[9] = kk_rotl<61>(a[22] ^ d2);                              \
    b[19] = kk_rotl<56>(a[23] ^ d3);                             \
    b[4] = kk_rotl<14>(a[24] ^ d4);                              \
    OURO_KK_CHI(0)                                               \
    OURO_KK_CHI(5)                                               \
    OURO_KK_CHI(10)                                              \
    OURO_KK_CHI(15)                                              \
    OURO_KK_CHI(20)                                              \
    a[0] ^= (rc);                                                \
  }

// Keccak-f[1600]: 24 rounds, unrolled, the round constants as literals
OURO_FI void keccak_f1600(uint64_t a[25]) {
  OURO_KK_ROUND(0x0000000000000001ULL)
  OURO_KK_ROUND(0x0000000000008082ULL)
  OURO_KK_ROUND(0x800000000000808aULL)
  OURO_KK_ROUND(0x8000000080008000ULL)
  OURO_KK_ROUND(0x000000000000808bULL)
  OURO_KK_ROUND(0x0000000080000001ULL)
  OURO_KK_ROUND(0x8000000080008081ULL)
  OURO_KK_ROUND(0x8000000000008009ULL)
  OURO_KK_ROUND(0x000000000000008aULL)
  OURO_KK_ROUND(0x0000000000000088ULL)
  OURO_KK_ROUND(0x0000000080008009ULL)
  OURO_KK_ROUND(0x000000008000000aULL)
  OURO_KK_ROUND(0x000000008000808bULL)
  OURO_KK_ROUND(0x800000000000008bULL)
  OURO_KK_ROUND(0x8000000000008089ULL)
  OURO_KK_ROUND(0x8000000000008003ULL)
  OURO_KK_ROUND(0x8000000000008002ULL)
  OURO_KK_ROUND(0x8000000000000080ULL)
  OURO_KK_ROUND(0x000000000000800aULL)
  OURO_KK_ROUND(0x800000008000000aULL)
  OURO_KK_ROUND(0x8000000080008081ULL)
  OURO_KK_ROUND(0x8000000000008080ULL)
  OURO_KK_ROUND(0x0000000080000001ULL)
  OURO_KK_ROUND(0x8000000080008008ULL)
}
#undef OURO_KK_ROUND
#undef OURO_KK_CHI

// out = SHA3-256 of the first `len` <= 135 bytes of in (34 little-endian 32-bit
// words, the 136-byte rate; bytes past len must be zero): the domain byte 0x06
// after the message, 0x80 into byte 135, one permutation.  The pad word is
// placed by a compare per word, never by an index, so a runtime len costs 34
// selects and no scratch.  out[0..7]: the digest as little-endian words.
OURO_FI void sha3_256_short(uint32_t out[8], const uint32_t in[34], uint32_t len) {
  const uint32_t pad_word = len >> 2, pad = 0x06u << (8 * (len & 3));
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 17; i++) {
    const uint32_t lo = in[2 * i] ^ (pad_word == (uint32_t)(2 * i) ? pad : 0u);
    const uint32_t hi = in[2 * i + 1] ^ (pad_word == (uint32_t)(2 * i + 1) ? pad : 0u);
    a[i] = (uint64_t)lo | ((uint64_t)hi << 32);
  }
  a[16] ^= 0x8000000000000000ULL;
#pragma unroll
  for (int i = 17; i < 25; i++) a[i] = 0;
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[2 * i] = (uint32_t)a[i];
    out[2 * i + 1] = (uint32_t)(a[i] >> 32);
  }
}

// Byron's hashKey of an XPub: out[0..6] = the 28 bytes of
// Blake2b-224(SHA3-256(58 40 || xpub)) as little-endian words.  xpub: 64 bytes
// (4-byte aligned on the device).
OURO_FI void byron_key_hash(uint32_t out[7], const uint8_t* xpub) {
  uint32_t m[34];
  uint32_t prev = 0x4058u;  // the CBOR head of bytes(64), then the key shifted by two bytes
#pragma unroll
  for (int w = 0; w < 16; w++) {
    const uint32_t x = (uint32_t)ldg1(xpub + 4 * w);
    m[w] = prev | (x << 16);
    prev = x >> 16;
  }
  m[16] = prev;
#pragma unroll
  for (int w = 17; w < 34; w++) m[w] = 0;
  uint32_t in[16];
  sha3_256_short(in, m, 66);
#pragma unroll
  for (int w = 8; w < 16; w++) in[w] = 0;
  blake2b224_short(out, in, 32);
}

}  // namespace ouro
