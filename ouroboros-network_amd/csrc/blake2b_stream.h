// blake2b_stream.h -- per-lane unkeyed Blake2b-256 (RFC 7693) of a span of any
// length up to 2^32 - 1: the block body hash (cbor_block.h; ledger-specs
// bbHash, SURVEY.md §3.3 blockMatchesHeader) and the generic batched hash
// (ouro_blake2b256_batch).  blake2b.h's blake2b256_short stays the one-block
// routine of the KES Merkle pairs, mkSeed and the nonce hashes.
//
// Full 128-byte blocks run with the running byte counter; the final block
// (the last 1..128 bytes, or the empty message's 0) is zero padded and carries
// the last-block flag.  One copy of the compression: the block loop ends on
// the final block.
#pragma once
#include "blake2b.h"

namespace ouro {

constexpr uint64_t kB2bIV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};

// h <- F(h, m, t, last): t = bytes hashed so far, this block's included
OURO_FI void b2b_compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = h[i];
    v[i + 8] = kB2bIV[i];
  }
  v[12] ^= t;  // (t1 = 0: spans are shorter than 2^32)
  if (last) v[14] = ~v[14];
#define OURO_B2G(a, b, c, d, x, y)                     \
  v[a] = v[a] + v[b] + (x);                            \
  v[d] = b2b_rotr(v[d] ^ v[a], 32);                    \
  v[c] = v[c] + v[d];                                  \
  v[b] = b2b_rotr(v[b] ^ v[c], 24);                    \
  v[a] = v[a] + v[b] + (y);                            \
  v[d] = b2b_rotr(v[d] ^ v[a], 16);                    \
  v[c] = v[c] + v[d];                                  \
  v[b] = b2b_rotr(v[b] ^ v[c], 63);
#pragma unroll
  for (int r = 0; r < 12; r++) {
    const uint8_t* s = kB2bSigma[r];
    OURO_B2G(0, 4, 8, 12, m[s[0]], m[s[1]])
    OURO_B2G(1, 5, 9, 13, m[s[2]], m[s[3]])
    OURO_B2G(2, 6, 10, 14, m[s[4]], m[s[5]])
    OURO_B2G(3, 7, 11, 15, m[s[6]], m[s[7]])
    OURO_B2G(0, 5, 10, 15, m[s[8]], m[s[9]])
    OURO_B2G(1, 6, 11, 12, m[s[10]], m[s[11]])
    OURO_B2G(2, 7, 8, 13, m[s[12]], m[s[13]])
    OURO_B2G(3, 4, 9, 14, m[s[14]], m[s[15]])
  }
#undef OURO_B2G
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}

// The low 32 bits of (next:prev) >> sh, sh in {0, 8, 16, 24}: v_alignbit_b32
OURO_FI uint32_t b2b_funnel(uint32_t next, uint32_t prev, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(next, prev, sh);
#else
  return (uint32_t)((((uint64_t)next << 32) | prev) >> sh);
#endif
}

// m <- the `take` <= 128 bytes at address a, zero padded, read as the aligned
// dwords that cover them and funnel-shifted by (a & 3): 33 dword loads for a
// full block instead of 128 byte loads.  ld(address) loads one aligned dword.
// Every dword read starts before a + take and ends after a, i.e. holds at
// least one byte of the span being hashed: nothing outside the dwords the
// span touches is read.  The device entries demand a 4-byte aligned buffer,
// so the first of those dwords starts inside it; the last one ends up to 3
// bytes past a span that ends at a buffer end which is no multiple of 4, so
// they also demand an allocation that extends to the next multiple of 4.
// tests/test_devcode_blake2b.py runs this routine on the host with a loader
// that checks exactly that rule.
template <class Ld>
OURO_FI void b2b_load_dwords(uint64_t m[16], uintptr_t a, uint32_t take, Ld ld) {
  const uintptr_t w0 = a & ~uintptr_t(3);
  const uint32_t mis = (uint32_t)(a & 3), sh = mis * 8;
  uint32_t w[32];
  // (take == 0: the empty message; no dword holds a byte of it)
  uint32_t prev = take ? ld(w0) : 0u;
#pragma unroll
  for (int k = 0; k < 32; k++) {
    // the dword after word k's first: read iff it starts before a + take
    const bool need = (uint32_t)(4 * k + 4) < take + mis;
    const uint32_t next = need ? ld(w0 + (uintptr_t)(4 * k + 4)) : 0u;
    uint32_t x = b2b_funnel(next, prev, sh);
    // the final block: bytes at and past `take` are padding
    const uint32_t lo = (uint32_t)(4 * k);
    if (lo >= take) x = 0;
    else if (take - lo < 4) x &= (1u << (8 * (take - lo))) - 1u;
    w[k] = x;
    prev = next;
  }
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

// m <- the `take` <= 128 bytes at p, zero padded.  Device: spans start at any
// byte address, so the block goes through b2b_load_dwords.  Host: memcpy (any
// alignment, nothing past the span).
OURO_FI void b2b_load_block(uint64_t m[16], const uint8_t* p, uint32_t take) {
#if defined(__HIP_DEVICE_COMPILE__)
  b2b_load_dwords(m, reinterpret_cast<uintptr_t>(p), take, [](uintptr_t x) {
    return (uint32_t)ldg1(reinterpret_cast<const void*>(x));
  });
#else
  uint8_t b[128];
  __builtin_memset(b, 0, sizeof b);
  if (take) __builtin_memcpy(b, p, take);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    uint64_t x = 0;
    for (int k = 7; k >= 0; k--) x = (x << 8) | b[8 * i + k];
    m[i] = x;
  }
#endif
}

// out (8 little-endian words) = Blake2b-256(msg[0 .. len))
OURO_HD inline void blake2b256_stream(uint32_t out[8], const uint8_t* msg, uint32_t len) {
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = kB2bIV[i];
  h[0] ^= 0x01010000ULL ^ 32;  // digest length 32, key length 0, fanout 1, depth 1
  const uint8_t* p = msg;
  uint32_t left = len;
  uint64_t t = 0;
  for (;;) {
    const bool last = left <= 128;
    const uint32_t take = last ? left : 128u;
    uint64_t m[16];
    b2b_load_block(m, p, take);
    t += take;
    b2b_compress(h, m, t, last);
    if (last) break;
    p += take;
    left -= take;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}

// out = Blake2b-256(pre ‖ msg[0 .. len)): npre <= 2 prefix bytes (pre: the
// first in bits 0..7, the second in bits 8..15) in front of a span, the header
// hash of a Byron header (envelope.h: 0x82, kind, then the header item).
// Block b of the hashed message covers the span's bytes
// [128 b - npre, 128 b + 128 - npre): the first block loads its 128 - npre
// span bytes (or fewer) as any other block does and shifts the prefix in;
// every later block is a plain load from a span address.  Each load is
// b2b_load_block over a piece of the span, so its rule -- every dword read
// holds at least one byte of the span -- holds here as it does there
// (tests/test_devcode_prefixed_blake2b.py drives b2b_prefixed_with through
// b2b_load_dwords and a loader that checks it).  len + npre < 2^32.
// load(m, p, take): m <- the `take` <= 128 bytes at p, zero padded.
template <class LoadBlock>
OURO_FI void b2b_prefixed_with(uint32_t out[8], uint32_t pre, uint32_t npre, const uint8_t* msg,
                               uint32_t len, LoadBlock load) {
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = kB2bIV[i];
  h[0] ^= 0x01010000ULL ^ 32;
  const uint8_t* p = msg;
  uint32_t left = len + npre, skip = npre;
  uint64_t t = 0;
  for (;;) {
    const bool last = left <= 128;
    const uint32_t blk = last ? left : 128u, take = blk - skip;
    uint64_t m[16];
    load(m, p, take);
    if (skip) {  // the first block: the span's bytes move up behind the prefix
      const uint32_t sh = 8 * skip;
#pragma unroll
      for (int i = 15; i > 0; i--) m[i] = (m[i] << sh) | (m[i - 1] >> (64 - sh));
      m[0] = (m[0] << sh) | (uint64_t)(pre & ((1u << sh) - 1u));
    }
    t += blk;
    b2b_compress(h, m, t, last);
    if (last) break;
    p += take;
    left -= blk;
    skip = 0;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}
OURO_HD inline void blake2b256_stream_prefixed(uint32_t out[8], uint32_t pre, uint32_t npre,
                                               const uint8_t* msg, uint32_t len) {
  b2b_prefixed_with(out, pre, npre, msg, len,
                    [](uint64_t m[16], const uint8_t* p, uint32_t take) { b2b_load_block(m, p, take); });
}

// Blake2b-256 of 96 bytes held as 24 little-endian words: one final
// compression with t = 96 (the block body hash over its three segment digests)
OURO_FI void blake2b256_96(uint32_t out[8], const uint32_t in[24]) {
  uint64_t h[8], m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = kB2bIV[i];
  h[0] ^= 0x01010000ULL ^ 32;
#pragma unroll
  for (int i = 0; i < 12; i++) m[i] = (uint64_t)in[2 * i] | ((uint64_t)in[2 * i + 1] << 32);
#pragma unroll
  for (int i = 12; i < 16; i++) m[i] = 0;
  b2b_compress(h, m, 96, true);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    out[2 * i] = (uint32_t)h[i];
    out[2 * i + 1] = (uint32_t)(h[i] >> 32);
  }
}

}  // namespace ouro
