// synth.h -- signing-side lane routines used ONLY to synthesise benchmark and
// test inputs on the device (Ed25519 keygen/sign, draft-03 VRF prove, Sum6KES
// leaf keys).  Not part of the verifier ABI; the forging side is out of scope
// for the hot path.  Deterministic, so tests pin these
// against the oracle's signer byte for byte.  The VRF prover and the scalar
// multiplications under it are the product's (prove.h), one copy.
#pragma once
#include "prove.h"

namespace ouro {

// Ed25519 signature of a message (register prefix-free tail source)
template <class Tail>
OURO_FI void ed25519_sign_lane(uint32_t sig[16], const ExpandedKey& k, const Tail& msg,
                               uint32_t mlen, Slot lane, const int32_t* btab) {
  uint64_t H[8];
  uint32_t hw[16], r[8], h[8];
  sha512_prefixed<32>(H, k.prefix, msg, mlen);
  sha512_digest_words(hw, H);
  sc_reduce512(r, hw);
  uint32_t R[8];
  encode_p2(R, base_mul(r, lane, btab));
  uint32_t pre[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    pre[i] = R[i];
    pre[8 + i] = k.pk[i];
  }
  sha512_prefixed<64>(H, pre, msg, mlen);
  sha512_digest_words(hw, H);
  sc_reduce512(h, hw);
  uint32_t S[8];
  sc_muladd(S, h, k.a, r);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] = R[i];
    sig[8 + i] = S[i];
  }
}

}  // namespace ouro
