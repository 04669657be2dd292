// cbor_byron_witness.h -- the Byron transaction-witness slicer, shared by the
// host path (byron_witness_api.cpp) and the device (kernels_byron_witness.hip
// k_byron_witness_count / k_byron_witness_emit): one block per call, no
// allocation, no recursion.  It is cbor_byron_block.h's byron_block_walk with a
// visitor that reads every witness vector.  Acceptance mirrors
// byron_witness.py parse_byron_witnesses item for item
// (tests/test_byron_block_witnesses.py pins the two against each other); that
// file defines the rule.
//
// Everything outside the witness vectors keeps byron_block_walk's acceptance,
// status for status (tag 0: OURO_PACK_EBB, tag >= 2: OURO_PACK_ESHELLEY).
//   witnesses = [* [type: uint, #6.24(bytes .cbor [key: bytes, sig: bytes])]]
//     definite or indefinite; each element a definite array(2); the payload a
//     definite byte string whose content, a definite array(2) of two definite
//     byte strings, ends exactly at the payload's end
//   type 0 (VKWitness): key bytes(64), sig bytes(64)
//   type 2 (RedeemWitness): key bytes(32), sig bytes(64)
// Another type, major type, tag or array length: OURO_PACK_ESHAPE; content
// malformed inside the payload or not ending at its end: OURO_PACK_ECBOR; a
// wrong string length: OURO_PACK_ESIZE -- per witness the content is walked
// first, then the two types, then the two sizes.  The first offending item in
// byte order decides: the visitor keeps its first error, which comes before
// whatever the outer walk meets after that element.
//
// tx id = Blake2b-256 of the tx item as it stands.  A witness signs
//   tag || CBOR(magic) || 0x58 0x20 || tx_id      tag 0x01 (SignTx) for type 0,
//                                                 0x02 (SignRedeemTx) for type 2
// (byron_witness_prefix: the 4 to 8 bytes before the id), verified under
// ByronDSIGN acceptance with XPub[0:32] or the redeem key.
// Pinned by the reference's golden Byron block: the witness vector's shape.
// NOT pinned by any reference fixture (restated from cardano-ledger's
// Cardano.Chain.UTxO.TxWitness and Cardano.Crypto.Signing.Tag): the signed
// message, that the tx id hashes the bytes as they stand, that the redeem kind
// uses ByronDSIGN's acceptance, that an unknown type fails the block's decode.
#pragma once
#include "cbor_byron_block.h"

namespace ouro {
namespace cbor {

constexpr uint8_t kBywVk = 0, kBywRedeem = 2;

// The witness vector c[w, e) (an array, well-formed CBOR: the outer walk has
// skipped it) of the block's t-th transaction.  V: wit(t, kind, key, sig) per
// witness in byte order, key 64 bytes for kind 0 and 32 for kind 2.
template <class V>
OURO_HD inline uint8_t byron_witness_vector(const Cur& c, uint64_t w, uint64_t e, uint32_t t, V& v) {
  const Cur vc{c.b, e};
  Seq s;
  uint64_t i;
  uint8_t st;
  if ((st = seq_open(vc, w, 4, &s, &i))) return st;
  for (;;) {
    const int r = seq_next(vc, &i, &s);
    if (r < 0) return OURO_PACK_ECBOR;
    if (!r) return OURO_PACK_OK;
    int mt;
    uint64_t arg, kind, j;
    bool ind;
    if (!head(vc, i, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 4 || ind || arg != 2) return OURO_PACK_ESHAPE;
    if (!head(vc, j, &mt, &kind, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 0 || ind) return OURO_PACK_ESHAPE;
    if (kind != kBywVk && kind != kBywRedeem) return OURO_PACK_ESHAPE;
    if (!head(vc, j, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 6 || ind || arg != 24) return OURO_PACK_ESHAPE;
    if (!head(vc, j, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 2 || ind) return OURO_PACK_ESHAPE;
    if (vc.n - j < arg) return OURO_PACK_ECBOR;  // (cannot happen after the outer skip)
    const Cur pc{c.b, j + arg};  // the payload bounds its content
    uint64_t k0, k1, k2;
    if (!head(pc, j, &mt, &arg, &k0, &ind)) return OURO_PACK_ECBOR;
    if (mt != 4 || ind || arg != 2) return OURO_PACK_ESHAPE;
    if (!skip(pc, k0, &k1) || !skip(pc, k1, &k2) || k2 != pc.n) return OURO_PACK_ECBOR;
    const uint8_t *key, *sg;
    const int r0 = bytes_at(pc, k0, kind == kBywVk ? 64 : 32, &key), r1 = bytes_at(pc, k1, 64, &sg);
    if (r0 == kBytesShape || r1 == kBytesShape) return OURO_PACK_ESHAPE;
    if (r0 | r1) return OURO_PACK_ESIZE;
    v.wit(t, (uint8_t)kind, key, sg);
    i = pc.n;
  }
}

// the magic field (item 0 of the header) of a regular block byron_block_walk
// accepted: the heads down to it, each known to be there
OURO_HD inline uint64_t byron_block_header_magic(const uint8_t* raw, uint64_t base, uint32_t len) {
  const Cur c{raw + base, len};
  int mt;
  uint64_t arg, j, magic = 0;
  bool ind;
  head(c, 0, &mt, &arg, &j, &ind);
  if (mt == 6) {  // the wire form: the tag, the byte string, [tag, block]
    head(c, j, &mt, &arg, &j, &ind);
    head(c, j, &mt, &arg, &j, &ind);
  }
  head(c, j, &mt, &arg, &j, &ind);  // the block tag (1)
  head(c, j, &mt, &arg, &j, &ind);  // [header, body, extra]
  head(c, j, &mt, &arg, &j, &ind);  // the header's array(5)
  uint_at(c, j, &magic);
  return magic;
}

// the walk with a visitor that has wit(): the outer walk's status unless a
// witness vector had an error before it
template <class W>
struct BywVisit {
  W& w;
  uint8_t err = 0;
  OURO_HD void tx(const Cur& c, uint32_t k, uint64_t a, uint64_t wt, uint64_t e) {
    if (err) return;
    w.tx(k, a, wt - a);
    err = byron_witness_vector(c, wt, e, k, w);
  }
};
template <class W>
OURO_HD inline uint8_t byron_witness_walk(const uint8_t* raw, uint64_t base, uint32_t len, W& w) {
  BywVisit<W> v{w};
  BybInfo bi;
  bi.msg_bytes = 0;
  // (the magic decides only the length of the block's signed message, which
  // nothing here uses)
  const uint8_t st = byron_block_walk<false>(raw, base, len, 0, ByronOut{}, 0, v, &bi);
  return v.err ? v.err : st;
}

// ---- the count pass ----
struct BywCount {
  uint32_t ntx = 0, nwit = 0;
  OURO_HD void tx(uint32_t, uint64_t, uint64_t) { ntx++; }
  OURO_HD void wit(uint32_t, uint8_t, const uint8_t*, const uint8_t*) { nwit++; }
};
OURO_HD inline uint8_t byron_witness_count_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                               uint32_t* ntx, uint32_t* nwit) {
  BywCount v;
  const uint8_t st = byron_witness_walk(raw, base, len, v);
  *ntx = st == OURO_PACK_OK ? v.ntx : 0;
  *nwit = st == OURO_PACK_OK ? v.nwit : 0;
  return st;
}

// ---- the emit pass ----
// The rows it fills (on the device: vk and sig 16-byte aligned).  wit_tx[row] =
// tx_base + the transaction's row, as cbor_witness.h WitRows has it.
struct BywRows {
  uint64_t* tx_off;  // per tx row: the tx item's span in raw
  uint32_t* tx_len;
  uint8_t *vk, *sig;  // per witness row: 64 bytes each (a redeem key then 32 zero bytes)
  uint32_t* wit_tx;
  uint8_t* kind;
  uint64_t tx_base;
};
// the emit pass of a block that owns the rows tx0 .. tx0 + ntx and wit0 ..
// wit0 + nwit (the count pass's figures: nothing is written past them)
struct BywEmit {
  BywRows r;
  uint64_t base, tx0, wit0;
  uint32_t ntx, nwit, w;
  OURO_HD void tx(uint32_t k, uint64_t a, uint64_t n) {
    if (k >= ntx) return;
    stg8(r.tx_off + tx0 + k, base + a);
    stg1(r.tx_len + tx0 + k, (int32_t)(uint32_t)n);
  }
  OURO_HD void wit(uint32_t t, uint8_t kind, const uint8_t* key, const uint8_t* sg) {
    if (w >= nwit) return;
    const uint64_t row = wit0 + w++;
    if (kind == kBywVk) {
      copy_bytes(r.vk + 64 * row, key, 64);
    } else {
      copy_bytes(r.vk + 64 * row, key, 32);
      zero_bytes(r.vk + 64 * row + 32, 32);
    }
    copy_bytes(r.sig + 64 * row, sg, 64);
    stg1(r.wit_tx + row, (int32_t)(uint32_t)(r.tx_base + tx0 + t));
    r.kind[row] = kind;
  }
};
// *magic: the header's own magic field
OURO_HD inline uint8_t byron_witness_emit_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                              const BywRows& r, uint64_t tx0, uint64_t wit0,
                                              uint32_t ntx, uint32_t nwit, uint64_t* magic) {
  BywEmit v{r, base, tx0, wit0, ntx, nwit, 0};
  const uint8_t st = byron_witness_walk(raw, base, len, v);
  if (st == OURO_PACK_OK) *magic = byron_block_header_magic(raw, base, len);
  return st;
}

// ---- the signed message ----
// tag || CBOR(magic) || 0x58 0x20: the bytes before the tx id, left-aligned in
// a big-endian word (byte q = bits 63 - 8q .. 56 - 8q); *pl: how many, 4 to 8
OURO_HD inline uint64_t byron_witness_prefix(uint8_t kind, uint64_t magic, uint32_t* pl) {
  // put_uint's canonical head of a Word32, in arithmetic (no byte array: the
  // verify kernel computes this per lane in registers)
  const uint64_t m = magic & kWord32Max;
  const uint32_t w = m < 24 ? 0u : m < 0x100ull ? 1u : m < 0x10000ull ? 2u : 4u;
  const uint64_t enc = w == 0 ? m : ((uint64_t)(w == 1 ? 24 : w == 2 ? 25 : 26) << (8 * w)) | m;
  const uint32_t n = 4 + w;  // tag, the head byte, w bytes, 0x58 0x20
  const uint64_t p = ((uint64_t)(kind == kBywVk ? 0x01 : 0x02) << (8 * (n - 1))) | (enc << 16) |
                     0x5820ull;
  *pl = n;
  return p << (8 * (8 - n));
}
// the whole message, for the host path: at most 40 bytes; returns its length
inline uint32_t byron_witness_message(uint8_t* d, uint8_t kind, uint64_t magic, const uint8_t* id) {
  uint32_t pl;
  const uint64_t p = byron_witness_prefix(kind, magic, &pl);
  for (uint32_t k = 0; k < pl; k++) d[k] = (uint8_t)(p >> (56 - 8 * k));
  __builtin_memcpy(d + pl, id, 32);
  return pl + 32;
}

}  // namespace cbor
}  // namespace ouro
