// cbor_witness.h -- the transaction-witness slicer, shared by the host path
// (witness_api.cpp) and the device (kernels_witness.hip k_witness_count /
// k_witness_emit): one block per call, no allocation, no recursion, built on
// cbor.h's head / skip / uint_at / bytes_at.  Acceptance mirrors witness.py
// parse_witnesses item for item (tests/test_block_witnesses.py pins the two
// against each other).
//
// One routine, witness_walk, with a visitor, so the same code runs twice: the
// count pass (WitCount: ntx, nwit) and the emit pass (WitEmit: the tx spans and
// the witness rows at the block's begin offsets).
//
//   block       = [header, txBodies, txWitnesses, txMetadata]   (cbor_block.h's
//                 four encodings; item 0 and item 3 are skipped, not examined)
//   txBodies    = [* map]                  definite or indefinite
//   txWitnesses = [* {uint => any}]        as many elements as txBodies
//     key 0: [* [vkey: bytes(32), sig: bytes(64)]]
//     key 2: [* [vkey: bytes(32), sig: bytes(64), chain_code: bytes(32), attributes]]
//     any other key: skipped; a repeated key is walked again
// An entry's fields are walked first (OURO_PACK_ECBOR), then their types
// (ESHAPE), then their sizes (ESIZE), as pack_fields orders its checks.
#pragma once
#include "cbor.h"

namespace ouro {
namespace cbor {

// a container being read: the items (pairs of a map) still to come, or until a break
struct Seq {
  uint64_t rem;
  bool indef;
};
// the array (want = 4) or map (5) whose head is at i; *j: the index after the head
OURO_HD inline uint8_t seq_open(const Cur& c, uint64_t i, int want, Seq* s, uint64_t* j) {
  int mt;
  uint64_t arg;
  bool ind;
  if (!head(c, i, &mt, &arg, j, &ind)) return OURO_PACK_ECBOR;
  if (mt != want) return OURO_PACK_ESHAPE;
  s->rem = arg;
  s->indef = ind;
  return OURO_PACK_OK;
}
// 1: an item starts at *i; 0: the container has ended (*i is past its break);
// -1: truncated before the break
OURO_HD inline int seq_next(const Cur& c, uint64_t* i, Seq* s) {
  if (s->indef) {
    if (*i >= c.n) return -1;
    if (cb(c, *i) == 0xFF) {
      (*i)++;
      return 0;
    }
    return 1;
  }
  if (s->rem == 0) return 0;
  s->rem--;
  return 1;
}

// V: tx(k, off, len) for the block's k-th tx body (off into raw), then
// wit(t, kind, vk, sig) per witness of the block's t-th transaction, in the
// order the walk meets them.  A visitor is called for items before a later
// error; the caller discards what it gathered unless the status is OK.
template <class V>
OURO_HD inline uint8_t witness_walk(const uint8_t* raw, uint64_t base, uint32_t len, V& v) {
  const Cur c{raw + base, len};
  int mt;
  uint64_t arg, j, tag;
  bool ind;
  // the four block encodings, as cbor_block.h block_one reads them
  if (!head(c, 0, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  if (mt == 6) {
    if (ind || arg != 24) return OURO_PACK_ESHAPE;
    uint64_t k;
    if (!head(c, j, &mt, &arg, &k, &ind)) return OURO_PACK_ECBOR;
    if (mt != 2 || ind) return OURO_PACK_ESHAPE;
    if (c.n - k < arg) return OURO_PACK_ECBOR;   // payload past the span
    if (k + arg != c.n) return OURO_PACK_ECBOR;  // bytes after the block
    if (!head(c, k, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  }
  if (mt != 4 || ind) return OURO_PACK_ESHAPE;
  if (arg == 2) {  // [tag, block]
    uint64_t pos;
    if (!uint_at(c, j, &tag)) return OURO_PACK_ESHAPE;
    if (tag <= 1) return OURO_PACK_EBYRON;
    if (!skip(c, j, &pos)) return OURO_PACK_ECBOR;
    if (!head(c, pos, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 4 || ind) return OURO_PACK_ESHAPE;
  }
  if (arg != 4) return OURO_PACK_ESHAPE;
  uint64_t i;
  if (!skip(c, j, &i)) return OURO_PACK_ECBOR;  // item 0: the header
  // item 1: txBodies
  Seq s;
  uint8_t st;
  if ((st = seq_open(c, i, 4, &s, &i))) return st;
  uint32_t ntx = 0;
  for (;;) {
    const int r = seq_next(c, &i, &s);
    if (r < 0) return OURO_PACK_ECBOR;
    if (!r) break;
    uint64_t k, e;
    if (!head(c, i, &mt, &arg, &k, &ind)) return OURO_PACK_ECBOR;
    if (mt != 5) return OURO_PACK_ESHAPE;
    if (!skip(c, i, &e)) return OURO_PACK_ECBOR;
    v.tx(ntx, base + i, e - i);
    ntx++;
    i = e;
  }
  // item 2: txWitnesses, one set per body (ledger-specs' TxSeq decoder rejects a mismatch)
  if ((st = seq_open(c, i, 4, &s, &i))) return st;
  if (!s.indef && s.rem != ntx) return OURO_PACK_ESHAPE;
  uint32_t t = 0;
  for (;;) {
    const int r = seq_next(c, &i, &s);
    if (r < 0) return OURO_PACK_ECBOR;
    if (!r) break;
    if (t == ntx) return OURO_PACK_ESHAPE;  // more sets than bodies
    Seq m;
    if ((st = seq_open(c, i, 5, &m, &i))) return st;
    for (;;) {
      const int rm = seq_next(c, &i, &m);
      if (rm < 0) return OURO_PACK_ECBOR;
      if (!rm) break;
      uint64_t key, val;
      if (!uint_at(c, i, &key)) return OURO_PACK_ESHAPE;
      if (!skip(c, i, &val)) return OURO_PACK_ECBOR;
      if (key != 0 && key != 2) {
        if (!skip(c, val, &i)) return OURO_PACK_ECBOR;
        continue;
      }
      const int nf = key == 0 ? 2 : 4;
      Seq a;
      if ((st = seq_open(c, val, 4, &a, &i))) return st;
      for (;;) {
        const int ra = seq_next(c, &i, &a);
        if (ra < 0) return OURO_PACK_ECBOR;
        if (!ra) break;
        uint64_t f[5];
        if (!head(c, i, &mt, &arg, &f[0], &ind)) return OURO_PACK_ECBOR;
        if (mt != 4 || ind || arg != (uint64_t)nf) return OURO_PACK_ESHAPE;
        for (int q = 0; q < nf; q++)
          if (!skip(c, f[q], &f[q + 1])) return OURO_PACK_ECBOR;
        const uint8_t *vk, *sg, *cc;
        const int r0 = bytes_at(c, f[0], 32, &vk), r1 = bytes_at(c, f[1], 64, &sg);
        const int r2 = nf == 4 ? bytes_at(c, f[2], 32, &cc) : (int)kBytesOk;
        if (r0 == kBytesShape || r1 == kBytesShape || r2 == kBytesShape) return OURO_PACK_ESHAPE;
        if (r0 | r1 | r2) return OURO_PACK_ESIZE;
        v.wit(t, (uint8_t)key, vk, sg);
        i = f[nf];
      }
    }
    t++;
  }
  if (t != ntx) return OURO_PACK_ESHAPE;  // fewer sets than bodies
  if (!skip(c, i, &i)) return OURO_PACK_ECBOR;  // item 3: the metadata
  if (i != c.n) return OURO_PACK_ECBOR;         // bytes after the block
  return OURO_PACK_OK;
}

// the count pass
struct WitCount {
  uint32_t ntx = 0, nwit = 0;
  OURO_HD void tx(uint32_t, uint64_t, uint64_t) { ntx++; }
  OURO_HD void wit(uint32_t, uint8_t, const uint8_t*, const uint8_t*) { nwit++; }
};
OURO_HD inline uint8_t witness_count_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                         uint32_t* ntx, uint32_t* nwit) {
  WitCount v;
  const uint8_t st = witness_walk(raw, base, len, v);
  *ntx = st == OURO_PACK_OK ? v.ntx : 0;
  *nwit = st == OURO_PACK_OK ? v.nwit : 0;
  return st;
}

// The rows the emit pass fills (on the device: vk and sig 16-byte aligned).
// wit_tx[row] = tx_base + the transaction's row: tx_base is the global row of
// this call's row 0 (a later group of a host-buffer call continues the
// earlier ones).
struct WitRows {
  uint64_t* tx_off;  // per tx row: the body's span in raw
  uint32_t* tx_len;
  uint8_t *vk, *sig;  // per witness row: 32 / 64 bytes
  uint32_t* wit_tx;
  uint8_t* kind;
  uint64_t tx_base;
};
// the emit pass of a block that owns the rows tx0 .. tx0 + ntx and wit0 ..
// wit0 + nwit (the count pass's figures: nothing is written past them)
struct WitEmit {
  WitRows r;
  uint64_t tx0, wit0;
  uint32_t ntx, nwit, w;
  OURO_HD void tx(uint32_t k, uint64_t off, uint64_t n) {
    if (k >= ntx) return;
    stg8(r.tx_off + tx0 + k, off);
    stg1(r.tx_len + tx0 + k, (int32_t)(uint32_t)n);
  }
  OURO_HD void wit(uint32_t t, uint8_t kind, const uint8_t* vk, const uint8_t* sg) {
    if (w >= nwit) return;
    const uint64_t row = wit0 + w++;
    copy_bytes(r.vk + 32 * row, vk, 32);
    copy_bytes(r.sig + 64 * row, sg, 64);
    stg1(r.wit_tx + row, (int32_t)(uint32_t)(r.tx_base + tx0 + t));
    r.kind[row] = kind;
  }
};
OURO_HD inline uint8_t witness_emit_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                        const WitRows& r, uint64_t tx0, uint64_t wit0,
                                        uint32_t ntx, uint32_t nwit) {
  WitEmit v{r, tx0, wit0, ntx, nwit, 0};
  return witness_walk(raw, base, len, v);
}

}  // namespace cbor
}  // namespace ouro
