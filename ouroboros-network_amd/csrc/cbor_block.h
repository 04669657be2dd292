// cbor_block.h -- the Shelley-family BLOCK slicer, shared by the host path and
// the device (kernels.hip k_block_pack): one block per call, no allocation, no
// recursion, built on cbor.h's head / skip and its header field extraction
// (pack_fields).  Acceptance mirrors block.py parse_block item for item
// (tests/test_block_integrity.py pins the two against each other).
//
// Block encodings (the reference's golden files):
//   block          = [header, txBodies, txWitnesses, txMetadata]    Shelley on disk
//   wire_block     = #6.24(bytes .cbor block)                       Shelley on the wire
//   hfc_block      = [tag, block]                                   Cardano on disk
//   hfc_wire_block = #6.24(bytes .cbor [tag, block])                Cardano on the wire
//   header         = [header_body, kes_sig]      (plain: NOT tag-24 wrapped in a block)
// For blocks the HFC tag is 0 = Byron EBB, 1 = Byron regular, 2 and up =
// Shelley family (the header wire form differs: there 0 is Byron, 1 and up
// Shelley).  Byron blocks (status OURO_PACK_EBYRON) are out of scope: their
// blockMatchesHeader checks a body proof, not a body hash.
//
// blockMatchesHeader (ouroboros-consensus-shelley/src/Ouroboros/Consensus/
// Shelley/Ledger/Block.hs:127-130) compares ledger-specs bbHash with the
// header body's field 8:
//   bbHash = Blake2b-256(Blake2b-256(txBodies) || Blake2b-256(txWitnesses)
//                        || Blake2b-256(txMetadata))
// each inner hash over the item's bytes exactly as they stand in the block
// (CBOR head included; the reference keeps them through its Annotator), so the
// slicer records the three spans and the claimed hash, nothing else.
#pragma once
#include "cbor.h"

namespace ouro {
namespace cbor {

// per block: the claimed bodyHash (32 B, 16-byte aligned rows) and the spans
// of items 1..3 (offsets into raw)
struct BlockOut {
  uint8_t* claimed;   // n x 32
  uint64_t* seg_off;  // 3n
  uint32_t* seg_len;  // 3n
};

OURO_HD inline uint8_t block_one(const uint8_t* raw, uint64_t base, uint32_t len, uint64_t spkp,
                                 const Out& o, const BlockOut& bo, size_t i) {
  Cur c{raw + base, len};
  int mt;
  uint64_t arg, j, pos = 0, tag = 2;
  bool ind;
  if (!head(c, 0, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  if (mt == 6) {  // the wire forms: #6.24(bytes .cbor ...), as pack_one reads a header's
    if (ind || arg != 24) return OURO_PACK_ESHAPE;
    uint64_t k;
    if (!head(c, j, &mt, &arg, &k, &ind)) return OURO_PACK_ECBOR;
    if (mt != 2 || ind) return OURO_PACK_ESHAPE;
    if (c.n - k < arg) return OURO_PACK_ECBOR;   // payload past the span
    if (k + arg != c.n) return OURO_PACK_ECBOR;  // bytes after the block
    pos = k;                                     // (the payload ends where the span does)
    if (!head(c, pos, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  }
  if (mt != 4 || ind) return OURO_PACK_ESHAPE;
  if (arg == 2) {  // [tag, block]
    if (!uint_at(c, j, &tag)) return OURO_PACK_ESHAPE;
    if (tag <= 1) return OURO_PACK_EBYRON;
    if (!skip(c, j, &pos)) return OURO_PACK_ECBOR;
    if (!head(c, pos, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
    if (mt != 4 || ind) return OURO_PACK_ESHAPE;
  }
  if (arg != 4) return OURO_PACK_ESHAPE;
  // item 0: the header (the HFC block tag is one above the header era)
  uint64_t p, f8;
  const uint8_t st = pack_fields(c, j, base, tag - 1, spkp, o, i, kAnyEnd, &p, &f8);
  if (st != OURO_PACK_OK) return st;
  const uint8_t* bh;
  const int rb = bytes_at(c, f8, 32, &bh);
  if (rb == kBytesShape) return OURO_PACK_ESHAPE;
  if (rb == kBytesSize) return OURO_PACK_ESIZE;
  // items 1..3: txBodies, txWitnesses, txMetadata as they stand
  uint64_t so[3], sl[3];
  for (int s = 0; s < 3; s++) {
    uint64_t q;
    if (!skip(c, p, &q)) return OURO_PACK_ECBOR;
    so[s] = base + p;
    sl[s] = q - p;
    p = q;
  }
  if (p != c.n) return OURO_PACK_ECBOR;  // bytes after the block
  copy_bytes(bo.claimed + 32 * i, bh, 32);
  for (int s = 0; s < 3; s++) {
    bo.seg_off[3 * i + s] = so[s];
    bo.seg_len[3 * i + s] = (uint32_t)sl[s];
  }
  return OURO_PACK_OK;
}

OURO_HD inline void block_zero_row(const Out& o, const BlockOut& bo, size_t i) {
  zero_row(o, i);
  zero_bytes(bo.claimed + 32 * i, 32);
  for (int s = 0; s < 3; s++) {
    bo.seg_off[3 * i + s] = 0;
    bo.seg_len[3 * i + s] = 0;
  }
}

// The arena of ouro_block_integrity_verify_cbor_device (ouro_block_pack_bytes):
// the TPraos header arena (layout(n)), then -- each 64-byte aligned -- the
// claimed hashes (32n), the segment offsets (24n) and lengths (12n), the 3n
// segment digests (96n), the KES verdicts (n), and the hash work area of 3n
// items (b2b_work_bytes).
constexpr int kB2bClasses = 27;  // bit length of a compression count <= 2^25: 0..26
inline size_t a64(size_t x) { return (x + 63) & ~(size_t)63; }
// the hash work area of m items: the work permutation (4m) and its class
// counters (2 x 32 words: counts, then running starts)
inline size_t b2b_work_bytes(size_t m) { return a64(4 * m) + 256 + 64; }
struct BlockLayout {
  size_t hdr, claimed, seg_off, seg_len, digest, kes, work, total;
};
inline BlockLayout block_layout(size_t n) {
  BlockLayout l{};
  size_t at = 0;
  l.hdr = at;
  at += a64(layout(n).total);
  l.claimed = at;
  at += a64(32 * n);
  l.seg_off = at;
  at += a64(24 * n);
  l.seg_len = at;
  at += a64(12 * n);
  l.digest = at;
  at += a64(96 * n);
  l.kes = at;
  at += a64(n);
  l.work = at;
  at += b2b_work_bytes(3 * n);
  l.total = at;
  return l;
}
inline BlockOut block_arena_out(uint8_t* a, const BlockLayout& l) {
  return BlockOut{a + l.claimed, reinterpret_cast<uint64_t*>(a + l.seg_off),
                  reinterpret_cast<uint32_t*>(a + l.seg_len)};
}

}  // namespace cbor
}  // namespace ouro
