// cbor_byron_block.h -- the Byron BLOCK slicer, shared by the host path
// (byron_block_api.cpp) and the device (kernels_byron_block.hip
// k_byron_block_count / k_byron_block_emit): one block per call, no allocation,
// no recursion, built on cbor.h's head / skip, cbor_witness.h's container
// reader and cbor_byron.h's header fields (byron_fields).  Acceptance mirrors
// byron_block.py parse_byron_block item for item
// (tests/test_byron_block_integrity.py pins the two against each other).
//
// verifyBlockIntegrity cfg blk = verifyHeaderIntegrity cfg hdr &&
// blockMatchesHeader hdr blk (ouroboros-consensus-byron/src/Ouroboros/
// Consensus/Byron/Ledger/Integrity.hs:63-68); blockMatchesHeader is
// CC.abobMatchesBody (Byron/Ledger/Block.hs:167-168): the header's body proof
// against the proof recomputed from the body, True for an EBB.
//
// Block forms (cbor_block.h's, with Byron tags):
//   [tag, block]                         on disk (Byron-only and Cardano alike)
//   #6.24(bytes .cbor [tag, block])      on the wire
// tag 0 = EBB (skipped; it must end at the span: OURO_PACK_EBB), 1 = regular,
// 2 and up = Shelley family (OURO_PACK_ESHELLEY).
//   regular = [header, body, extra]                       definite array(3)
//   header  = [magic, prevHash, proof, consensusData, extraData]   (plain)
//   proof   = [[txpNumber, txpRoot, txpWitnessesHash], [sscTag, sscHash],
//              dlgHash, updHash]
//   body    = [txPayload, sscPayload, dlgPayload, updPayload]   definite array(4)
//   txPayload = [* [tx, witnesses]]      definite or indefinite; each element a
//               definite array(2) of two arrays, recorded as they stand
// The block must end exactly where its span ends.
//
// The recomputed proof, every hash Blake2b-256 over bytes as they stand:
//   leaf_k = H(0x00 || tx_k), node(l, r) = H(0x01 || l || r); the root of n
//   leaves is H("") for n = 0, the leaf for n = 1, else node(root(first i),
//   root(rest)) with i the largest power of two strictly below n;
//   txpNumber = n; txpWitnessesHash = H(0x9f || witnesses_0 || ... || 0xff);
//   dlgHash = H(dlgPayload); updHash = H(updPayload).  The SSC proof is not
//   compared (the reference's SscProof is a unit): only [uint, bytes(32)] is
//   demanded of it.
// Pinned by the reference's golden Byron block: the leaf form, the witnesses
// list form and the two payload hashes.  NOT pinned by any reference fixture
// (restated from cardano-ledger's Cardano.Chain.Common.Merkle and its Byron
// block decoder): the tree shape for n >= 2 and the empty root; non-canonical
// or indefinite encodings inside a witness vector (the reference may
// re-serialise there, this slicer hashes the bytes as they stand); that the
// SSC proof's content is ignored.  The transaction witnesses are verified by
// cbor_byron_witness.h's visitors over this walk, not here.
#pragma once
#include "blake2b_stream.h"
#include "cbor_byron.h"
#include "cbor_witness.h"

namespace ouro {
namespace cbor {

// what the walk learns about a regular block besides its transactions
struct BybInfo {
  uint64_t tx_num;            // the proof's txpNumber
  const uint8_t* claimed[4];  // txpRoot, txpWitnessesHash, dlgHash, updHash (32 bytes each)
  uint64_t seg_s[2], seg_e[2];  // dlgPayload and updPayload, indices into the block's span
  uint32_t msg_bytes;         // the length of the signed message
};

// V: tx(c, k, tx, wit, end) for the block's k-th transaction: tx is c[tx, wit),
// its witness vector c[wit, end).  A visitor is called for items before a later
// error; the caller discards what it gathered unless the status is OK.
// kRows: row i of `o` is written as byron_pack_one writes it (the emit pass of
// a block the count pass accepted).
template <bool kRows, class V>
OURO_HD inline uint8_t byron_block_walk(const uint8_t* raw, uint64_t base, uint32_t len,
                                        int64_t magic_cfg, const ByronOut& o, size_t i, V& v,
                                        BybInfo* bi) {
  const Cur c{raw + base, len};
  int mt;
  uint64_t arg, j, tag, pos;
  bool ind;
  uint8_t st;
  if (!head(c, 0, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  if (mt == 6) {  // the wire form, as cbor_block.h block_one reads it
    if (ind || arg != 24) return OURO_PACK_ESHAPE;
    uint64_t k;
    if (!head(c, j, &mt, &arg, &k, &ind)) return OURO_PACK_ECBOR;
    if (mt != 2 || ind) return OURO_PACK_ESHAPE;
    if (c.n - k < arg) return OURO_PACK_ECBOR;   // payload past the span
    if (k + arg != c.n) return OURO_PACK_ECBOR;  // bytes after the block
    if (!head(c, k, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  }
  if (mt != 4 || ind || arg != 2) return OURO_PACK_ESHAPE;  // [tag, block]
  if (!uint_at(c, j, &tag)) return OURO_PACK_ESHAPE;
  if (tag >= 2) return OURO_PACK_ESHELLEY;
  if (!skip(c, j, &pos)) return OURO_PACK_ECBOR;
  if (tag == 0) {  // an EBB: no signature and no proof to match
    uint64_t e;
    if (!skip(c, pos, &e)) return OURO_PACK_ECBOR;
    return e == c.n ? OURO_PACK_EBB : OURO_PACK_ECBOR;
  }
  if (!head(c, pos, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  if (mt != 4 || ind || arg != 3) return OURO_PACK_ESHAPE;
  // item 0: the header, then its proof
  uint64_t p, pr[2];
  if ((st = byron_fields<kRows>(c, j, base, magic_cfg, o, i, nullptr, 0, kAnyEnd, &p, pr,
                                &bi->msg_bytes)))
    return st;
  uint64_t ps[4], pe[4], ts[3], te[3], ss[2], se[2], ssc_tag;
  if ((st = fixed_array(c, pr[0], ps, pe, 4))) return st;
  if ((st = fixed_array(c, ps[0], ts, te, 3))) return st;
  if ((st = fixed_array(c, ps[1], ss, se, 2))) return st;
  if (!uint_le(c, ts[0], kWord32Max, &bi->tx_num) || !uint_at(c, ss[0], &ssc_tag))
    return OURO_PACK_ESHAPE;
  const uint8_t* ssc;
  const int r0 = bytes_at(c, ts[1], 32, &bi->claimed[0]), r1 = bytes_at(c, ts[2], 32, &bi->claimed[1]),
            r2 = bytes_at(c, ss[1], 32, &ssc), r3 = bytes_at(c, ps[2], 32, &bi->claimed[2]),
            r4 = bytes_at(c, ps[3], 32, &bi->claimed[3]);
  if (r0 == kBytesShape || r1 == kBytesShape || r2 == kBytesShape || r3 == kBytesShape ||
      r4 == kBytesShape)
    return OURO_PACK_ESHAPE;
  if (r0 | r1 | r2 | r3 | r4) return OURO_PACK_ESIZE;
  // item 1: the body
  if (!head(c, p, &mt, &arg, &j, &ind)) return OURO_PACK_ECBOR;
  if (mt != 4 || ind || arg != 4) return OURO_PACK_ESHAPE;
  Seq s;
  if ((st = seq_open(c, j, 4, &s, &p))) return st;  // txPayload
  uint32_t ntx = 0;
  for (;;) {
    const int r = seq_next(c, &p, &s);
    if (r < 0) return OURO_PACK_ECBOR;
    if (!r) break;
    uint64_t a, w, e;
    int m1;
    if (!head(c, p, &mt, &arg, &a, &ind)) return OURO_PACK_ECBOR;
    if (mt != 4 || ind || arg != 2) return OURO_PACK_ESHAPE;
    if (!head(c, a, &m1, &arg, &w, &ind)) return OURO_PACK_ECBOR;
    if (m1 != 4) return OURO_PACK_ESHAPE;
    if (!skip(c, a, &w)) return OURO_PACK_ECBOR;
    if (!head(c, w, &m1, &arg, &e, &ind)) return OURO_PACK_ECBOR;
    if (m1 != 4) return OURO_PACK_ESHAPE;
    if (!skip(c, w, &e)) return OURO_PACK_ECBOR;
    v.tx(c, ntx, a, w, e);
    ntx++;
    p = e;
  }
  if (!skip(c, p, &p)) return OURO_PACK_ECBOR;  // sscPayload
  for (int q = 0; q < 2; q++) {                 // dlgPayload, updPayload
    bi->seg_s[q] = p;
    if (!skip(c, p, &p)) return OURO_PACK_ECBOR;
    bi->seg_e[q] = p;
  }
  if (!skip(c, p, &p)) return OURO_PACK_ECBOR;  // item 2: the extra data
  if (p != c.n) return OURO_PACK_ECBOR;         // bytes after the block
  return OURO_PACK_OK;
}

// ---- the count pass ----
// ntx, the gathered witness bytes (the witness spans + the 0x9f and 0xff
// around them) and the message length; zeros unless the status is OK
struct BybCount {
  uint32_t ntx = 0;
  uint64_t wit = 0;
  OURO_HD void tx(const Cur&, uint32_t, uint64_t, uint64_t w, uint64_t e) {
    ntx++;
    wit += e - w;
  }
};
OURO_HD inline uint8_t byron_block_count_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                             int64_t magic_cfg, uint32_t* ntx, uint32_t* gather,
                                             uint32_t* msg) {
  BybCount v;
  BybInfo bi;
  bi.msg_bytes = 0;
  const uint8_t st = byron_block_walk<false>(raw, base, len, magic_cfg, ByronOut{}, 0, v, &bi);
  const bool ok = st == OURO_PACK_OK;
  *ntx = ok ? v.ntx : 0;
  *gather = ok ? (uint32_t)(v.wit + 2) : 0;  // (the spans lie inside len < 2^32 bytes with > 2 to spare)
  *msg = ok ? bi.msg_bytes : 0;
  return st;
}

// ---- the emit pass ----
// The rows it fills, beside the block's Byron row (ByronOut): per block the
// four claimed hashes (128 bytes, 16-byte aligned rows), txpNumber, the dlg and
// upd spans and the span of its gathered witness list; per transaction row the
// tx span (offsets into raw); the gather area.
struct BybRows {
  uint8_t* claimed;   // n x 128: txpRoot | txpWitnessesHash | dlgHash | updHash
  uint32_t* tx_num;   // n
  uint64_t* seg_off;  // 2n: dlgPayload, updPayload
  uint32_t* seg_len;  // 2n
  uint64_t* g_off;    // n: the block's list in the gather area
  uint32_t* g_len;    // n
  uint64_t* tx_off;   // per tx row
  uint32_t* tx_len;
  uint8_t* gather;
};
// the emit pass of a block that owns the tx rows tx0 .. tx0 + ntx and the
// gather bytes g0 .. g0 + gbytes (the count pass's figures: nothing is written
// past them)
struct BybEmit {
  BybRows r;
  uint64_t base, tx0, g0;
  uint32_t ntx, gbytes, g;
  OURO_HD void tx(const Cur& c, uint32_t k, uint64_t a, uint64_t w, uint64_t e) {
    if (k >= ntx) return;
    stg8(r.tx_off + tx0 + k, base + a);
    stg1(r.tx_len + tx0 + k, (int32_t)(uint32_t)(w - a));
    if (e - w > (uint64_t)gbytes || (uint64_t)g + 1 > (uint64_t)gbytes - (e - w)) return;
    g += (uint32_t)put_span(r.gather + g0 + g, c, w, e);
  }
};
OURO_HD inline uint8_t byron_block_emit_one(const uint8_t* raw, uint64_t base, uint32_t len,
                                            int64_t magic_cfg, const ByronOut& o, const BybRows& r,
                                            size_t i, uint64_t tx0, uint64_t g0, uint32_t ntx,
                                            uint32_t gbytes) {
  BybEmit v{r, base, tx0, g0, ntx, gbytes, 1};
  BybInfo bi;
  if (gbytes >= 2) r.gather[g0] = 0x9f;
  const uint8_t st = byron_block_walk<true>(raw, base, len, magic_cfg, o, i, v, &bi);
  if (st != OURO_PACK_OK) return st;
  if (gbytes >= 2 && v.g + 1 == gbytes) r.gather[g0 + v.g] = 0xff;
  for (int q = 0; q < 4; q++) copy_bytes(r.claimed + 128 * i + 32 * q, bi.claimed[q], 32);
  stg1(r.tx_num + i, (int32_t)(uint32_t)bi.tx_num);
  for (int q = 0; q < 2; q++) {
    stg8(r.seg_off + 2 * i + q, base + bi.seg_s[q]);
    stg1(r.seg_len + 2 * i + q, (int32_t)(uint32_t)(bi.seg_e[q] - bi.seg_s[q]));
  }
  stg8(r.g_off + i, g0);
  stg1(r.g_len + i, (int32_t)gbytes);
  return OURO_PACK_OK;
}

// the rows of a block nothing is emitted for (not sliced, an EBB, or past a
// capacity): a zero Byron row, zero claims, and spans outside every buffer, for
// which launch_blake2b writes a zero digest.  msg_off[i], until here the scan's
// begin of block i, becomes 0: a begin past the message capacity must not reach
// the signature launch (launches.h ByronBlockDev says so for later readers)
constexpr uint64_t kNoSpan = ~0ull;
OURO_HD inline void byron_block_zero_row(const ByronOut& o, const BybRows& r, size_t i) {
  byron_zero_row(o, i);
  stg8(o.msg_off + i, 0);
  zero_bytes(r.claimed + 128 * i, 128);
  stg1(r.tx_num + i, 0);
  for (int q = 0; q < 2; q++) {
    stg8(r.seg_off + 2 * i + q, kNoSpan);
    stg1(r.seg_len + 2 * i + q, 0);
  }
  stg8(r.g_off + i, kNoSpan);
  stg1(r.g_len + i, 0);
}

// Blake2b-256 of the 65 bytes 0x01 || l || r, two digests of eight
// little-endian words each: one final compression with the prefix folded in
OURO_FI void byron_merkle_node(uint32_t out[8], const uint32_t l[8], const uint32_t r[8]) {
  uint64_t h[8], m[16];
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = kB2bIV[k];
  h[0] ^= 0x01010000ULL ^ 32;
  uint32_t w[17];
  w[0] = 0x01u | (l[0] << 8);
#pragma unroll
  for (int k = 1; k < 8; k++) w[k] = (l[k - 1] >> 24) | (l[k] << 8);
  w[8] = (l[7] >> 24) | (r[0] << 8);
#pragma unroll
  for (int k = 1; k < 8; k++) w[8 + k] = (r[k - 1] >> 24) | (r[k] << 8);
  w[16] = r[7] >> 24;
#pragma unroll
  for (int k = 0; k < 8; k++) m[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
  m[8] = w[16];
#pragma unroll
  for (int k = 9; k < 16; k++) m[k] = 0;
  b2b_compress(h, m, 65, true);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    out[2 * k] = (uint32_t)h[k];
    out[2 * k + 1] = (uint32_t)(h[k] >> 32);
  }
}

// eight words at a 16-byte aligned row of digests, and back
OURO_FI void byb_load8(uint32_t w[8], const uint8_t* p) {
  const int4 a = ldg4(p), b = ldg4(p + 16);
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
  w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
OURO_FI void byb_store8(uint8_t* p, const uint32_t w[8]) {
  stg4(p, make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]));
  stg4(p + 16, make_int4((int)w[4], (int)w[5], (int)w[6], (int)w[7]));
}

// The OURO_BYB_* bits of one block: the five comparisons of blockMatchesHeader
// (claimed: txpRoot | txpWitnessesHash | dlgHash | updHash against the four
// recomputed digests; txpNumber against the transactions counted) and
// verifyHeaderIntegrity (hdr_ok: the signature verifies and the magic
// matches).  An EBB passes everything; any other status but OK gives 0.
OURO_HD inline uint8_t byron_block_verdict(uint8_t st, uint32_t ntx, uint32_t tx_num, bool hdr_ok,
                                           const uint8_t* claimed, const uint8_t* root,
                                           const uint8_t* wit, const uint8_t* dlg,
                                           const uint8_t* upd) {
  if (st == OURO_PACK_EBB) return (uint8_t)OURO_BYB_ALL_OK;
  if (st != OURO_PACK_OK) return 0;
  const uint8_t* got[4] = {root, wit, dlg, upd};
  const uint32_t bit[4] = {OURO_BYB_TXROOT_OK, OURO_BYB_TXWIT_OK, OURO_BYB_DLG_OK, OURO_BYB_UPD_OK};
  uint32_t v = tx_num == ntx ? OURO_BYB_TXNUM_OK : 0u;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint32_t c[8], x[8], diff = 0;
    byb_load8(c, claimed + 32 * q);
    byb_load8(x, got[q]);
#pragma unroll
    for (int k = 0; k < 8; k++) diff |= c[k] ^ x[k];
    if (diff == 0) v |= bit[q];
  }
  const uint32_t five = OURO_BYB_TXNUM_OK | OURO_BYB_TXROOT_OK | OURO_BYB_TXWIT_OK |
                        OURO_BYB_DLG_OK | OURO_BYB_UPD_OK;
  if ((v & five) == five) v |= OURO_BYB_BODY_OK;
  if (hdr_ok) v |= OURO_BYB_HDR_OK;
  return (uint8_t)v;
}

// d = the Merkle root of the m leaf digests at `row` (m x 32 bytes, 16-byte
// aligned), reduced IN PLACE: pair neighbours level by level and carry an odd
// last node up unchanged.  That is the recursive definition's tree: its left
// subtree is always a full tree of the largest power of two below the count,
// which level-by-level pairing builds from the left, and the carried node is
// the right spine (tests/test_byron_block_rule.py checks the two against each
// other for every count up to 300).  Pair p of a level is written to slot p
// after slots 2p and 2p + 1 were read.  H("") for m = 0.
OURO_HD inline void byron_merkle_root(uint32_t d[8], uint8_t* row, uint32_t m) {
  if (m == 0) {
    blake2b256_stream(d, row, 0);  // (the empty message: nothing is read)
    return;
  }
  while (m > 1) {
    for (uint32_t p = 0; p < m / 2; p++) {
      uint32_t l[8], r[8];
      byb_load8(l, row + 64 * (size_t)p);
      byb_load8(r, row + 64 * (size_t)p + 32);
      byron_merkle_node(d, l, r);
      byb_store8(row + 32 * (size_t)p, d);
    }
    if (m & 1) {
      byb_load8(d, row + 32 * (size_t)(m - 1));
      byb_store8(row + 32 * (size_t)(m / 2), d);
    }
    m = (m + 1) / 2;
  }
  byb_load8(d, row);
}

}  // namespace cbor
}  // namespace ouro
