// Stand-alone AddressSanitizer + UBSan run of the host Byron block walker
// (csrc/cbor_byron_block.h), in both passes, and the host hashes of the body
// proof (csrc/blake2b_stream.h, byron_merkle_root): the routines
// ouro_byron_block_integrity_verify_cbor_host runs per block, compiled here
// with -fsanitize=address,undefined and called from this program's own main
// (tests/test_byron_block_asan.py builds and runs it; nothing is loaded into
// Python).
//
// Input: a file of cases, each a little-endian uint32 length followed by that
// many bytes of raw block CBOR.  Every case is copied into a heap buffer of
// exactly its length (so any read past the span is a heap-buffer-overflow),
// counted, and -- when it is a regular block that slices -- emitted into rows
// of exactly the counted sizes (so any row past the counts is one too), its
// proof recomputed and compared.
// Output: one line "cases N ok K digest <hex>" where digest folds every
// status, count, verdict bit, root and message (the test compares it with its
// own computation).  The signature is not verified here: hdr_ok is 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cbor_byron_block.h"

using namespace ouro;

static uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
template <class T>
static T* rows(size_t count) {
  return static_cast<T*>(malloc(count ? count * sizeof(T) : 1));
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: byron_block_asan CASES MAGIC\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const int64_t magic = strtoll(argv[2], nullptr, 10);
  size_t cases = 0, ok = 0;
  uint32_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (;;) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const uint32_t len = le32(lb);
    uint8_t* raw = rows<uint8_t>(len);
    if (!raw || (len && fread(raw, 1, len, f) != len)) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    uint32_t ntx, gb, mb, x[8] = {0, 0, 0, 0, 0, 0, 0, 0}, verdict = 0;
    const uint8_t st = cbor::byron_block_count_one(raw, 0, len, magic, &ntx, &gb, &mb);
    if (st == OURO_PACK_OK) {
      // rows of exactly the counted sizes, each its own allocation
      uint64_t msg_off = 0, magic_row, seg_off[2], g_off;
      uint32_t msg_len, tx_num, seg_len[2], g_len;
      uint8_t *pk = rows<uint8_t>(32), *sig = rows<uint8_t>(64), *gvk = rows<uint8_t>(64),
              *dvk = rows<uint8_t>(64), *msg = rows<uint8_t>(mb), *claimed = rows<uint8_t>(128),
              *gather = rows<uint8_t>(gb), *leaf = rows<uint8_t>(32 * (size_t)ntx);
      uint64_t* tx_off = rows<uint64_t>(ntx);
      uint32_t* tx_len = rows<uint32_t>(ntx);
      const cbor::ByronOut o{pk, sig, gvk, dvk, msg, &msg_off, &magic_row, &msg_len};
      const cbor::BybRows r{claimed, &tx_num, seg_off, seg_len, &g_off, &g_len, tx_off, tx_len, gather};
      if (cbor::byron_block_emit_one(raw, 0, len, magic, o, r, 0, 0, 0, ntx, gb) != OURO_PACK_OK ||
          msg_len != mb || g_len != gb || gather[0] != 0x9f || gather[gb - 1] != 0xff) {
        fprintf(stderr, "the emit pass differs from what the count pass found\n");
        return 3;
      }
      uint32_t d[8], root[8], wit[8], seg[2][8];
      for (uint32_t t = 0; t < ntx; t++) {
        blake2b256_stream_prefixed(d, 0u, 1u, raw + tx_off[t], tx_len[t]);
        cbor::byb_store8(leaf + 32 * (size_t)t, d);
      }
      cbor::byron_merkle_root(root, leaf, ntx);
      blake2b256_stream(wit, gather, gb);
      for (int q = 0; q < 2; q++) blake2b256_stream(seg[q], raw + seg_off[q], seg_len[q]);
      uint8_t got[4][32];
      cbor::byb_store8(got[0], root);
      cbor::byb_store8(got[1], wit);
      cbor::byb_store8(got[2], seg[0]);
      cbor::byb_store8(got[3], seg[1]);
      verdict = cbor::byron_block_verdict(st, ntx, tx_num, true, claimed, got[0], got[1], got[2],
                                          got[3]);
      blake2b256_stream(d, msg, mb);
      for (int k = 0; k < 8; k++)
        x[k] = root[k] ^ d[k] ^ le32(pk + 4 * k) ^ le32(sig + 4 * k) ^ le32(sig + 32 + 4 * k);
      free(pk), free(sig), free(gvk), free(dvk), free(msg), free(claimed), free(gather), free(leaf);
      free(tx_off), free(tx_len);
      ok++;
    } else {
      verdict = cbor::byron_block_verdict(st, 0, 0, true, raw, raw, raw, raw, raw);
    }
    for (int k = 0; k < 8; k++)
      fold[k] = fold[k] * 1000003u + x[k] + st + 7 * ntx + 11 * gb + 13 * mb + 17 * verdict;
    free(raw);
    cases++;
  }
  fclose(f);
  printf("cases %zu ok %zu digest", cases, ok);
  for (int k = 0; k < 8; k++) printf(" %08x", fold[k]);
  printf("\n");
  return 0;
}
