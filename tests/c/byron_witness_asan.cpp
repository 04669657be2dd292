// Stand-alone AddressSanitizer + UBSan run of the host Byron witness walker
// (csrc/cbor_byron_witness.h), in both passes, the host tx-id hash
// (csrc/blake2b_stream.h) and the message builder: the routines
// ouro_byron_block_witness_verify_cbor_host runs per block, compiled here with
// -fsanitize=address,undefined and called from this program's own main
// (tests/test_byron_witness_asan.py builds and runs it; nothing is loaded into
// Python).
//
// Input: a file of cases, each a little-endian uint32 length followed by that
// many bytes of raw block CBOR.  Every case is copied into a heap buffer of
// exactly its length (so any read past the span is a heap-buffer-overflow),
// counted, and -- when it is a regular block that slices -- emitted into rows
// of exactly the counted sizes (so any row past the counts is one too), its tx
// ids hashed and its rows' messages built under MAGIC (-1: the header's own).
// Output: one line "cases N ok K digest <hex>" where digest folds every status,
// count, kind, key, signature, tx row and message (the test compares it with
// its own computation).  No signature is verified here.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cbor_byron_witness.h"

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
    fprintf(stderr, "usage: byron_witness_asan CASES MAGIC\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const int64_t magic_cfg = strtoll(argv[2], nullptr, 10);
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
    uint32_t ntx, nwit, x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint8_t st = cbor::byron_witness_count_one(raw, 0, len, &ntx, &nwit);
    if (st == OURO_PACK_OK) {
      // rows of exactly the counted sizes, each its own allocation
      uint64_t* tx_off = rows<uint64_t>(ntx);
      uint32_t *tx_len = rows<uint32_t>(ntx), *wit_tx = rows<uint32_t>(nwit);
      uint8_t *vk = rows<uint8_t>(64 * (size_t)nwit), *sig = rows<uint8_t>(64 * (size_t)nwit),
              *kind = rows<uint8_t>(nwit), *id = rows<uint8_t>(32 * (size_t)ntx);
      const cbor::BywRows r{tx_off, tx_len, vk, sig, wit_tx, kind, 0};
      uint64_t magic = ~0ull;
      if (cbor::byron_witness_emit_one(raw, 0, len, r, 0, 0, ntx, nwit, &magic) != OURO_PACK_OK) {
        fprintf(stderr, "the emit pass differs from what the count pass found\n");
        return 3;
      }
      if (magic_cfg >= 0) magic = (uint64_t)magic_cfg;
      for (uint32_t t = 0; t < ntx; t++) {
        uint32_t d[8];
        blake2b256_stream(d, raw + tx_off[t], tx_len[t]);
        cbor::byb_store8(id + 32 * (size_t)t, d);
      }
      for (uint32_t w = 0; w < nwit; w++) {
        uint8_t* msg = rows<uint8_t>(40);
        const uint32_t ml = cbor::byron_witness_message(msg, kind[w], magic, id + 32 * (size_t)wit_tx[w]);
        uint32_t d[8];
        blake2b256_stream(d, msg, ml);
        for (int k = 0; k < 8; k++)
          x[k] = x[k] * 31u + (d[k] ^ le32(vk + 64 * (size_t)w + 4 * k) ^
                               le32(vk + 64 * (size_t)w + 32 + 4 * k) ^ le32(sig + 64 * (size_t)w + 4 * k) ^
                               le32(sig + 64 * (size_t)w + 32 + 4 * k)) + kind[w] + 3 * wit_tx[w];
        free(msg);
      }
      free(tx_off), free(tx_len), free(wit_tx), free(vk), free(sig), free(kind), free(id);
      ok++;
    }
    for (int k = 0; k < 8; k++) fold[k] = fold[k] * 1000003u + x[k] + st + 7 * ntx + 11 * nwit;
    free(raw);
    cases++;
  }
  fclose(f);
  printf("cases %zu ok %zu digest", cases, ok);
  for (int k = 0; k < 8; k++) printf(" %08x", fold[k]);
  printf("\n");
  return 0;
}
