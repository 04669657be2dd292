// Stand-alone AddressSanitizer + UBSan run of the host witness walker
// (csrc/cbor_witness.h), in both passes, and the host streaming Blake2b
// (csrc/blake2b_stream.h): the routines ouro_block_witness_verify_cbor_host
// runs per block, compiled here with -fsanitize=address,undefined and called
// from this program's own main (tests/test_witness_asan.py builds and runs
// it; nothing is loaded into Python).
//
// Input: a file of cases, each a little-endian uint32 length followed by that
// many bytes of raw block CBOR.  Every case is copied into a heap buffer of
// exactly its length (so any read past the span is a heap-buffer-overflow),
// counted, and -- when it slices -- emitted into rows of exactly the counted
// sizes (so any row past the counts is one too) and its tx bodies hashed.
// Output: one line "cases N ok K digest <hex>" where digest folds every
// status, count, tx id and witness row (the test compares it with its own
// computation).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blake2b_stream.h"
#include "cbor_witness.h"

using namespace ouro;

static uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: witness_asan CASES\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  size_t cases = 0, ok = 0;
  uint32_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (;;) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const uint32_t len = le32(lb);
    uint8_t* raw = static_cast<uint8_t*>(malloc(len ? len : 1));
    if (!raw || (len && fread(raw, 1, len, f) != len)) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    uint32_t ntx, nwit, x[8] = {0, 0, 0, 0, 0, 0, 0, 0}, extra = 0;
    const uint8_t st = cbor::witness_count_one(raw, 0, len, &ntx, &nwit);
    if (st == OURO_PACK_OK) {
      // rows of exactly the counted sizes, each its own allocation
      uint64_t* tx_off = static_cast<uint64_t*>(malloc(ntx ? 8 * ntx : 1));
      uint32_t* tx_len = static_cast<uint32_t*>(malloc(ntx ? 4 * ntx : 1));
      uint8_t* vk = static_cast<uint8_t*>(malloc(nwit ? 32 * nwit : 1));
      uint8_t* sig = static_cast<uint8_t*>(malloc(nwit ? 64 * nwit : 1));
      uint32_t* wit_tx = static_cast<uint32_t*>(malloc(nwit ? 4 * nwit : 1));
      uint8_t* kind = static_cast<uint8_t*>(malloc(nwit ? nwit : 1));
      const cbor::WitRows rows{tx_off, tx_len, vk, sig, wit_tx, kind, 0};
      if (cbor::witness_emit_one(raw, 0, len, rows, 0, 0, ntx, nwit) != OURO_PACK_OK) {
        fprintf(stderr, "the emit pass rejects what the count pass accepted\n");
        return 3;
      }
      for (uint32_t t = 0; t < ntx; t++) {
        uint32_t d[8];
        blake2b256_stream(d, raw + tx_off[t], tx_len[t]);
        for (int k = 0; k < 8; k++) x[k] ^= d[k];
      }
      for (uint32_t w = 0; w < nwit; w++) {
        for (int k = 0; k < 8; k++)
          x[k] ^= le32(vk + 32 * w + 4 * k) ^ le32(sig + 64 * w + 4 * k) ^
                  le32(sig + 64 * w + 32 + 4 * k);
        extra += 3 * wit_tx[w] + kind[w];
      }
      free(tx_off);
      free(tx_len);
      free(vk);
      free(sig);
      free(wit_tx);
      free(kind);
      ok++;
    }
    for (int k = 0; k < 8; k++)
      fold[k] = fold[k] * 1000003u + x[k] + st + 7 * ntx + 11 * nwit + extra;
    free(raw);
    cases++;
  }
  fclose(f);
  printf("cases %zu ok %zu digest", cases, ok);
  for (int k = 0; k < 8; k++) printf(" %08x", fold[k]);
  printf("\n");
  return 0;
}
