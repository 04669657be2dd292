// Stand-alone AddressSanitizer + UBSan run of the host block slicer
// (csrc/cbor_block.h) and the host streaming Blake2b (csrc/blake2b_stream.h):
// the routines ouro_block_integrity_verify_cbor_host runs per block, compiled
// here with -fsanitize=address,undefined and called from this program's own
// main (tests/test_block_asan.py builds and runs it; nothing is loaded into
// Python).
//
// Input: a file of cases, each a little-endian uint32 length followed by that
// many bytes of raw block CBOR.  Every case is copied into a heap buffer of
// exactly its length (so any read past the span is a heap-buffer-overflow),
// sliced, and -- when it slices -- its three segments and the body hash are
// hashed.  Output: one line "cases N ok K digest <hex>" where digest folds
// every status and body hash (the test compares it with its own computation).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blake2b_stream.h"
#include "cbor_block.h"

using namespace ouro;

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: block_asan CASES\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const cbor::BlockLayout L = cbor::block_layout(1);
  std::vector<uint8_t> mem(L.total + 64);
  uint8_t* a = cbor::arena_base(mem.data());
  const cbor::Out o = cbor::arena_out(a + L.hdr, 1, nullptr, nullptr);
  const cbor::BlockOut bo = cbor::block_arena_out(a, L);
  size_t cases = 0, ok = 0;
  uint32_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (;;) {
    uint8_t lb[4];
    if (fread(lb, 1, 4, f) != 4) break;
    const uint32_t len = (uint32_t)lb[0] | ((uint32_t)lb[1] << 8) | ((uint32_t)lb[2] << 16) |
                         ((uint32_t)lb[3] << 24);
    uint8_t* raw = static_cast<uint8_t*>(malloc(len ? len : 1));
    if (!raw || (len && fread(raw, 1, len, f) != len)) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    // (a zero-length case: a one-byte allocation of which nothing may be read)
    const uint8_t st = cbor::block_one(raw, 0, len, 129600, o, bo, 0);
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (st == OURO_PACK_OK) {
      uint32_t d[24];
      for (int s = 0; s < 3; s++) blake2b256_stream(d + 8 * s, raw + bo.seg_off[s], bo.seg_len[s]);
      blake2b256_96(h, d);
      ok++;
    } else {
      cbor::block_zero_row(o, bo, 0);
    }
    // the whole case as one message too: every length the file holds
    uint32_t w[8];
    blake2b256_stream(w, raw, len);
    for (int k = 0; k < 8; k++) fold[k] = fold[k] * 1000003u + (h[k] ^ w[k]) + st;
    free(raw);
    cases++;
  }
  fclose(f);
  printf("cases %zu ok %zu digest", cases, ok);
  for (int k = 0; k < 8; k++) printf(" %08x", fold[k]);
  printf("\n");
  return 0;
}
