// vrfkey_ws.h -- sizes of the per-key VRF table workspace (kernels.hip
// launch_hdr, OURO_VRFKEY_SHARE).  Plain C++ with no HIP in it, so the
// arithmetic can be tested on its own (tests/c/vrfkey_ws_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ouro {

// Headers per distinct key below which the tables are not built.  In
// instructions a key's table (one decode, ~126 doublings, ~680 additions with
// their conversions: ~1.1 M VALU at width 6) pays for itself after four
// headers at ~310 k VALU saved each; 16 leaves a fourfold margin for the
// build kernels, which run one lane per key or per window and so well below
// the header kernel's issue rate.  Measured (tools/vrfkey_ratio.py,
// profiles/vrfkey_share): at 1,048,576 headers over 65,536 keys, 16 per key,
// the tables still save 8 % (50.7 against 55.2 ms), so the crossover lies
// below 16; it was not looked for, and the derived value stands.
#ifndef OURO_VRFKEY_MIN_PER_KEY
#define OURO_VRFKEY_MIN_PER_KEY 16
#endif
constexpr size_t kVrfKeyMinPerKey = OURO_VRFKEY_MIN_PER_KEY;

// The grouping buffer of a batch of n headers:
//   counter (one 16-B row) | the header kernel's record (64 B) | table[cap] |
//   rep[n] | uniq[n] | kidx[n] | flag[kmax]
// table entries are header index + 1 in 32 bits, cap the power of two >= 2n.
// (The counts and the keys' flags now live in the stream's key directory,
// key_cache.h, which outlives the call; their places here stay, unused, so
// that the offsets are the ones the layout check pins.)
struct VrfKeyLayout {
  size_t kmax = 0;       // distinct keys the tables are sized for (0: do not share)
  size_t cap = 0;        // entries of the open-addressing table
  size_t off_desc = 16, off_table = 0, off_rep = 0, off_uniq = 0, off_kidx = 0, off_flag = 0;
  size_t group_bytes = 0;
  size_t table_bytes = 0;  // kmax keys' tables and window base points
};
// key_bytes: a key's table and base points (verify.h kYKeyBytes); budget: the
// bytes the tables may take (OURO_VRFKEY_TAB_MB)
inline VrfKeyLayout vrfkey_layout(size_t n, size_t key_bytes, size_t budget,
                                  size_t min_per_key = kVrfKeyMinPerKey) {
  VrfKeyLayout L;
  if (n == 0 || n > ((size_t)1 << 30) || key_bytes == 0 || min_per_key == 0) return L;
  const size_t by_ratio = n / min_per_key, by_budget = budget / key_bytes;
  L.kmax = by_ratio < by_budget ? by_ratio : by_budget;
  if (L.kmax == 0) return L;
  L.cap = 64;
  while (L.cap < 2 * n) L.cap <<= 1;
  L.off_table = L.off_desc + 64;
  L.off_rep = L.off_table + 4 * L.cap;
  L.off_uniq = L.off_rep + 4 * n;
  L.off_kidx = L.off_uniq + 4 * n;
  L.off_flag = L.off_kidx + 4 * n;
  L.group_bytes = (L.off_flag + L.kmax + 15) & ~(size_t)15;
  L.table_bytes = L.kmax * key_bytes;
  return L;
}

}  // namespace ouro
