// key_cache.h -- a key directory in device memory that outlives the launch
// (kernels.hip launch_hdr, OURO_KEY_CACHE).  Plain C++ with no HIP in it: the
// device kernels and a host program (tests/c/key_cache_asan.cpp) compile the
// same text; a unit that calls it from device code defines OURO_KC_FN as its
// function attributes before including it.
//
// A directory maps key bytes (KW 32-bit words) to a slot 0 .. slots - 1.  What
// a slot stands for is the caller's: a VRF key's table and flag, or an
// operational certificate's verdict byte (val[]).  It is open-addressed:
// cells[] holds slot + 1 (0 = empty), the hash only picks where the probe
// starts, and a lookup always compares the full key bytes kept per slot, so
// two keys with one hash never share a slot.
//
// Every access is ordered by the stream the directory belongs to, pass by
// pass:
//   lookup   reads cells and keys only; a hit stamps its slot with the call's
//            generation (an atomic exchange: the first stamp per call is the
//            one that counts the key);
//   insert   one caller per NEW distinct key (absent, and distinct among the
//            callers of the pass, so no key is compared): takes the next slot,
//            writes the key bytes, claims an empty cell by compare-and-swap;
//   decide / reset   the counters between the passes (one caller) and the
//            emptying of the cells.
// No caller ever waits for another's write: probe, compare-and-swap, store.
// A probe chain is followed for at most kKcProbeCap cells by lookup and insert
// alike, so what was inserted is found; a key that finds no cell in that many
// probes keeps its slot for the call and is simply not found again (the slot
// comes back when the directory is next emptied).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef OURO_KC_FN
#define OURO_KC_FN inline
#endif

namespace ouro {

constexpr int kKcProbeCap = 64;

// the counters of a directory, 16 words at its start
enum KcWord : int {
  kKcGen = 0,       // the generation: the calls so far
  kKcResident = 1,  // slots handed out since the directory was last emptied
  kKcEmptied = 2,   // times emptied by a launch whose new keys did not fit
  kKcBuilt = 3,     // keys the last launch inserted
  kKcFresh = 4,     // this call: distinct keys not found (the grouping's count)
  kKcHit = 5,       // this call: distinct keys found
  kKcTotal = 6,     // this call: distinct keys (the sharing decision's count)
  kKcWork = 7,      // this call: the build list's length, all ones = do not share
  kKcReset = 8,     // this call: empty the directory and insert again
  kKcInsert = 9,    // this call: the insert pass runs
  kKcDirty = 10,    // the per-call grouping table has entries
  kKcWords = 16,
};
constexpr uint32_t kKcNoShare = 0xffffffffu;

struct KcDir {
  uint32_t* hdr = nullptr;    // kKcWords counters
  uint32_t* cells = nullptr;  // mask + 1 cells: slot + 1, 0 = empty
  uint32_t* stamp = nullptr;  // per slot: the generation that last saw it
  uint32_t* keys = nullptr;   // per slot: the key's words
  uint8_t* val = nullptr;     // per slot: a byte of the caller's
  uint32_t mask = 0;
  uint32_t slots = 0;
};

// hdr | cells[cap] | stamp[slots] | keys[slots][kw] | extra[slots] words of
// the caller's | val[slots]; cap the power of two >= 2 slots (at least 16)
struct KcLayout {
  size_t cap = 0, off_cells = 0, off_stamp = 0, off_keys = 0, off_extra = 0, off_val = 0;
  size_t clear_bytes = 0;  // counters and cells: zeroing them empties the directory
  size_t bytes = 0;
};
inline KcLayout kc_layout(size_t slots, size_t kw, bool extra = false) {
  KcLayout L;
  if (slots == 0 || slots > ((size_t)1 << 30)) return L;
  L.cap = 16;
  while (L.cap < 2 * slots) L.cap <<= 1;
  L.off_cells = 4 * (size_t)kKcWords;
  L.off_stamp = L.off_cells + 4 * L.cap;
  L.off_keys = L.off_stamp + 4 * slots;
  L.off_extra = L.off_keys + 4 * kw * slots;
  L.off_val = L.off_extra + (extra ? 4 * slots : 0);
  L.clear_bytes = L.off_stamp;
  L.bytes = (L.off_val + slots + 15) & ~(size_t)15;
  return L;
}
inline KcDir kc_dir(void* base, const KcLayout& L, size_t slots) {
  uint8_t* p = static_cast<uint8_t*>(base);
  KcDir d;
  d.hdr = reinterpret_cast<uint32_t*>(p);
  d.cells = reinterpret_cast<uint32_t*>(p + L.off_cells);
  d.stamp = reinterpret_cast<uint32_t*>(p + L.off_stamp);
  d.keys = reinterpret_cast<uint32_t*>(p + L.off_keys);
  d.val = p + L.off_val;
  d.mask = (uint32_t)(L.cap - 1);
  d.slots = (uint32_t)slots;
  return d;
}

OURO_KC_FN uint32_t kc_start(uint64_t h, uint32_t hash_mask, uint32_t mask) {
  return (uint32_t)(h ^ (h >> 32)) & hash_mask & mask;
}

// the slot of `key`, -1 when it is not in the directory (read only)
template <int KW>
OURO_KC_FN int32_t kc_lookup(const KcDir& d, const uint32_t* key, uint64_t h, uint32_t hash_mask) {
  uint32_t pos = kc_start(h, hash_mask, d.mask);
  for (int probe = 0; probe < kKcProbeCap; probe++) {
    const uint32_t v = d.cells[pos];
    if (v == 0u) return -1;
    if (v <= d.slots) {
      const uint32_t* k = d.keys + (size_t)(v - 1u) * KW;
      uint32_t diff = 0;
      for (int w = 0; w < KW; w++) diff |= k[w] ^ key[w];
      if (diff == 0u) return (int32_t)(v - 1u);
    }
    pos = (pos + 1u) & d.mask;
  }
  return -1;
}

// stamp `slot` with the call's generation; true for the call's first stamp of
// it (the plain load only spares the exchange: a stale value costs one more)
OURO_KC_FN bool kc_stamp(const KcDir& d, uint32_t slot, uint32_t gen) {
  if (d.stamp[slot] == gen) return false;
  return __atomic_exchange_n(&d.stamp[slot], gen, __ATOMIC_RELAXED) != gen;
}

// a new distinct key: its slot, -1 when no slot is left (kc_decide rules that
// out for the callers of an insert pass)
template <int KW>
OURO_KC_FN int32_t kc_insert(const KcDir& d, const uint32_t* key, uint64_t h, uint32_t hash_mask,
                             uint32_t gen) {
  const uint32_t slot = __atomic_fetch_add(&d.hdr[kKcResident], 1u, __ATOMIC_RELAXED);
  if (slot >= d.slots) return -1;
  uint32_t* k = d.keys + (size_t)slot * KW;
  for (int w = 0; w < KW; w++) k[w] = key[w];
  d.stamp[slot] = gen;
  uint32_t pos = kc_start(h, hash_mask, d.mask);
  for (int probe = 0; probe < kKcProbeCap; probe++) {
    uint32_t expect = 0u;
    if (__atomic_compare_exchange_n(&d.cells[pos], &expect, slot + 1u, false, __ATOMIC_RELAXED,
                                    __ATOMIC_RELAXED))
      break;
    pos = (pos + 1u) & d.mask;
  }
  return (int32_t)slot;
}

// ---- the counters between the passes (one caller each) ----
// a call begins: the next generation, this call's counts cleared.  `empty`:
// the host has zeroed the cells (a re-sized workspace, OURO_KEY_CACHE=0).
OURO_KC_FN void kc_begin(uint32_t* hdr, bool empty) {
  hdr[kKcGen] += 1u;
  if (empty) hdr[kKcResident] = 0u;
  hdr[kKcBuilt] = 0u;
  hdr[kKcFresh] = 0u;
  hdr[kKcHit] = 0u;
  hdr[kKcTotal] = 0u;
  hdr[kKcWork] = kKcNoShare;
  hdr[kKcReset] = 0u;
  hdr[kKcInsert] = 0u;
}

// after the lookup and the grouping of its misses: the batch's distinct count
// and what follows from it.  share_max: the launch shares iff the batch's
// distinct keys number at most this.  readd: emptying the directory loses the
// keys found too, and the call inserts them again (the VRF tables, whose
// slots the emptying hands out anew); otherwise only the new ones go in.
// after_reset: the second decision of a call that emptied the directory (its
// grouping ran again over every key).
OURO_KC_FN void kc_decide(uint32_t* hdr, uint32_t share_max, uint32_t slots, bool readd,
                          bool after_reset) {
  if (after_reset && !hdr[kKcReset]) return;
  const uint32_t fresh = hdr[kKcFresh], total = fresh + hdr[kKcHit];
  const bool share = total <= share_max;
  hdr[kKcTotal] = total;
  hdr[kKcDirty] = fresh ? 1u : 0u;
  hdr[kKcWork] = share ? fresh : kKcNoShare;
  const uint32_t resident = hdr[kKcResident];
  const bool fits = resident <= slots && fresh <= slots - resident;
  const bool reset = !after_reset && share && fresh && !fits && (readd ? total : fresh) <= slots;
  hdr[kKcReset] = reset ? 1u : 0u;
  hdr[kKcInsert] = share && fresh && (fits || reset) ? 1u : 0u;
  hdr[kKcBuilt] = hdr[kKcInsert] ? (reset && readd ? total : fresh) : 0u;
}

// the reset pass's one caller (the cells are zeroed by all of its callers).
// regroup: the grouping runs again, so its count starts over.
OURO_KC_FN void kc_reset_counts(uint32_t* hdr, bool regroup) {
  hdr[kKcResident] = 0u;
  hdr[kKcEmptied] += 1u;
  if (regroup) {
    hdr[kKcFresh] = 0u;
    hdr[kKcHit] = 0u;
  }
}

}  // namespace ouro
