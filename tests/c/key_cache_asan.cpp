// TEST-ONLY: the key directory (csrc/key_cache.h) on the host, in a program of
// its own: the text the kernels compile, driven pass by pass the way
// kernels.hip launch_hdr drives it (begin, lookup + stamp, the grouping of the
// misses, decide, reset, insert), over a directory of 16 cells and 12 slots so
// that probes collide.  tests/test_key_cache_host.py builds it plainly and
// with -fsanitize=address,undefined and runs it as a child process; every
// check prints "ok <name>", a failed one "FAIL <name>: ..." and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "key_cache.h"

using namespace ouro;

namespace {

constexpr int KW = 8;
struct Key {
  uint32_t w[KW];
  bool operator<(const Key& o) const { return memcmp(w, o.w, sizeof w) < 0; }
};
// the hash keeps two bits of word 0: keys that differ elsewhere collide
uint64_t hash_of(const Key& k) { return k.w[0] & 3u; }
Key key_of(uint32_t id, uint32_t h) {
  Key k;
  for (int i = 0; i < KW; i++) k.w[i] = 0x9e3779b9u * (id + 1) + (uint32_t)i;
  k.w[0] = (k.w[0] & ~3u) | (h & 3u);
  return k;
}

int g_failed = 0;
void check(bool ok, const char* name, const char* what = "") {
  if (ok) {
    printf("ok %s\n", name);
  } else {
    printf("FAIL %s: %s\n", name, what);
    g_failed = 1;
  }
}

struct Dir {
  std::vector<uint8_t> mem;
  KcDir d;
  Dir(size_t cells, size_t slots) {
    // (kc_layout sizes the cells from the slots; here they are set by hand so
    // that 12 keys share 16 cells)
    KcLayout L = kc_layout(slots, KW);
    mem.assign(L.bytes, 0);
    d = kc_dir(mem.data(), L, slots);
    d.mask = (uint32_t)(cells - 1);
  }
};

struct Result {
  uint32_t total = 0, built = 0, work = 0;
  bool reset = false;
  std::vector<int32_t> slot;  // per batch key; -1: not in the directory after the call
};

// one call over `batch`, as launch_hdr runs it.  readd: the VRF instance.
Result call(Dir& D, const std::vector<Key>& batch, uint32_t share_max, bool readd) {
  KcDir& d = D.d;
  uint32_t* hdr = d.hdr;
  Result r;
  r.slot.assign(batch.size(), -1);
  kc_begin(hdr, false);
  const uint32_t gen = hdr[kKcGen];
  std::vector<size_t> uniq;
  auto find = [&](bool retry) {
    std::map<Key, size_t> seen;  // the per-call grouping: first index with the key
    uniq.clear();
    for (size_t i = 0; i < batch.size(); i++) {
      const int32_t s = retry ? -1 : kc_lookup<KW>(d, batch[i].w, hash_of(batch[i]), ~0u);
      if (s >= 0) {
        r.slot[i] = s;
        if (kc_stamp(d, (uint32_t)s, gen)) hdr[kKcHit]++;
      } else if (seen.emplace(batch[i], i).second) {
        uniq.push_back(i);
        hdr[kKcFresh]++;
      }
    }
  };
  find(false);
  kc_decide(hdr, share_max, d.slots, readd, false);
  r.reset = hdr[kKcReset] != 0;
  if (hdr[kKcReset]) {
    for (uint32_t c = 0; c <= d.mask; c++) d.cells[c] = 0;
    kc_reset_counts(hdr, readd);
    if (readd) {
      std::fill(r.slot.begin(), r.slot.end(), -1);
      find(true);
    }
  }
  if (readd) kc_decide(hdr, share_max, d.slots, readd, true);
  if (hdr[kKcInsert])
    for (uint32_t k = 0; k < hdr[kKcWork]; k++) {
      const Key& key = batch[uniq[k]];
      const int32_t s = kc_insert<KW>(d, key.w, hash_of(key), ~0u, gen);
      for (size_t i = 0; i < batch.size(); i++)
        if (!memcmp(batch[i].w, key.w, sizeof key.w) && r.slot[i] < 0) r.slot[i] = s;
    }
  r.total = hdr[kKcTotal];
  r.built = hdr[kKcBuilt];
  r.work = hdr[kKcWork];
  return r;
}

}  // namespace

int main() {
  // --- the layout ---
  {
    const KcLayout L = kc_layout(12, KW, true);
    check(L.cap == 32 && L.off_cells == 64 && L.off_stamp == 64 + 4 * 32 &&
              L.off_keys == L.off_stamp + 48 && L.off_extra == L.off_keys + 4 * KW * 12 &&
              L.off_val == L.off_extra + 48 && L.bytes >= L.off_val + 12 && L.bytes % 16 == 0 &&
              L.clear_bytes == L.off_stamp,
          "layout");
    check(kc_layout(0, KW).bytes == 0 && kc_layout(((size_t)1 << 30) + 1, KW).bytes == 0,
          "layout_rejects");
  }
  // --- 12 keys into 16 cells, four start cells: every probe chain collides ---
  std::vector<Key> twelve;
  for (uint32_t id = 0; id < 12; id++) twelve.push_back(key_of(id, id));
  {
    Dir D(16, 12);
    // each key three times, interleaved
    std::vector<Key> batch;
    for (int rep = 0; rep < 3; rep++) batch.insert(batch.end(), twelve.begin(), twelve.end());
    Result a = call(D, batch, 12, true);
    bool ok = a.total == 12 && a.built == 12 && !a.reset && D.d.hdr[kKcResident] == 12;
    std::map<int32_t, int> used;
    for (size_t i = 0; i < batch.size(); i++) {
      ok = ok && a.slot[i] >= 0 && a.slot[i] < 12 && a.slot[i] == a.slot[i % 12];
      used[a.slot[i]]++;
    }
    check(ok && used.size() == 12, "insert_12");
    for (size_t i = 0; i < 12; i++)
      ok = ok && kc_lookup<KW>(D.d, twelve[i].w, hash_of(twelve[i]), ~0u) == a.slot[i];
    check(ok, "lookup_12");
    // the same batch again: all found, nothing built, 12 distinct by the stamps
    Result b = call(D, batch, 12, true);
    check(b.total == 12 && b.built == 0 && b.work == 0 && !b.reset && b.slot == a.slot &&
              D.d.hdr[kKcHit] == 12 && D.d.hdr[kKcFresh] == 0 && D.d.hdr[kKcGen] == 2,
          "generation_distinct_count");
    // a sub-batch: its own distinct count, not the directory's
    std::vector<Key> five(twelve.begin() + 3, twelve.begin() + 8);
    five.push_back(twelve[3]);
    Result c = call(D, five, 12, true);
    check(c.total == 5 && c.built == 0, "distinct_of_this_batch");
    // an absent key with a resident key's hash and all but one word
    Key near = twelve[5];
    near.w[7] ^= 1u;
    check(kc_lookup<KW>(D.d, near.w, hash_of(near), ~0u) == -1, "equal_hash_other_bytes_absent");
    // the full directory: a 13th key does not fit; the VRF instance empties
    // the directory and inserts the batch's keys again
    std::vector<Key> mix = {twelve[0], key_of(100, 0), twelve[1], key_of(100, 0)};
    Result e = call(D, mix, 12, true);
    bool ok2 = e.reset && e.total == 3 && e.built == 3 && D.d.hdr[kKcResident] == 3 &&
               D.d.hdr[kKcEmptied] == 1 && e.slot[1] == e.slot[3] && e.slot[0] != e.slot[1] &&
               e.slot[0] != e.slot[2] && e.slot[1] != e.slot[2];
    for (int32_t s : e.slot) ok2 = ok2 && s >= 0 && s < 3;
    check(ok2, "full_empties_and_reinserts");
    check(kc_lookup<KW>(D.d, twelve[7].w, hash_of(twelve[7]), ~0u) == -1 &&
              kc_lookup<KW>(D.d, twelve[1].w, hash_of(twelve[1]), ~0u) == e.slot[2],
          "emptied_forgets_the_rest");
  }
  // --- equal hash, different bytes: kept apart, each with its own byte ---
  {
    Dir D(16, 12);
    std::vector<Key> same;
    for (uint32_t id = 0; id < 6; id++) same.push_back(key_of(id, 2));
    Result a = call(D, same, 12, false);
    bool ok = a.total == 6 && a.built == 6;
    for (size_t i = 0; i < 6; i++) D.d.val[a.slot[i]] = (uint8_t)(i + 1);
    for (size_t i = 0; i < 6; i++) {
      const int32_t s = kc_lookup<KW>(D.d, same[i].w, hash_of(same[i]), ~0u);
      ok = ok && s == a.slot[i] && D.d.val[s] == i + 1;
      for (size_t j = 0; j < i; j++) ok = ok && a.slot[i] != a.slot[j];
    }
    check(ok, "equal_hash_kept_apart");
  }
  // --- the certificate instance: a full directory takes the new keys only;
  // more new keys than slots are not inserted; over the limit nothing is ---
  {
    Dir D(16, 12);
    call(D, twelve, 100, false);
    std::vector<Key> two = {twelve[4], key_of(200, 1), key_of(201, 1)};
    Result a = call(D, two, 100, false);
    check(a.reset && a.total == 3 && a.built == 2 && a.work == 2 && D.d.hdr[kKcResident] == 2 &&
              a.slot[0] == 4 && a.slot[1] >= 0 && a.slot[2] >= 0 &&
              kc_lookup<KW>(D.d, twelve[4].w, hash_of(twelve[4]), ~0u) == -1,
          "certificates_full_takes_new_only");
    std::vector<Key> many;
    for (uint32_t id = 300; id < 313; id++) many.push_back(key_of(id, id));
    Result b = call(D, many, 100, false);
    check(!b.reset && b.total == 13 && b.built == 0 && b.work == 13 && D.d.hdr[kKcResident] == 2,
          "more_new_than_slots_not_inserted");
    Result c = call(D, many, 12, false);
    check(c.total == 13 && c.work == kKcNoShare && c.built == 0 && D.d.hdr[kKcResident] == 2 &&
              D.d.hdr[kKcInsert] == 0,
          "over_the_limit_inserts_nothing");
  }
  // --- a chain longer than the probe cap: the key keeps its slot for the call
  // and is not found again; nothing loops ---
  {
    Dir D(128, 100);
    std::vector<Key> chain;
    for (uint32_t id = 0; id < 70; id++) chain.push_back(key_of(id, 0));
    Result a = call(D, chain, 100, true);
    bool ok = a.total == 70 && a.built == 70;
    int found = 0;
    for (size_t i = 0; i < 70; i++) {
      ok = ok && a.slot[i] >= 0 && a.slot[i] < 70;
      found += kc_lookup<KW>(D.d, chain[i].w, hash_of(chain[i]), ~0u) == a.slot[i];
    }
    check(ok && found == kKcProbeCap, "probe_cap");
  }
  return g_failed;
}
