// Stand-alone AddressSanitizer + UBSan run of the Byron ledger-view checks'
// host side: the lane routines (csrc/sha3.h, csrc/pbft_view.h), the window
// fold and the host check entry (csrc/pbft_api.cpp, compiled into this program
// as it stands), built here with -fsanitize=address,undefined and called from
// this program's own main (tests/test_pbft_asan.py builds and runs it; nothing
// is loaded into Python).  This program has no device: the few runtime
// functions the unit's device path calls are defined below and report
// OURO_EDEVICE, so ouro_pbft_ledger_checks recomputes on the host path -- the
// route a device error takes in the product.
//
// Input: one case file, little-endian.
//   k:u32 window:u64 threshold:u64 first_slot[k]:u64 dlg_begin[k + 1]:u32
//   then per schedule row delegate_id[28] genesis_id[28];
//   m:u32, then per incoming signer slot:u64 id[28];
//   n:u32, then per row delegate_vk[64] slot:u64 status:u8.
// Every array is copied into a heap buffer of exactly its size, so a read or
// write past it is a heap-buffer-overflow; the state's out-buffers hold exactly
// `window` rows.
// Output: "sha3 <hex>" folding SHA3-256 of the messages 0^len for every length
// 0 .. 135, and "rows N fold <hex>" folding every row's bits, schedule row,
// count and key hash and the window afterwards (the test folds the same from
// hashlib and pbft.pbft_rule).  The aliased fold and the recompute route must
// reproduce the host entry's outputs byte for byte (exit status 3 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pbft_api.cpp"
#include "task_pool.cpp"

namespace ouro_rt {
thread_local std::string t_last_error;
std::atomic<unsigned long long> g_host_single{0}, g_host_recompute{0};
int fail(int code, const std::string& what) {
  t_last_error = what;
  return code;
}
static int no_device() { return fail(OURO_EDEVICE, "no device in this program"); }
bool recompute_on_error() { return true; }
int current_device(int*) { return no_device(); }
int device_state(DeviceState**) { return no_device(); }
int thread_stream(hipStream_t*) { return no_device(); }
int ensure(Buf&, size_t) { return no_device(); }
int finish(hipStream_t) { return no_device(); }
int download(hipStream_t, void*, const void*, size_t) { return no_device(); }
ThreadCtx& ctx() {
  static ThreadCtx c;
  return c;
}
int launch_pbft(hipStream_t, size_t, const uint8_t*, const uint64_t*, const uint8_t*,
                const ouro_pbft_views&, uint8_t*, uint32_t*) {
  return no_device();
}
int launch_byron_key_hash(hipStream_t, size_t, const uint8_t*, uint8_t*) { return no_device(); }
}  // namespace ouro_rt
namespace ouro_host {
int threads_for(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(4, n / 16)); }
}  // namespace ouro_host

static uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

template <class T>
static T* heap(size_t count) {
  T* p = static_cast<T*>(malloc(count ? count * sizeof(T) : 1));
  if (!p) exit(2);
  return p;
}
static FILE* g_f;
static void rd(void* p, size_t n) {
  if (n && fread(p, 1, n, g_f) != n) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
}
static uint32_t rd32() {
  uint8_t b[4];
  rd(b, 4);
  return le32(b);
}
static uint64_t rd64() {
  uint8_t b[8];
  rd(b, 8);
  return le64(b);
}

static uint32_t g_fold;
static void fold(uint32_t v) { g_fold = g_fold * 1000003u + v; }
static void fold_bytes28(const uint8_t* p) {
  for (int w = 0; w < 7; w++) fold(le32(p + 4 * w));
}

int main(int argc, char** argv) {
  if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: pbft_asan CASES\n");
    return 2;
  }
  // ---- sha3_256_short at every length it takes ----
  g_fold = 0;
  for (uint32_t len = 0; len <= 135; len++) {
    uint32_t in[34], out[8];
    for (int w = 0; w < 34; w++) in[w] = 0;
    ouro::sha3_256_short(out, in, len);
    for (int w = 0; w < 8; w++) fold(out[w]);
  }
  printf("sha3 %08x\n", g_fold);

  // ---- the schedule, the state and the rows, each in its own allocation ----
  const uint32_t k = rd32();
  ouro_pbft_views v;
  v.k = k;
  v.window = rd64();
  v.threshold = rd64();
  uint64_t* first_slot = heap<uint64_t>(k);
  uint32_t* dlg_begin = heap<uint32_t>(k + 1);
  for (uint32_t j = 0; j < k; j++) first_slot[j] = rd64();
  for (uint32_t j = 0; j <= k; j++) dlg_begin[j] = rd32();
  const size_t rows = dlg_begin[k];
  uint8_t* delegate_id = heap<uint8_t>(28 * rows);
  uint8_t* genesis_id = heap<uint8_t>(28 * rows);
  for (size_t r = 0; r < rows; r++) {
    rd(delegate_id + 28 * r, 28);
    rd(genesis_id + 28 * r, 28);
  }
  v.first_slot = first_slot;
  v.dlg_begin = dlg_begin;
  v.delegate_id = delegate_id;
  v.genesis_id = genesis_id;
  const size_t W = (size_t)v.window;
  const uint32_t m = rd32();
  // the incoming state in buffers of the window's capacity: the aliased run
  // below writes the outgoing state over it
  uint8_t* st_id = heap<uint8_t>(28 * W);
  uint64_t* st_slot = heap<uint64_t>(W);
  if (m > W) return 2;
  for (uint32_t i = 0; i < m; i++) {
    st_slot[i] = rd64();
    rd(st_id + 28 * i, 28);
  }
  const ouro_pbft_state st{m, st_id, st_slot};
  const uint32_t n = rd32();
  uint8_t* vk = heap<uint8_t>(64 * (size_t)n);
  uint64_t* slot = heap<uint64_t>(n);
  uint8_t* status = heap<uint8_t>(n);
  for (uint32_t i = 0; i < n; i++) {
    rd(vk + 64 * (size_t)i, 64);
    slot[i] = rd64();
    rd(status + i, 1);
  }

  // ---- the host entry ----
  uint8_t* bits = heap<uint8_t>(n);
  uint32_t* grow = heap<uint32_t>(n);
  uint64_t* cnt = heap<uint64_t>(n);
  uint8_t* out_id = heap<uint8_t>(28 * W);
  uint64_t* out_slot = heap<uint64_t>(W);
  size_t n_out = 0;
  if (ouro_pbft_ledger_checks_host(n, vk, slot, status, &v, &st, out_id, out_slot, &n_out, bits,
                                   grow, cnt) != OURO_OK) {
    fprintf(stderr, "host entry: %s\n", ouro_rt::t_last_error.c_str());
    return 2;
  }
  uint8_t* kh = heap<uint8_t>(28 * (size_t)n);
  if (ouro_byron_key_hash_batch_host(n, vk, kh) != OURO_OK) return 2;
  g_fold = 0;
  for (uint32_t i = 0; i < n; i++) {
    fold(bits[i]);
    fold(grow[i]);
    fold((uint32_t)cnt[i]);
    fold((uint32_t)(cnt[i] >> 32));
    fold_bytes28(kh + 28 * (size_t)i);
  }
  fold((uint32_t)n_out);
  for (size_t i = 0; i < n_out; i++) {
    fold((uint32_t)out_slot[i]);
    fold((uint32_t)(out_slot[i] >> 32));
    fold_bytes28(out_id + 28 * i);
  }
  printf("rows %u fold %08x\n", n, g_fold);

  // ---- the recompute route: the entry whose device run fails ----
  {
    uint8_t* b2 = heap<uint8_t>(n);
    uint32_t* r2 = heap<uint32_t>(n);
    uint64_t* c2 = heap<uint64_t>(n);
    uint8_t* id2 = heap<uint8_t>(28 * W);
    uint64_t* sl2 = heap<uint64_t>(W);
    uint8_t* kh2 = heap<uint8_t>(28 * (size_t)n);
    size_t n2 = 0;
    if (ouro_pbft_ledger_checks(n, vk, slot, status, &v, &st, id2, sl2, &n2, b2, r2, c2) != OURO_OK ||
        (n && ouro_byron_key_hash_batch(n, vk, kh2) != OURO_OK))
      return 2;
    if (n2 != n_out || memcmp(b2, bits, n) || memcmp(r2, grow, 4 * (size_t)n) ||
        memcmp(c2, cnt, 8 * (size_t)n) || memcmp(id2, out_id, 28 * n_out) ||
        memcmp(sl2, out_slot, 8 * n_out) || memcmp(kh2, kh, 28 * (size_t)n))
      return 3;
    free(b2), free(r2), free(c2), free(id2), free(sl2), free(kh2);
  }
  // ---- the fold entry from the lookup's bits, its outputs over its inputs ----
  {
    uint8_t* b3 = heap<uint8_t>(n);
    uint64_t* c3 = heap<uint64_t>(n);
    for (uint32_t i = 0; i < n; i++) b3[i] = bits[i] & ~(OURO_PBFT_SLOT_OK | OURO_PBFT_WINDOW_OK);
    // (a boundary row keeps BOUNDARY | ALL_OK: the fold leaves it as it is)
    for (uint32_t i = 0; i < n; i++)
      if (bits[i] & OURO_PBFT_BOUNDARY) b3[i] = bits[i];
    size_t n3 = 0;
    if (ouro_pbft_window_fold(n, grow, slot, &v, &st, st_id, st_slot, &n3, b3, c3) != OURO_OK)
      return 2;
    if (n3 != n_out || memcmp(b3, bits, n) || memcmp(c3, cnt, 8 * (size_t)n) ||
        memcmp(st_id, out_id, 28 * n_out) || memcmp(st_slot, out_slot, 8 * n_out))
      return 3;
    free(b3), free(c3);
  }
  free(first_slot), free(dlg_begin), free(delegate_id), free(genesis_id), free(st_id), free(st_slot);
  free(vk), free(slot), free(status), free(bits), free(grow), free(cnt), free(out_id), free(out_slot);
  free(kh);
  fclose(g_f);
  return 0;
}
