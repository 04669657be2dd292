// host_util.h -- the steps every host unit over the C ABI takes, once: the
// span check of an (offset, length) batch, rows over the worker pool, digest
// words to bytes, the 16-byte round-up, and the prelude of a *_device entry.
// Host units only (no kernel unit includes it); internal to the library
// (hidden visibility), like runtime.h.
#pragma once
#include <algorithm>
#include <atomic>
#include <string>

#include "../../include/ouro_verify.h"
#include "host_path.h"
#include "runtime.h"
#include "task_pool.h"

#pragma GCC visibility push(hidden)
namespace ouro_rt {

constexpr size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- the span check ----
// [off, off + len) inside a buffer of `bytes` bytes, compared without wrapping
inline bool span_inside(size_t bytes, uint64_t off, uint32_t len) {
  return off <= bytes && bytes - off >= len;
}
// "<item> <i>: span outside <bound>" (OURO_EINVAL)
inline int span_fail(const char* item, const char* bound, size_t i) {
  return fail(OURO_EINVAL, std::string(item) + " " + std::to_string(i) + ": span outside " + bound);
}
// every span of a batch, before any work and any output; the first bad one's
// index in the text
inline int spans_check(const char* item, const char* bound, size_t bytes, const uint64_t* off,
                       const uint32_t* len, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!span_inside(bytes, off[i], len[i])) return span_fail(item, bound, i);
  return OURO_OK;
}

// [0, n) in tasks of `per` items over the library's worker pool
template <class F>
int host_rows(size_t n, size_t per, F work) {
  const size_t tasks = (n + per - 1) / per;
  if (tasks <= 1) {
    if (n) work(0, n);
    return OURO_OK;
  }
  const int width = std::max(1, ouro_host::threads_for(n));
  const int r = ouro_pool::parallel_for(tasks, width, [&](size_t t) {
    work(t * per, std::min(n, (t + 1) * per));
  });
  return r ? fail(OURO_EDEVICE, "host worker pool failed") : OURO_OK;
}

// the eight words of a Blake2b-256 digest as its 32 bytes
inline void digest_bytes(uint8_t* d, const uint32_t w[8]) {
  for (int k = 0; k < 32; k++) d[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

// ---- a *_device entry, after its argument checks ----
// the device ready (its tables built), then the caller's stream
// (NULL = HIP's default stream)
inline int device_entry(void* stream, hipStream_t* st) {
  DeviceState* ds;
  if (int rc = device_state(&ds)) return rc;
  *st = static_cast<hipStream_t>(stream);
  return OURO_OK;
}
// p not a multiple of k (a power of two); a null pointer is aligned
inline bool misaligned(const void* p, size_t k) {
  return (reinterpret_cast<uintptr_t>(p) & (k - 1)) != 0;
}

// ---- host-buffer block batches in groups (witness_flow.h, byron_block_api.cpp) ----
// a group's byte budget: the entry's *_group_bytes knob (knobs.h), or its default
inline size_t group_budget(const std::atomic<size_t>& knob, size_t dflt = (size_t)256 << 20) {
  const size_t b = knob.load(std::memory_order_relaxed);
  return b ? b : dflt;
}
// the end of the group of whole blocks that starts at lo: as many as the byte
// budget holds, at least one
inline size_t group_end(const uint32_t* len, size_t n, size_t lo, size_t budget) {
  size_t hi = lo, bytes = 0;
  while (hi < n && (hi == lo || bytes + len[hi] <= budget)) bytes += len[hi++];
  return hi;
}
// a group's raw bytes and spans on the device; the raw buffer is allocated up
// to the next multiple of 4 (the kernels read the aligned dwords a span touches)
struct GroupUp {
  Window w;
  const uint8_t* raw = nullptr;
  const uint64_t* off = nullptr;
  const uint32_t* len = nullptr;
};
inline int group_upload(Stager& sg, hipStream_t st, const uint8_t* raw, const uint64_t* off,
                        const uint32_t* len, size_t m, GroupUp* g) {
  if (int rc = window_of(m, off, len, &g->w)) return rc;
  uint8_t* d = sg.out<uint8_t>(g->w.span() + 4);
  g->off = sg.up(g->w.off.data(), m);
  g->len = sg.up(len, m);
  if (sg.rc) return sg.rc;
  if (g->w.span())
    OURO_HIP(hipMemcpyAsync(d, raw + g->w.lo, g->w.span(), hipMemcpyHostToDevice, st));
  g->raw = d;
  return OURO_OK;
}

}  // namespace ouro_rt
#pragma GCC visibility pop
