// byron_block_api.cpp -- Byron whole-block storage integrity from raw block
// CBOR (include/ouro_verify.h ouro_byron_block_*; cbor_byron_block.h): the
// device sequence over blocks in device memory (byb_count_scan, byb_rows), the
// host-buffer form over it in groups of whole blocks (byb_dev), the host path
// over the same batch (byb_host), and the C entries.  Host code only: kernels
// are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor_block.h"
#include "cbor_byron_block.h"
#include "host_path.h"
#include "host_util.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

using Dev = ByronBlockDev;

// ---- the rows of one sequence as one area, each array 64-byte aligned ----
// a: the area's base, or null to size it only
template <class T>
void put(T** f, uint8_t* a, size_t* at, size_t bytes) {
  if (a) *f = reinterpret_cast<T*>(a + *at);
  *at += cbor::a64(bytes);
}
// ... the part the count pass and the scan fill (n alone sizes it)
size_t carve_counts(uint8_t* a, size_t n, Dev* d) {
  size_t at = 0;
  put(&d->ntx, a, &at, 4 * n);
  put(&d->gather_n, a, &at, 4 * n);
  put(&d->msg_n, a, &at, 4 * n);
  put(&d->sums, a, &at, 24 * scan_tiles(n));
  put(&d->rows, a, &at, 64);
  put(&d->tx_begin, a, &at, 8 * (n + 1));
  put(&d->g_begin, a, &at, 8 * (n + 1));
  put(&d->msg_off, a, &at, 8 * (n + 1));
  return at;
}
// ... and the rest, which the capacities size too.  The gather area and the
// messages end on padding: the hash and signature kernels read the aligned
// dwords a span touches.  device = false: the host path's rows, without
// launch_blake2b's work area.
size_t carve_rows(uint8_t* a, size_t n, size_t T, size_t G, size_t M, Dev* d,
                  bool device = true) {
  size_t at = 0;
  put(&d->pk, a, &at, 32 * n);
  put(&d->sig, a, &at, 64 * n);
  put(&d->genesis_vk, a, &at, 64 * n);
  put(&d->delegate_vk, a, &at, 64 * n);
  put(&d->magic, a, &at, 8 * n);
  put(&d->msg_len, a, &at, 4 * n);
  put(&d->claimed, a, &at, 128 * n);
  put(&d->tx_num, a, &at, 4 * n);
  put(&d->seg_off, a, &at, 16 * n);
  put(&d->seg_len, a, &at, 8 * n);
  put(&d->g_off, a, &at, 8 * n);
  put(&d->g_len, a, &at, 4 * n);
  put(&d->tx_off, a, &at, 8 * T);
  put(&d->tx_len, a, &at, 4 * T);
  put(&d->leaf, a, &at, 32 * T);
  put(&d->root, a, &at, 32 * n);
  put(&d->wit_digest, a, &at, 32 * n);
  put(&d->seg_digest, a, &at, 64 * n);
  put(&d->sig_ok, a, &at, n);
  if (device) put(&d->b2b, a, &at, cbor::b2b_work_bytes(2 * n));
  put(&d->gather, a, &at, G + 64);
  put(&d->msg, a, &at, M + 64);
  return at;
}

// the count pass and the scan over n blocks in device memory, on `st`
int byb_count_scan(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                   const uint32_t* dlen, size_t n, int64_t magic, const Dev& d, size_t T, size_t G,
                   size_t M, uint8_t* dstatus) {
  if (int rc = launch_byron_block_count(st, draw, raw_bytes, doff, dlen, n, magic, dstatus, d.ntx,
                                        d.gather_n, d.msg_n))
    return rc;
  return launch_byron_block_scan(st, n, d.ntx, d.gather_n, d.msg_n, d.sums, d.tx_begin, d.g_begin,
                                 d.msg_off, T, G, M, d.rows);
}
// ... and the rest: emit, the leaf hashes and the Merkle roots, the plain
// hashes (the dlg / upd spans over the raw buffer, the gathered witness lists
// over the gather area), ByronDSIGN over the emitted rows, the finish.  Nothing
// here waits for the host.
int byb_rows(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
             const uint32_t* dlen, size_t n, int64_t magic, const Dev& d, size_t T, size_t G,
             size_t M, uint8_t* dstatus, uint8_t* dverdict, uint8_t* dtx_root) {
  int rc;
  if ((rc = launch_byron_block_emit(st, draw, doff, dlen, n, magic, d.ntx, d.gather_n, d.msg_n,
                                    d.tx_begin, d.g_begin, T, G, M, d, dstatus)))
    return rc;
  if ((rc = launch_byron_leaf_hash(st, T, d.rows, draw, raw_bytes, d.tx_off, d.tx_len, d.leaf)))
    return rc;
  if ((rc = launch_byron_merkle(st, n, dstatus, d.ntx, d.tx_begin, d.leaf, d.root))) return rc;
  if ((rc = launch_blake2b(st, 2 * n, draw, raw_bytes, d.seg_off, d.seg_len, d.seg_digest, d.b2b)))
    return rc;
  if ((rc = launch_blake2b(st, n, d.gather, G, d.g_off, d.g_len, d.wit_digest, d.b2b))) return rc;
  if ((rc = launch_ed(st, n, d.pk, d.sig, d.msg, d.msg_off, d.msg_len, d.sig_ok, 1))) return rc;
  return launch_byron_block_finish(st, n, magic, dstatus, d.ntx, d.tx_num, d.magic, d.claimed,
                                   d.root, d.wit_digest, d.seg_digest, d.sig_ok, dverdict, dtx_root);
}

// ---- argument checks ----
int blocks_check(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                 size_t n, int64_t magic) {
  if (!off || !len || (!raw && raw_bytes)) return fail(OURO_EINVAL, "null argument");
  if (magic < -1 || magic > (int64_t)cbor::kWord32Max)
    return fail(OURO_EINVAL, "protocol_magic outside -1 .. 2^32 - 1");
  if (2 * n > 0xffffffffull) return fail(OURO_EINVAL, "too many blocks in one call");
  return spans_check("block", "raw_bytes", raw_bytes, off, len, n);
}

// ---- the host path ----
int count_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
               uint8_t* status, uint32_t* ntx, uint32_t* gather, uint32_t* msg) {
  return host_rows(n, 64, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      status[i] = cbor::byron_block_count_one(raw, off[i], len[i], magic, &ntx[i], &gather[i],
                                              &msg[i]);
  });
}

// The same walker, the host build of the same hashes and the host ByronDSIGN
// batch, over the task pool, in chunks (no batch-sized area).  Every span was
// checked by the caller.
int byb_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
             uint8_t* status, uint8_t* verdict, uint8_t* tx_root) {
  const size_t C = 1 << 12;
  for (size_t lo = 0; lo < n; lo += C) {
    const size_t m = std::min(C, n - lo);
    const uint64_t* o = off + lo;
    const uint32_t* l = len + lo;
    uint8_t* st = status + lo;
    Dev d{};
    std::unique_ptr<uint8_t[]> mem1(new (std::nothrow) uint8_t[carve_counts(nullptr, m, &d) + 64]);
    if (!mem1) return fail(OURO_EDEVICE, "Byron block host path: out of host memory");
    carve_counts(cbor::arena_base(mem1.get()), m, &d);
    int rc = count_host(raw, o, l, m, magic, st, d.ntx, d.gather_n, d.msg_n);
    if (rc) return rc;
    uint64_t T = 0, G = 0, M = 0;
    for (size_t i = 0; i < m; i++) {
      d.tx_begin[i] = T;
      d.g_begin[i] = G;
      d.msg_off[i] = M;
      T += d.ntx[i];
      G += d.gather_n[i];
      M += d.msg_n[i];
    }
    std::unique_ptr<uint8_t[]> mem2(
        new (std::nothrow) uint8_t[carve_rows(nullptr, m, T, G, M, &d, false) + 64]);
    if (!mem2) return fail(OURO_EDEVICE, "Byron block host path: out of host memory");
    carve_rows(cbor::arena_base(mem2.get()), m, T, G, M, &d, false);
    const cbor::ByronOut bo{d.pk, d.sig, d.genesis_vk, d.delegate_vk, d.msg, d.msg_off, d.magic,
                            d.msg_len};
    const cbor::BybRows rows{d.claimed, d.tx_num, d.seg_off, d.seg_len, d.g_off,
                             d.g_len,   d.tx_off, d.tx_len,  d.gather};
    if ((rc = host_rows(m, 16, [&](size_t r0, size_t r1) {
           for (size_t i = r0; i < r1; i++) {
             uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
             if (st[i] != OURO_PACK_OK) {
               cbor::byron_block_zero_row(bo, rows, i);
               cbor::byb_store8(d.root + 32 * i, w);
               continue;
             }
             const uint64_t t0 = d.tx_begin[i];
             cbor::byron_block_emit_one(raw, o[i], l[i], magic, bo, rows, i, t0, d.g_begin[i],
                                        d.ntx[i], d.gather_n[i]);
             for (uint64_t t = t0; t < t0 + d.ntx[i]; t++) {
               blake2b256_stream_prefixed(w, 0u, 1u, raw + d.tx_off[t], d.tx_len[t]);
               cbor::byb_store8(d.leaf + 32 * t, w);
             }
             cbor::byron_merkle_root(w, d.leaf + 32 * t0, d.ntx[i]);
             cbor::byb_store8(d.root + 32 * i, w);
             blake2b256_stream(w, d.gather + d.g_off[i], d.g_len[i]);
             cbor::byb_store8(d.wit_digest + 32 * i, w);
             for (int q = 0; q < 2; q++) {
               blake2b256_stream(w, raw + d.seg_off[2 * i + q], d.seg_len[2 * i + q]);
               cbor::byb_store8(d.seg_digest + 64 * i + 32 * q, w);
             }
           }
         })))
      return rc;
    if ((rc = ouro_host::ed_batch(m, d.pk, d.sig, d.msg, d.msg_off, d.msg_len, d.sig_ok, 1)))
      return fail(rc, "Byron block host path failed");
    for (size_t i = 0; i < m; i++) {
      const bool hdr_ok = d.sig_ok[i] && (magic < 0 || d.magic[i] == (uint64_t)magic);
      verdict[lo + i] = cbor::byron_block_verdict(
          st[i], d.ntx[i], d.tx_num[i], hdr_ok, d.claimed + 128 * i, d.root + 32 * i,
          d.wit_digest + 32 * i, d.seg_digest + 64 * i, d.seg_digest + 64 * i + 32);
    }
    if (tx_root) memcpy(tx_root + 32 * lo, d.root, 32 * m);
  }
  return OURO_OK;
}

void totals_of(size_t n, const uint32_t* ntx, const uint32_t* gather, const uint32_t* msg,
               uint64_t* totals) {
  totals[0] = totals[1] = totals[2] = 0;
  for (size_t i = 0; i < n; i++) {
    totals[0] += ntx[i];
    totals[1] += gather[i];
    totals[2] += msg[i];
  }
}

// ---- the host-buffer forms on the device ----
size_t budget_bytes() { return group_budget(ouro_knobs::get().byron_block_group_bytes); }

int count_dev(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
              uint8_t* status, uint32_t* ntx, uint32_t* gather, uint32_t* msg) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  const size_t budget = budget_bytes();
  for (size_t lo = 0; lo < n;) {
    const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
    Stager sg{st};
    GroupUp g;
    if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
    auto dst = sg.out<uint8_t>(m);
    auto dc = sg.out<uint32_t>(3 * m);
    if (sg.rc) return sg.rc;
    if ((rc = launch_byron_block_count(st, g.raw, g.w.span(), g.off, g.len, m, magic, dst, dc,
                                       dc + m, dc + 2 * m)))
      return rc;
    std::vector<uint8_t> ts(m);
    std::vector<uint32_t> tc(3 * m);
    if ((rc = download(st, ts.data(), dst, m)) || (rc = download(st, tc.data(), dc, 12 * m)) ||
        (rc = finish(st)))
      return rc;
    memcpy(status + lo, ts.data(), m);
    memcpy(ntx + lo, tc.data(), 4 * m);
    memcpy(gather + lo, tc.data() + m, 4 * m);
    memcpy(msg + lo, tc.data() + 2 * m, 4 * m);
    lo = hi;
  }
  return OURO_OK;
}

// Consecutive groups of whole blocks on the calling thread's stream.  Per
// group: upload, count and scan, read the group's three totals, size the
// group's rows from them (so nothing passes a capacity), the rest of the
// sequence, copy back.
int byb_dev(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
            uint8_t* status, uint8_t* verdict, uint8_t* tx_root) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  const size_t budget = budget_bytes();
  for (size_t lo = 0; lo < n;) {
    const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
    Stager sg{st};
    GroupUp g;
    if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
    Dev d{};
    uint8_t* a1 = sg.out<uint8_t>(carve_counts(nullptr, m, &d) + 64);
    auto dst = sg.out<uint8_t>(m);
    auto dver = sg.out<uint8_t>(m);
    auto droot = sg.out<uint8_t>(32 * m);
    if (sg.rc) return sg.rc;
    carve_counts(cbor::arena_base(a1), m, &d);
    // (no capacity yet: the row counts are the group's totals)
    if ((rc = byb_count_scan(st, g.raw, g.w.span(), g.off, g.len, m, magic, d, ~(size_t)0,
                             ~(size_t)0, ~(size_t)0, dst)))
      return rc;
    uint64_t tot[6];
    if ((rc = download(st, tot, d.rows, sizeof tot)) || (rc = finish(st))) return rc;
    const size_t T = (size_t)tot[3], G = (size_t)tot[4], M = (size_t)tot[5];
    uint8_t* a2 = sg.out<uint8_t>(carve_rows(nullptr, m, T, G, M, &d) + 64);
    if (sg.rc) return sg.rc;
    carve_rows(cbor::arena_base(a2), m, T, G, M, &d);
    if ((rc = byb_rows(st, g.raw, g.w.span(), g.off, g.len, m, magic, d, T, G, M, dst, dver, droot)))
      return rc;
    std::vector<uint8_t> ts(m), tv(m), tr(32 * m);
    if ((rc = download(st, ts.data(), dst, m)) || (rc = download(st, tv.data(), dver, m)) ||
        (rc = download(st, tr.data(), droot, 32 * m)) || (rc = finish(st)))
      return rc;
    memcpy(status + lo, ts.data(), m);
    memcpy(verdict + lo, tv.data(), m);
    if (tx_root) memcpy(tx_root + 32 * lo, tr.data(), 32 * m);
    lo = hi;
  }
  return OURO_OK;
}

int verify_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                size_t n, int64_t magic, uint8_t* status, uint8_t* verdict, uint8_t* tx_root,
                bool host) {
  if (n == 0) return OURO_OK;
  if (!status || !verdict) return fail(OURO_EINVAL, "null argument");
  if (int rc = blocks_check(raw, raw_bytes, off, len, n, magic)) return rc;
  auto on_host = [&] { return byb_host(raw, off, len, n, magic, status, verdict, tx_root); };
  return host ? on_host()
              : or_host(byb_dev(raw, off, len, n, magic, status, verdict, tx_root), on_host);
}

int count_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
               size_t n, int64_t magic, uint8_t* status, uint32_t* ntx, uint32_t* gather,
               uint32_t* msg, uint64_t* totals, bool host) {
  if (!totals) return fail(OURO_EINVAL, "null argument");
  if (n == 0) {
    totals[0] = totals[1] = totals[2] = 0;
    return OURO_OK;
  }
  if (!status || !ntx || !gather || !msg) return fail(OURO_EINVAL, "null argument");
  if (int rc = blocks_check(raw, raw_bytes, off, len, n, magic)) return rc;
  auto on_host = [&] { return count_host(raw, off, len, n, magic, status, ntx, gather, msg); };
  const int rc = host ? on_host()
                      : or_host(count_dev(raw, off, len, n, magic, status, ntx, gather, msg),
                                on_host);
  if (rc == OURO_OK) totals_of(n, ntx, gather, msg, totals);
  return rc;
}

}  // namespace

extern "C" {

int ouro_byron_block_count_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                const uint32_t* len, size_t n, int64_t protocol_magic,
                                uint8_t* status, uint32_t* ntx, uint32_t* gather_bytes,
                                uint32_t* msg_bytes, uint64_t* totals) {
  return count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, gather_bytes,
                    msg_bytes, totals, false);
}

int ouro_byron_block_count_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                     const uint32_t* len, size_t n, int64_t protocol_magic,
                                     uint8_t* status, uint32_t* ntx, uint32_t* gather_bytes,
                                     uint32_t* msg_bytes, uint64_t* totals) {
  return count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, gather_bytes,
                    msg_bytes, totals, true);
}

int ouro_byron_block_integrity_verify_cbor(const uint8_t* raw, size_t raw_bytes,
                                           const uint64_t* off, const uint32_t* len, size_t n,
                                           int64_t protocol_magic, uint8_t* status,
                                           uint8_t* verdict, uint8_t* tx_root) {
  return verify_call(raw, raw_bytes, off, len, n, protocol_magic, status, verdict, tx_root, false);
}

int ouro_byron_block_integrity_verify_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                                const uint64_t* off, const uint32_t* len,
                                                size_t n, int64_t protocol_magic,
                                                uint8_t* status, uint8_t* verdict,
                                                uint8_t* tx_root) {
  return verify_call(raw, raw_bytes, off, len, n, protocol_magic, status, verdict, tx_root, true);
}

size_t ouro_byron_block_work_bytes(size_t n, size_t tx_cap, size_t gather_cap, size_t msg_cap) {
  Dev d{};
  return carve_counts(nullptr, n, &d) + carve_rows(nullptr, n, tx_cap, gather_cap, msg_cap, &d) + 64;
}

int ouro_byron_block_integrity_verify_cbor_device(void* stream, const uint8_t* raw,
                                                  size_t raw_bytes, const uint64_t* off,
                                                  const uint32_t* len, size_t n,
                                                  int64_t protocol_magic, size_t tx_cap,
                                                  size_t gather_cap, size_t msg_cap, void* work,
                                                  size_t work_bytes, uint8_t* status,
                                                  uint8_t* verdict, uint8_t* tx_root) {
  if (n == 0) return OURO_OK;
  if (!raw || !off || !len || !work || !status || !verdict)
    return fail(OURO_EINVAL, "null argument");
  if (protocol_magic < -1 || protocol_magic > (int64_t)cbor::kWord32Max)
    return fail(OURO_EINVAL, "protocol_magic outside -1 .. 2^32 - 1");
  if (2 * n > 0xffffffffull || tx_cap > 0xffffffffull)
    return fail(OURO_EINVAL, "too many blocks or transaction rows in one call");
  if (work_bytes < ouro_byron_block_work_bytes(n, tx_cap, gather_cap, msg_cap))
    return fail(OURO_EINVAL, "work area too small");
  if (misaligned(raw, 4)) return fail(OURO_EINVAL, "raw must be 4-byte aligned");
  if (misaligned(off, 8) || misaligned(len, 4))
    return fail(OURO_EINVAL, "off must be 8-byte and len 4-byte aligned");
  if (misaligned(tx_root, 16)) return fail(OURO_EINVAL, "tx_root must be 16-byte aligned");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  uint8_t* a = cbor::arena_base(work);
  Dev d{};
  a += carve_counts(a, n, &d);
  carve_rows(a, n, tx_cap, gather_cap, msg_cap, &d);
  if (int rc = byb_count_scan(st, raw, raw_bytes, off, len, n, protocol_magic, d, tx_cap,
                              gather_cap, msg_cap, status))
    return rc;
  return byb_rows(st, raw, raw_bytes, off, len, n, protocol_magic, d, tx_cap, gather_cap, msg_cap,
                  status, verdict, tx_root);
}

}  // extern "C"
