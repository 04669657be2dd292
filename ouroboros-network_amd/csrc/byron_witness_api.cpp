// byron_witness_api.cpp -- Byron transaction witnesses from raw block CBOR
// (include/ouro_verify.h ouro_byron_block_witness_*; cbor_byron_witness.h): the
// device sequence over blocks in device memory (byw_count_scan, byw_rows), the
// host-buffer form over it in groups of whole blocks (byw_dev), the host path
// over the same batch (byw_host), and the C entries.  It follows
// witness_api.cpp step for step; what differs is the magic, the 64-byte key
// rows, the message (built per row, not the bare tx id) and the EBB's verdict.
// Host code only: kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor_block.h"
#include "cbor_byron_witness.h"
#include "host_path.h"
#include "host_util.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

using Out = ouro_byron_block_witness_out;
constexpr size_t kGroupBytes = (size_t)256 << 20;  // OURO_BYRON_WITNESS_GROUP_BYTES' default
constexpr uint32_t kMsgSlot = 40;                  // a signed message has at most 8 + 32 bytes

// the work of one device sequence: counts, the scan's tile sums and row
// counts, the blocks' magics, the tx spans, the witness keys and signatures,
// the hash work area
struct BywDev {
  uint32_t *ntx, *nwit;
  uint64_t *sums, *rows, *magic;
  uint64_t* tx_off;
  uint32_t* tx_len;
  uint8_t *vk, *sig;
  void* b2b;
};
// ... as one area (ouro_byron_block_witness_work_bytes), each part 64-byte aligned
struct BywLayout {
  size_t ntx, nwit, sums, rows, magic, tx_off, tx_len, vk, sig, b2b, total;
};
BywLayout byw_layout(size_t n, size_t tx_cap, size_t wit_cap) {
  using cbor::a64;
  BywLayout l{};
  size_t at = 0;
  l.ntx = at;
  at += a64(4 * n);
  l.nwit = at;
  at += a64(4 * n);
  l.sums = at;
  at += a64(16 * byron_witness_scan_tiles(n));
  l.rows = at;
  at += 64;
  l.magic = at;
  at += a64(8 * n);
  l.tx_off = at;
  at += a64(8 * tx_cap);
  l.tx_len = at;
  at += a64(4 * tx_cap);
  l.vk = at;
  at += a64(64 * wit_cap);
  l.sig = at;
  at += a64(64 * wit_cap);
  l.b2b = at;
  at += cbor::b2b_work_bytes(tx_cap);
  l.total = at;
  return l;
}

// the count pass and the scan over n blocks in device memory, on `st`
int byw_count_scan(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                   const uint32_t* dlen, size_t n, const BywDev& d, uint64_t* tx_begin,
                   uint64_t* wit_begin, size_t tx_cap, size_t wit_cap, uint8_t* dstatus) {
  if (int rc = launch_byron_witness_count(st, draw, raw_bytes, doff, dlen, n, dstatus, d.ntx,
                                          d.nwit))
    return rc;
  return launch_byron_witness_scan(st, n, d.ntx, d.nwit, d.sums, tx_begin, wit_begin, tx_cap,
                                   wit_cap, d.rows);
}
// ... and the rest: emit, the tx ids, the witness verification, the finish.
// o: device pointers; nothing here waits for the host -- the later kernels
// read the row counts the scan left in d.rows
int byw_rows(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
             const uint32_t* dlen, size_t n, int64_t magic, const BywDev& d, const Out& o,
             uint64_t tx_base, uint8_t* dstatus, uint8_t* dverdict, uint32_t* dn_bad) {
  int rc;
  if ((rc = launch_byron_witness_emit(st, draw, doff, dlen, n, magic, d.ntx, d.nwit, o.tx_begin,
                                      o.wit_begin, o.tx_cap, o.wit_cap, tx_base, d.tx_off, d.tx_len,
                                      d.vk, d.sig, o.wit_tx, o.wit_kind, d.magic, dstatus)))
    return rc;
  if ((rc = launch_blake2b(st, o.tx_cap, draw, raw_bytes, d.tx_off, d.tx_len, o.tx_id, d.b2b)))
    return rc;
  if ((rc = launch_byron_witness_verify(st, o.wit_cap, d.rows, d.vk, d.sig, o.wit_tx, o.tx_id,
                                        o.tx_cap, tx_base, o.wit_begin, n, d.magic, o.wit_kind,
                                        o.wit_ok)))
    return rc;
  return launch_byron_witness_finish(st, n, dstatus, o.wit_begin, o.wit_ok, o.wit_cap, dverdict,
                                     dn_bad);
}

// ---- argument checks ----
int magic_check(int64_t magic) {
  if (magic < -1 || magic > (int64_t)cbor::kWord32Max)
    return fail(OURO_EINVAL, "protocol_magic outside -1 .. 2^32 - 1");
  return OURO_OK;
}
int blocks_check(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                 size_t n, int64_t magic) {
  if (!off || !len || (!raw && raw_bytes)) return fail(OURO_EINVAL, "null argument");
  if (int rc = magic_check(magic)) return rc;
  return spans_check("block", "raw_bytes", raw_bytes, off, len, n);
}
int out_check(const Out* o) {
  if (!o || !o->tx_begin || !o->wit_begin) return fail(OURO_EINVAL, "null argument");
  if (o->tx_cap && !o->tx_id) return fail(OURO_EINVAL, "null tx_id");
  if (o->wit_cap && (!o->wit_tx || !o->wit_kind || !o->wit_ok))
    return fail(OURO_EINVAL, "null witness array");
  if (o->tx_cap > 0xffffffffull || o->wit_cap > 0xffffffffull)
    return fail(OURO_EINVAL, "a capacity above 2^32 - 1 rows");
  return OURO_OK;
}

// A sliced block fits iff its rows end inside both capacities; the blocks that
// fit are a prefix of the sliced ones (the begins only grow).
bool fits(const Out& o, uint64_t t0, uint64_t nt, uint64_t w0, uint64_t nw) {
  return t0 <= o.tx_cap && o.tx_cap - t0 >= nt && w0 <= o.wit_cap && o.wit_cap - w0 >= nw;
}

// ---- the host path ----
int count_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
               uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
  return host_rows(n, 64, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      status[i] = cbor::byron_witness_count_one(raw, off[i], len[i], &ntx[i], &nwit[i]);
  });
}

// The same walker, the host build of the streaming Blake2b and the host
// ByronDSIGN batch, over the task pool.  Every span was checked by the caller.
int byw_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
             const Out& o, uint8_t* status, uint8_t* verdict, uint32_t* n_bad) {
  std::vector<uint32_t> ntx(n), nwit(n);
  int rc = count_host(raw, off, len, n, status, ntx.data(), nwit.data());
  if (rc) return rc;
  uint64_t T = 0, W = 0, t = 0, w = 0;  // the rows that fit; the running totals
  for (size_t i = 0; i < n; i++) {
    o.tx_begin[i] = t;
    o.wit_begin[i] = w;
    if (status[i] == OURO_PACK_OK) {
      if (fits(o, t, ntx[i], w, nwit[i])) {
        T = t + ntx[i];
        W = w + nwit[i];
      } else {
        status[i] = OURO_PACK_ECAP;
      }
    }
    t += ntx[i];
    w += nwit[i];
  }
  o.tx_begin[n] = t;
  o.wit_begin[n] = w;
  std::vector<uint64_t> tx_off(T), msg_off(W), bmagic(n);
  std::vector<uint32_t> tx_len(T), msg_len(W);
  std::vector<uint8_t> sig(64 * W), vk_own(o.wit_vk ? 0 : 64 * W), pk(32 * W), msg(kMsgSlot * W);
  const cbor::BywRows rows{tx_off.data(), tx_len.data(), o.wit_vk ? o.wit_vk : vk_own.data(),
                           sig.data(), o.wit_tx, o.wit_kind, 0};
  if ((rc = host_rows(n, 64, [&](size_t lo, size_t hi) {
         for (size_t i = lo; i < hi; i++)
           if (status[i] == OURO_PACK_OK) {
             cbor::byron_witness_emit_one(raw, off[i], len[i], rows, o.tx_begin[i], o.wit_begin[i],
                                          ntx[i], nwit[i], &bmagic[i]);
             if (magic >= 0) bmagic[i] = (uint64_t)magic;
           }
       })))
    return rc;
  if ((rc = host_rows((size_t)T, 256, [&](size_t lo, size_t hi) {
         for (size_t r = lo; r < hi; r++) {
           uint32_t d[8];
           blake2b256_stream(d, raw + tx_off[r], tx_len[r]);
           digest_bytes(o.tx_id + 32 * r, d);
         }
       })))
    return rc;
  // the rows' messages and 32-byte keys (the blocks that fit own rows 0 .. W)
  if ((rc = host_rows(n, 64, [&](size_t lo, size_t hi) {
         for (size_t i = lo; i < hi; i++) {
           if (status[i] != OURO_PACK_OK) continue;
           for (uint64_t r = o.wit_begin[i]; r < o.wit_begin[i] + nwit[i]; r++) {
             msg_off[r] = kMsgSlot * r;
             msg_len[r] = cbor::byron_witness_message(msg.data() + kMsgSlot * r, o.wit_kind[r],
                                                      bmagic[i], o.tx_id + 32 * (size_t)o.wit_tx[r]);
             memcpy(pk.data() + 32 * r, rows.vk + 64 * r, 32);
           }
         }
       })))
    return rc;
  if (W && (rc = ouro_host::ed_batch((size_t)W, pk.data(), sig.data(), msg.data(), msg_off.data(),
                                     msg_len.data(), o.wit_ok, 1)))
    return fail(rc, "Byron witness host path failed");
  for (size_t i = 0; i < n; i++) {
    uint32_t bad = 0;
    if (status[i] == OURO_PACK_OK)
      for (uint64_t r = o.wit_begin[i]; r < o.wit_begin[i + 1]; r++) bad += o.wit_ok[r] ? 0 : 1;
    n_bad[i] = bad;
    verdict[i] = (status[i] == OURO_PACK_OK && bad == 0) || status[i] == OURO_PACK_EBB
                     ? OURO_BYW_ALL_OK
                     : 0;
  }
  return OURO_OK;
}

// ---- the host-buffer forms on the device ----
size_t group_budget() {
  const size_t b = ouro_knobs::get().byron_witness_group_bytes.load(std::memory_order_relaxed);
  return b ? b : kGroupBytes;
}
// (the groups of whole blocks and their upload: host_util.h group_end, group_upload)

int count_dev(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
              uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  const size_t budget = group_budget();
  for (size_t lo = 0; lo < n;) {
    const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
    Stager sg{st};
    GroupUp g;
    if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
    auto dst = sg.out<uint8_t>(m);
    auto da = sg.out<uint32_t>(m);
    auto db = sg.out<uint32_t>(m);
    if (sg.rc) return sg.rc;
    if ((rc = launch_byron_witness_count(st, g.raw, g.w.span(), g.off, g.len, m, dst, da, db)))
      return rc;
    std::vector<uint8_t> ts(m);
    std::vector<uint32_t> ta(m), tb(m);
    if ((rc = download(st, ts.data(), dst, m)) || (rc = download(st, ta.data(), da, 4 * m)) ||
        (rc = download(st, tb.data(), db, 4 * m)) || (rc = finish(st)))
      return rc;
    memcpy(status + lo, ts.data(), m);
    memcpy(ntx + lo, ta.data(), 4 * m);
    memcpy(nwit + lo, tb.data(), 4 * m);
    lo = hi;
  }
  return OURO_OK;
}

// Consecutive groups of whole blocks on the calling thread's stream.  Per
// group: upload, count and scan, read the group's totals, size the group's
// rows from them, the rest of the sequence, copy back.  The begins of a later
// group continue the earlier ones (tx_base / wit_base), and the capacities are
// applied here, to the global rows.
int byw_dev(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
            const Out& o, uint8_t* status, uint8_t* verdict, uint32_t* n_bad) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  const size_t budget = group_budget();
  uint64_t tx_base = 0, wit_base = 0;
  for (size_t lo = 0; lo < n;) {
    const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
    Stager sg{st};
    GroupUp g;
    if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
    BywDev d{};
    d.ntx = sg.out<uint32_t>(m);
    d.nwit = sg.out<uint32_t>(m);
    d.sums = sg.out<uint64_t>(2 * byron_witness_scan_tiles(m) + 4);
    d.magic = sg.out<uint64_t>(m);
    auto dst = sg.out<uint8_t>(m);
    auto dtb = sg.out<uint64_t>(m + 1);
    auto dwb = sg.out<uint64_t>(m + 1);
    if (sg.rc) return sg.rc;
    d.rows = d.sums + 2 * byron_witness_scan_tiles(m);
    // (no capacity yet: the row counts are the group's totals)
    if ((rc = byw_count_scan(st, g.raw, g.w.span(), g.off, g.len, m, d, dtb, dwb, ~(size_t)0,
                             ~(size_t)0, dst)))
      return rc;
    std::vector<uint64_t> tb(m + 1), wb(m + 1);
    if ((rc = download(st, tb.data(), dtb, 8 * (m + 1))) ||
        (rc = download(st, wb.data(), dwb, 8 * (m + 1))) || (rc = finish(st)))
      return rc;
    const size_t T = (size_t)tb[m], W = (size_t)wb[m];
    if (tx_base + T > 0xffffffffull) return fail(OURO_EINVAL, "more than 2^32 - 1 transactions");
    Out go{};  // the group's rows, all of them: device pointers
    go.tx_cap = T;
    go.wit_cap = W;
    go.tx_begin = dtb;
    go.wit_begin = dwb;
    d.tx_off = sg.out<uint64_t>(T);
    d.tx_len = sg.out<uint32_t>(T);
    d.vk = sg.out<uint8_t>(64 * W);
    d.sig = sg.out<uint8_t>(64 * W);
    d.b2b = sg.out<uint8_t>(cbor::b2b_work_bytes(T));
    go.tx_id = sg.out<uint8_t>(32 * T);
    go.wit_tx = sg.out<uint32_t>(W);
    go.wit_kind = sg.out<uint8_t>(W);
    go.wit_ok = sg.out<uint8_t>(W);
    auto dver = sg.out<uint8_t>(m);
    auto dbad = sg.out<uint32_t>(m);
    if (sg.rc) return sg.rc;
    if ((rc = byw_rows(st, g.raw, g.w.span(), g.off, g.len, m, magic, d, go, tx_base, dst, dver,
                       dbad)))
      return rc;
    std::vector<uint8_t> ts(m), tv(m), tid(32 * T), tk(W), tok(W), tvk(o.wit_vk ? 64 * W : 0);
    std::vector<uint32_t> tbad(m), twt(W);
    if ((rc = download(st, ts.data(), dst, m)) || (rc = download(st, tv.data(), dver, m)) ||
        (rc = download(st, tbad.data(), dbad, 4 * m)) ||
        (rc = download(st, tid.data(), go.tx_id, 32 * T)) ||
        (rc = download(st, twt.data(), go.wit_tx, 4 * W)) ||
        (rc = download(st, tk.data(), go.wit_kind, W)) ||
        (rc = download(st, tok.data(), go.wit_ok, W)) ||
        (rc = download(st, tvk.data(), d.vk, tvk.size())) || (rc = finish(st)))
      return rc;
    // the group's blocks into the caller's arrays; its rows as far as they fit
    size_t Tf = 0, Wf = 0;
    for (size_t i = 0; i < m; i++) {
      o.tx_begin[lo + i] = tx_base + tb[i];
      o.wit_begin[lo + i] = wit_base + wb[i];
      status[lo + i] = ts[i];
      verdict[lo + i] = tv[i];
      n_bad[lo + i] = tbad[i];
      if (ts[i] != OURO_PACK_OK) continue;
      if (fits(o, tx_base + tb[i], tb[i + 1] - tb[i], wit_base + wb[i], wb[i + 1] - wb[i])) {
        Tf = (size_t)tb[i + 1];
        Wf = (size_t)wb[i + 1];
      } else {
        status[lo + i] = OURO_PACK_ECAP;
        verdict[lo + i] = 0;
        n_bad[lo + i] = 0;
      }
    }
    if (Tf) memcpy(o.tx_id + 32 * tx_base, tid.data(), 32 * Tf);
    if (Wf) {
      memcpy(o.wit_tx + wit_base, twt.data(), 4 * Wf);
      memcpy(o.wit_kind + wit_base, tk.data(), Wf);
      memcpy(o.wit_ok + wit_base, tok.data(), Wf);
      if (o.wit_vk) memcpy(o.wit_vk + 64 * wit_base, tvk.data(), 64 * Wf);
    }
    tx_base += T;
    wit_base += W;
    lo = hi;
  }
  o.tx_begin[n] = tx_base;
  o.wit_begin[n] = wit_base;
  return OURO_OK;
}

int verify_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                size_t n, int64_t magic, const Out* out, uint8_t* status, uint8_t* verdict,
                uint32_t* n_bad, bool host) {
  if (int rc = out_check(out)) return rc;
  if (int rc = magic_check(magic)) return rc;
  if (n == 0) {
    out->tx_begin[0] = out->wit_begin[0] = 0;
    return OURO_OK;
  }
  if (!status || !verdict || !n_bad) return fail(OURO_EINVAL, "null argument");
  if (int rc = blocks_check(raw, raw_bytes, off, len, n, magic)) return rc;
  auto on_host = [&] { return byw_host(raw, off, len, n, magic, *out, status, verdict, n_bad); };
  return host ? on_host()
              : or_host(byw_dev(raw, off, len, n, magic, *out, status, verdict, n_bad), on_host);
}

int count_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
               size_t n, int64_t magic, uint8_t* status, uint32_t* ntx, uint32_t* nwit, bool host) {
  if (int rc = magic_check(magic)) return rc;
  if (n == 0) return OURO_OK;
  if (!status || !ntx || !nwit) return fail(OURO_EINVAL, "null argument");
  if (int rc = blocks_check(raw, raw_bytes, off, len, n, magic)) return rc;
  auto on_host = [&] { return count_host(raw, off, len, n, status, ntx, nwit); };
  return host ? on_host() : or_host(count_dev(raw, off, len, n, status, ntx, nwit), on_host);
}

}  // namespace

extern "C" {

int ouro_byron_block_witness_count_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                        const uint32_t* len, size_t n, int64_t protocol_magic,
                                        uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
  return count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, nwit, false);
}

int ouro_byron_block_witness_count_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                             const uint64_t* off, const uint32_t* len, size_t n,
                                             int64_t protocol_magic, uint8_t* status,
                                             uint32_t* ntx, uint32_t* nwit) {
  return count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, nwit, true);
}

int ouro_byron_block_witness_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                         const uint32_t* len, size_t n, int64_t protocol_magic,
                                         const ouro_byron_block_witness_out* out, uint8_t* status,
                                         uint8_t* verdict, uint32_t* n_bad) {
  return verify_call(raw, raw_bytes, off, len, n, protocol_magic, out, status, verdict, n_bad,
                     false);
}

int ouro_byron_block_witness_verify_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                              const uint64_t* off, const uint32_t* len, size_t n,
                                              int64_t protocol_magic,
                                              const ouro_byron_block_witness_out* out,
                                              uint8_t* status, uint8_t* verdict, uint32_t* n_bad) {
  return verify_call(raw, raw_bytes, off, len, n, protocol_magic, out, status, verdict, n_bad, true);
}

size_t ouro_byron_block_witness_work_bytes(size_t n, size_t tx_cap, size_t wit_cap) {
  return byw_layout(n, tx_cap, wit_cap).total + 64;
}

int ouro_byron_block_witness_verify_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                                const uint64_t* off, const uint32_t* len, size_t n,
                                                int64_t protocol_magic,
                                                const ouro_byron_block_witness_out* out, void* work,
                                                size_t work_bytes, uint8_t* status,
                                                uint8_t* verdict, uint32_t* n_bad) {
  if (int rc = out_check(out)) return rc;
  if (int rc = magic_check(protocol_magic)) return rc;
  if (n == 0) return OURO_OK;
  if (!raw || !off || !len || !work || !status || !verdict || !n_bad)
    return fail(OURO_EINVAL, "null argument");
  if (work_bytes < ouro_byron_block_witness_work_bytes(n, out->tx_cap, out->wit_cap))
    return fail(OURO_EINVAL, "work area too small");
  if (misaligned(raw, 4)) return fail(OURO_EINVAL, "raw must be 4-byte aligned");
  if (misaligned(out->tx_begin, 8) || misaligned(out->wit_begin, 8) || misaligned(off, 8))
    return fail(OURO_EINVAL, "off, tx_begin and wit_begin must be 8-byte aligned");
  if (misaligned(out->tx_id, 16) || misaligned(out->wit_vk, 16))
    return fail(OURO_EINVAL, "tx_id and wit_vk must be 16-byte aligned");
  if (misaligned(out->wit_tx, 4) || misaligned(n_bad, 4) || misaligned(len, 4))
    return fail(OURO_EINVAL, "len, wit_tx and n_bad must be 4-byte aligned");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  uint8_t* a = cbor::arena_base(work);
  const BywLayout l = byw_layout(n, out->tx_cap, out->wit_cap);
  BywDev d;
  d.ntx = reinterpret_cast<uint32_t*>(a + l.ntx);
  d.nwit = reinterpret_cast<uint32_t*>(a + l.nwit);
  d.sums = reinterpret_cast<uint64_t*>(a + l.sums);
  d.rows = reinterpret_cast<uint64_t*>(a + l.rows);
  d.magic = reinterpret_cast<uint64_t*>(a + l.magic);
  d.tx_off = reinterpret_cast<uint64_t*>(a + l.tx_off);
  d.tx_len = reinterpret_cast<uint32_t*>(a + l.tx_len);
  d.vk = out->wit_vk ? out->wit_vk : a + l.vk;
  d.sig = a + l.sig;
  d.b2b = a + l.b2b;
  if (int rc = byw_count_scan(st, raw, raw_bytes, off, len, n, d, out->tx_begin, out->wit_begin,
                              out->tx_cap, out->wit_cap, status))
    return rc;
  return byw_rows(st, raw, raw_bytes, off, len, n, protocol_magic, d, *out, 0, status, verdict,
                  n_bad);
}

}  // extern "C"
