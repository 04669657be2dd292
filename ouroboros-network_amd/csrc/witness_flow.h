// witness_flow.h -- the transaction-witness entries' host flow, written once
// for both eras (witness_api.cpp: Shelley, byron_witness_api.cpp: Byron): the
// work-area layout, the device sequence over blocks in device memory
// (count_scan, rows), the host-buffer form over it in groups of whole blocks
// (on_device), the host path over the same batch (on_host), the argument
// checks and the bodies of the C entries.  Host units only, like host_util.h:
// kernels are reached through launches.h.
//
// Flow<E> is instantiated on an era description E:
//   Out, Rows     the public out struct (both eras: the same fields) and the
//                 walker's row struct (cbor_witness.h, cbor_byron_witness.h)
//   kKey          a witness key row's width: 32, Byron 64
//   kBlockMagic   whether every block has a magic of its own for its messages
//   kAllOk, kEbbOk  the all-OK verdict; whether an EBB has it too
//   count, scan, emit, verify, finish   the era's launches (launches.h)
//   budget()      the group byte budget (the era's knob)
//   magic_check(magic)   the check of the configured magic, in front of the
//                 others that follow the out struct's
//   count_one, emit_one  the walker's passes on the host (emit_one: the
//                 block's magic to *bmagic where kBlockMagic)
//   verify_host(h)  the host message step: wit_ok of the rows that fit
#pragma once
#include <cstring>
#include <vector>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor_block.h"
#include "host_path.h"
#include "host_util.h"
#include "launches.h"

#pragma GCC visibility push(hidden)
namespace ouro_rt {

// what verify_host sees: the blocks (bmagic: null unless kBlockMagic), the
// caller's rows, and the keys and signatures of the W witness rows that fit
template <class Out>
struct WitnessHostRows {
  size_t n;
  const uint8_t* status;
  const uint32_t* nwit;
  const uint64_t* bmagic;
  const Out& o;
  size_t W;
  const uint8_t *vk, *sig;
};

template <class E>
struct WitnessFlow {
  using Out = typename E::Out;

  // ---- the work of one device sequence as one area, each part 64-byte
  // aligned (launches.h WitnessDev); a: the area's base, or null to size it ----
  template <class T>
  static void put(T** f, uint8_t* a, size_t* at, size_t bytes) {
    if (a) *f = reinterpret_cast<T*>(a + *at);
    *at += ouro::cbor::a64(bytes);
  }
  static size_t carve(uint8_t* a, size_t n, size_t tx_cap, size_t wit_cap, WitnessDev* d) {
    static_assert(8 * scan_rows_words(kWitnessVals) <= 64, "the scan's rows have 64 bytes");
    size_t at = 0;
    put(&d->ntx, a, &at, 4 * n);
    put(&d->nwit, a, &at, 4 * n);
    put(&d->sums, a, &at, 8 * kWitnessVals * scan_tiles(n));
    put(&d->rows, a, &at, 64);
    if (E::kBlockMagic) put(&d->magic, a, &at, 8 * n);
    put(&d->tx_off, a, &at, 8 * tx_cap);
    put(&d->tx_len, a, &at, 4 * tx_cap);
    put(&d->vk, a, &at, E::kKey * wit_cap);
    put(&d->sig, a, &at, 64 * wit_cap);
    put(&d->b2b, a, &at, ouro::cbor::b2b_work_bytes(tx_cap));
    return at;
  }
  static size_t work_bytes(size_t n, size_t tx_cap, size_t wit_cap) {
    WitnessDev d{};
    return carve(nullptr, n, tx_cap, wit_cap, &d) + 64;
  }
  // the rows of a call (o: device pointers) as the launches take them
  static void rows_of(const Out& o, uint64_t tx_base, WitnessDev* d) {
    d->tx_cap = o.tx_cap;
    d->wit_cap = o.wit_cap;
    d->tx_begin = o.tx_begin;
    d->wit_begin = o.wit_begin;
    d->tx_base = tx_base;
    d->tx_id = o.tx_id;
    d->wit_tx = o.wit_tx;
    d->kind = o.wit_kind;
    d->wit_ok = o.wit_ok;
  }

  // the count pass and the scan over n blocks in device memory, on `st`
  static int count_scan(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                        const uint32_t* dlen, size_t n, const WitnessDev& d, uint8_t* dstatus) {
    if (int rc = E::count(st, draw, raw_bytes, doff, dlen, n, dstatus, d.ntx, d.nwit)) return rc;
    return E::scan(st, n, d);
  }
  // ... and the rest: emit, the tx ids, the witness verification, the finish.
  // Nothing here waits for the host -- the later kernels read the row counts
  // the scan left in d.rows
  static int rows(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                  const uint32_t* dlen, size_t n, int64_t magic, const WitnessDev& d,
                  uint8_t* dstatus, uint8_t* dverdict, uint32_t* dn_bad) {
    int rc;
    if ((rc = E::emit(st, draw, doff, dlen, n, magic, d, dstatus))) return rc;
    if ((rc = launch_blake2b(st, d.tx_cap, draw, raw_bytes, d.tx_off, d.tx_len, d.tx_id, d.b2b)))
      return rc;
    if ((rc = E::verify(st, n, d))) return rc;
    return E::finish(st, n, dstatus, d, dverdict, dn_bad);
  }

  // ---- argument checks ----
  static int blocks_check(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                          const uint32_t* len, size_t n) {
    if (!off || !len || (!raw && raw_bytes)) return fail(OURO_EINVAL, "null argument");
    return spans_check("block", "raw_bytes", raw_bytes, off, len, n);
  }
  static int out_check(const Out* o) {
    if (!o || !o->tx_begin || !o->wit_begin) return fail(OURO_EINVAL, "null argument");
    if (o->tx_cap && !o->tx_id) return fail(OURO_EINVAL, "null tx_id");
    if (o->wit_cap && (!o->wit_tx || !o->wit_kind || !o->wit_ok))
      return fail(OURO_EINVAL, "null witness array");
    if (o->tx_cap > 0xffffffffull || o->wit_cap > 0xffffffffull)
      return fail(OURO_EINVAL, "a capacity above 2^32 - 1 rows");
    return OURO_OK;
  }

  // A sliced block fits iff its rows end inside both capacities; the blocks
  // that fit are a prefix of the sliced ones (the begins only grow).
  static bool fits(const Out& o, uint64_t t0, uint64_t nt, uint64_t w0, uint64_t nw) {
    return t0 <= o.tx_cap && o.tx_cap - t0 >= nt && w0 <= o.wit_cap && o.wit_cap - w0 >= nw;
  }

  // ---- the host path ----
  static int count_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                        uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
    return host_rows(n, 64, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++)
        status[i] = E::count_one(raw, off[i], len[i], &ntx[i], &nwit[i]);
    });
  }

  // The same walker, the host build of the streaming Blake2b and the host
  // signature batch, over the task pool.  Every span was checked by the
  // caller.  The rows are written through the walker's row struct, o.wit_vk's
  // included when the caller passes one.
  static int on_host(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                     int64_t magic, const Out& o, uint8_t* status, uint8_t* verdict,
                     uint32_t* n_bad) {
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
    std::vector<uint64_t> tx_off(T), bmagic(E::kBlockMagic ? n : 0);
    std::vector<uint32_t> tx_len(T);
    std::vector<uint8_t> sig(64 * W), vk_own(o.wit_vk ? 0 : E::kKey * W);
    const typename E::Rows r{tx_off.data(), tx_len.data(), o.wit_vk ? o.wit_vk : vk_own.data(),
                             sig.data(), o.wit_tx, o.wit_kind, 0};
    if ((rc = host_rows(n, 64, [&](size_t lo, size_t hi) {
           for (size_t i = lo; i < hi; i++)
             if (status[i] == OURO_PACK_OK)
               E::emit_one(raw, off[i], len[i], r, o.tx_begin[i], o.wit_begin[i], ntx[i], nwit[i],
                           magic, E::kBlockMagic ? &bmagic[i] : nullptr);
         })))
      return rc;
    if ((rc = host_rows((size_t)T, 256, [&](size_t lo, size_t hi) {
           for (size_t k = lo; k < hi; k++) {
             uint32_t d[8];
             ouro::blake2b256_stream(d, raw + tx_off[k], tx_len[k]);
             digest_bytes(o.tx_id + 32 * k, d);
           }
         })))
      return rc;
    const WitnessHostRows<Out> h{n,    status,    nwit.data(), E::kBlockMagic ? bmagic.data() : nullptr,
                                 o,    (size_t)W, r.vk,        sig.data()};
    if ((rc = E::verify_host(h))) return rc;
    for (size_t i = 0; i < n; i++) {
      uint32_t bad = 0;
      if (status[i] == OURO_PACK_OK)
        for (uint64_t k = o.wit_begin[i]; k < o.wit_begin[i + 1]; k++) bad += o.wit_ok[k] ? 0 : 1;
      n_bad[i] = bad;
      verdict[i] = (status[i] == OURO_PACK_OK && bad == 0) ||
                           (E::kEbbOk && status[i] == OURO_PACK_EBB)
                       ? E::kAllOk
                       : 0;
    }
    return OURO_OK;
  }

  // ---- the host-buffer forms on the device ----
  // (the groups of whole blocks and their upload: host_util.h group_end, group_upload)
  static int count_dev(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                       uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
    hipStream_t st;
    int rc = thread_stream(&st);
    if (rc) return rc;
    const size_t budget = E::budget();
    for (size_t lo = 0; lo < n;) {
      const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
      Stager sg{st};
      GroupUp g;
      if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
      auto dst = sg.out<uint8_t>(m);
      auto da = sg.out<uint32_t>(m);
      auto db = sg.out<uint32_t>(m);
      if (sg.rc) return sg.rc;
      if ((rc = E::count(st, g.raw, g.w.span(), g.off, g.len, m, dst, da, db))) return rc;
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
  // group continue the earlier ones (tx_base / wit_base), and the capacities
  // are applied here, to the global rows: the caller's rows past the blocks
  // that fit are left untouched.
  static int on_device(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                       int64_t magic, const Out& o, uint8_t* status, uint8_t* verdict,
                       uint32_t* n_bad) {
    hipStream_t st;
    int rc = thread_stream(&st);
    if (rc) return rc;
    const size_t budget = E::budget();
    uint64_t tx_base = 0, wit_base = 0;
    for (size_t lo = 0; lo < n;) {
      const size_t hi = group_end(len, n, lo, budget), m = hi - lo;
      Stager sg{st};
      GroupUp g;
      if ((rc = group_upload(sg, st, raw, off + lo, len + lo, m, &g))) return rc;
      const size_t sums = kWitnessVals * scan_tiles(m);
      WitnessDev d{};
      d.ntx = sg.out<uint32_t>(m);
      d.nwit = sg.out<uint32_t>(m);
      d.sums = sg.out<uint64_t>(sums + scan_rows_words(kWitnessVals));
      if (E::kBlockMagic) d.magic = sg.out<uint64_t>(m);
      auto dst = sg.out<uint8_t>(m);
      d.tx_begin = sg.out<uint64_t>(m + 1);
      d.wit_begin = sg.out<uint64_t>(m + 1);
      if (sg.rc) return sg.rc;
      d.rows = d.sums + sums;
      d.tx_cap = d.wit_cap = ~(size_t)0;  // (no capacity yet: the row counts are the group's totals)
      if ((rc = count_scan(st, g.raw, g.w.span(), g.off, g.len, m, d, dst))) return rc;
      std::vector<uint64_t> tb(m + 1), wb(m + 1);
      if ((rc = download(st, tb.data(), d.tx_begin, 8 * (m + 1))) ||
          (rc = download(st, wb.data(), d.wit_begin, 8 * (m + 1))) || (rc = finish(st)))
        return rc;
      const size_t T = (size_t)tb[m], W = (size_t)wb[m];
      if (tx_base + T > 0xffffffffull) return fail(OURO_EINVAL, "more than 2^32 - 1 transactions");
      d.tx_cap = T;  // the group's rows, all of them
      d.wit_cap = W;
      d.tx_base = tx_base;
      d.tx_off = sg.out<uint64_t>(T);
      d.tx_len = sg.out<uint32_t>(T);
      d.vk = sg.out<uint8_t>(E::kKey * W);
      d.sig = sg.out<uint8_t>(64 * W);
      d.b2b = sg.out<uint8_t>(ouro::cbor::b2b_work_bytes(T));
      d.tx_id = sg.out<uint8_t>(32 * T);
      d.wit_tx = sg.out<uint32_t>(W);
      d.kind = sg.out<uint8_t>(W);
      d.wit_ok = sg.out<uint8_t>(W);
      auto dver = sg.out<uint8_t>(m);
      auto dbad = sg.out<uint32_t>(m);
      if (sg.rc) return sg.rc;
      if ((rc = rows(st, g.raw, g.w.span(), g.off, g.len, m, magic, d, dst, dver, dbad))) return rc;
      std::vector<uint8_t> ts(m), tv(m), tid(32 * T), tk(W), tok(W),
          tvk(o.wit_vk ? E::kKey * W : 0);
      std::vector<uint32_t> tbad(m), twt(W);
      if ((rc = download(st, ts.data(), dst, m)) || (rc = download(st, tv.data(), dver, m)) ||
          (rc = download(st, tbad.data(), dbad, 4 * m)) ||
          (rc = download(st, tid.data(), d.tx_id, 32 * T)) ||
          (rc = download(st, twt.data(), d.wit_tx, 4 * W)) ||
          (rc = download(st, tk.data(), d.kind, W)) || (rc = download(st, tok.data(), d.wit_ok, W)) ||
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
        if (o.wit_vk) memcpy(o.wit_vk + E::kKey * wit_base, tvk.data(), E::kKey * Wf);
      }
      tx_base += T;
      wit_base += W;
      lo = hi;
    }
    o.tx_begin[n] = tx_base;
    o.wit_begin[n] = wit_base;
    return OURO_OK;
  }

  // ---- the bodies of the C entries (host: the *_host form) ----
  static int verify_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                         const uint32_t* len, size_t n, int64_t magic, const Out* out,
                         uint8_t* status, uint8_t* verdict, uint32_t* n_bad, bool host) {
    if (int rc = out_check(out)) return rc;
    if (int rc = E::magic_check(magic)) return rc;
    if (n == 0) {
      out->tx_begin[0] = out->wit_begin[0] = 0;
      return OURO_OK;
    }
    if (!status || !verdict || !n_bad) return fail(OURO_EINVAL, "null argument");
    if (int rc = blocks_check(raw, raw_bytes, off, len, n)) return rc;
    auto recompute = [&] { return on_host(raw, off, len, n, magic, *out, status, verdict, n_bad); };
    return host ? recompute()
                : or_host(on_device(raw, off, len, n, magic, *out, status, verdict, n_bad),
                          recompute);
  }

  static int count_call(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                        const uint32_t* len, size_t n, int64_t magic, uint8_t* status,
                        uint32_t* ntx, uint32_t* nwit, bool host) {
    if (int rc = E::magic_check(magic)) return rc;
    if (n == 0) return OURO_OK;
    if (!status || !ntx || !nwit) return fail(OURO_EINVAL, "null argument");
    if (int rc = blocks_check(raw, raw_bytes, off, len, n)) return rc;
    auto recompute = [&] { return count_host(raw, off, len, n, status, ntx, nwit); };
    return host ? recompute()
                : or_host(count_dev(raw, off, len, n, status, ntx, nwit), recompute);
  }

  // device pointers, enqueued on `stream`: rows past the blocks that fit are zero
  static int device_call(void* stream, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                         const uint32_t* len, size_t n, int64_t magic, const Out* out, void* work,
                         size_t work_size, uint8_t* status, uint8_t* verdict, uint32_t* n_bad) {
    if (int rc = out_check(out)) return rc;
    if (int rc = E::magic_check(magic)) return rc;
    if (n == 0) return OURO_OK;
    if (!raw || !off || !len || !work || !status || !verdict || !n_bad)
      return fail(OURO_EINVAL, "null argument");
    if (work_size < work_bytes(n, out->tx_cap, out->wit_cap))
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
    WitnessDev d{};
    carve(ouro::cbor::arena_base(work), n, out->tx_cap, out->wit_cap, &d);
    if (out->wit_vk) d.vk = out->wit_vk;
    rows_of(*out, 0, &d);
    if (int rc = count_scan(st, raw, raw_bytes, off, len, n, d, status)) return rc;
    return rows(st, raw, raw_bytes, off, len, n, magic, d, status, verdict, n_bad);
  }
};

}  // namespace ouro_rt
#pragma GCC visibility pop
