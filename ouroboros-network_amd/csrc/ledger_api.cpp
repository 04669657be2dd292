// ledger_api.cpp -- the ledger-view header checks (include/ouro_verify.h
// OURO_LV_*; ledger_view.h): the argument checks, the views packed for the
// device, the host path, the OCERT counter fold and the C entries.  Host code
// only: the kernel is reached through launches.h (launch_ledger).
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "host_util.h"
#include "launch.h"
#include "launches.h"
#include "ledger_view.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

struct ouro_ledger_views_dev {
  int dev;
  void* block;
  ouro_ledger_views d;  // device pointers into block
  bool has_genesis;     // uploaded with a genesis-delegation schedule:
  ouro_genesis_delegs g;  // device pointers into the same block
};

namespace {
int cmp28(const uint8_t* a, const uint8_t* b) { return memcmp(a, b, 28); }

// the rows of a (checked) schedule packed as one block; *d: the same schedule
// with its pointers at `base` + the block's offsets.  gd (or null): a checked
// genesis-delegation schedule packed behind the views in the same block -- what
// the kernel reads of it: gen_begin, delegate_id, delegate_vrf; *dgd likewise
// (its genesis_id stays null: the order matters to the argument check alone)
size_t lv_pack(const ouro_ledger_views& v, const ouro_genesis_delegs* gd, std::vector<uint8_t>* blk,
               ouro_ledger_views* d, ouro_genesis_delegs* dgd, const uint8_t* base) {
  const size_t k = v.k, rows = v.pool_begin[k];
  const size_t o_fs = 0, o_dn = o_fs + a16(8 * k), o_dd = o_dn + a16(8 * k), o_pb = o_dd + a16(8 * k);
  const size_t o_sn = o_pb + a16(4 * (k + 1)), o_sd = o_sn + a16(8 * rows);
  const size_t o_vh = o_sd + a16(8 * rows), o_id = o_vh + a16(32 * rows);
  const size_t grows = gd ? gd->gen_begin[k] : 0;
  const size_t o_gb = o_id + a16(28 * rows) + 16, o_gi = o_gb + (gd ? a16(4 * (k + 1)) : 0);
  const size_t o_gv = o_gi + a16(28 * grows);
  const size_t total = gd ? o_gv + a16(32 * grows) + 16 : o_gb;
  if (blk) {
    blk->assign(total, 0);
    uint8_t* p = blk->data();
    memcpy(p + o_fs, v.first_slot, 8 * k);
    memcpy(p + o_dn, v.d_num, 8 * k);
    memcpy(p + o_dd, v.d_den, 8 * k);
    memcpy(p + o_pb, v.pool_begin, 4 * (k + 1));
    if (rows) {
      memcpy(p + o_sn, v.sigma_num, 8 * rows);
      memcpy(p + o_sd, v.sigma_den, 8 * rows);
      memcpy(p + o_vh, v.vrf_hash, 32 * rows);
      memcpy(p + o_id, v.pool_id, 28 * rows);
    }
    if (gd) memcpy(p + o_gb, gd->gen_begin, 4 * (k + 1));
    if (grows) {
      memcpy(p + o_gi, gd->delegate_id, 28 * grows);
      memcpy(p + o_gv, gd->delegate_vrf, 32 * grows);
    }
  }
  if (d) {
    d->k = k;
    d->first_slot = reinterpret_cast<const uint64_t*>(base + o_fs);
    d->d_num = reinterpret_cast<const uint64_t*>(base + o_dn);
    d->d_den = reinterpret_cast<const uint64_t*>(base + o_dd);
    d->pool_begin = reinterpret_cast<const uint32_t*>(base + o_pb);
    d->sigma_num = reinterpret_cast<const uint64_t*>(base + o_sn);
    d->sigma_den = reinterpret_cast<const uint64_t*>(base + o_sd);
    d->vrf_hash = base + o_vh;
    d->pool_id = base + o_id;
  }
  if (gd && dgd) {
    dgd->k = k;
    dgd->gen_begin = reinterpret_cast<const uint32_t*>(base + o_gb);
    dgd->genesis_id = nullptr;
    dgd->delegate_id = base + o_gi;
    dgd->delegate_vrf = base + o_gv;
    dgd->asc_inv = gd->asc_inv;
  }
  return total;
}

struct RowArgs {
  size_t n;
  const uint8_t *issuer_vk, *vrf_vk;
  const uint64_t* slot;
  const uint8_t* leader_output;
  const uint64_t *c0, *counter;
};

int rows_check(const RowArgs& r, const uint8_t* ledger, bool need_counter) {
  if (!r.issuer_vk || !r.vrf_vk || !r.slot || !r.leader_output || !r.c0 || !ledger)
    return fail(OURO_EINVAL, "null argument");
  if (need_counter && !r.counter) return fail(OURO_EINVAL, "null ocert_counter beside counters");
  return OURO_OK;
}

int lv_dev(const RowArgs& r, const ouro_ledger_views& v, const ouro_ledger_globals& g,
           const ouro_genesis_delegs* gd, uint8_t* ledger, uint32_t* pool_row) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  std::vector<uint8_t> blk;
  lv_pack(v, gd, &blk, nullptr, nullptr, nullptr);
  Stager sg{st};
  const uint8_t* dblk = sg.up(blk.data(), blk.size());
  auto dis = sg.up(r.issuer_vk, 32 * r.n);
  auto dvk = sg.up(r.vrf_vk, 32 * r.n);
  auto dsl = sg.up(r.slot, r.n);
  auto dlo = sg.up(r.leader_output, 64 * r.n);
  auto dc0 = sg.up(r.c0, r.n);
  auto dl = sg.out<uint8_t>(r.n);
  auto dr = sg.out<uint32_t>(r.n);
  if (sg.rc) return sg.rc;
  ouro_ledger_views d;
  ouro_genesis_delegs dgd{};
  lv_pack(v, gd, nullptr, &d, &dgd, dblk);
  if ((rc = lv_launch(st, r.n, dis, dvk, dsl, dlo, dc0, d, g, gd ? &dgd : nullptr, dl, dr)))
    return rc;
  std::vector<uint8_t> tl(r.n);
  std::vector<uint32_t> tr(r.n);
  if ((rc = download(st, tl.data(), dl, r.n))) return rc;
  if ((rc = download(st, tr.data(), dr, 4 * r.n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(ledger, tl.data(), r.n);
  memcpy(pool_row, tr.data(), 4 * r.n);
  return OURO_OK;
}

int rows_call(const RowArgs& r, const ouro_ledger_views* v, const ouro_genesis_delegs* gd,
              const ouro_ledger_globals* g, const ouro_ocert_counters* t, uint64_t* counter_out,
              uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row, bool host) {
  int rc;
  if ((rc = lv_views_check(v)) || (rc = lv_globals_check(g)) ||
      (gd && (rc = lv_genesis_check(gd, *v))) ||
      (rc = lv_counters_check(t, counter_out, present_out)))
    return rc;
  std::vector<uint32_t> map, gmap, rows;
  if (t && (rc = lv_fold_map(*v, *t, &map))) return rc;
  if (t && gd && (rc = lv_fold_gmap(*gd, *t, &gmap))) return rc;
  if (r.n) {
    if ((rc = rows_check(r, ledger, t != nullptr))) return rc;
    if (!pool_row) {
      rows.resize(r.n);
      pool_row = rows.data();
    }
    auto on_host = [&] {
      return lv_host_rows(r.n, r.issuer_vk, r.vrf_vk, r.slot, r.leader_output, r.c0, *v, *g, gd,
                          ledger, pool_row);
    };
    rc = host ? on_host() : or_host(lv_dev(r, *v, *g, gd, ledger, pool_row), on_host);
    if (rc) return rc;
  }
  if (t) {
    LvFold f;
    lv_fold_begin(&f, *t, &map, gd ? &gmap : nullptr, counter_out, present_out);
    lv_fold_run(&f, r.n, pool_row, r.counter, ledger);
  }
  return OURO_OK;
}
}  // namespace

namespace ouro_rt {

// everything that is OURO_EINVAL in a schedule, before anything runs
int lv_views_check(const ouro_ledger_views* v) {
  if (!v) return fail(OURO_EINVAL, "null ledger views");
  if (v->k < 1 || v->k > OURO_EPOCHS_MAX)
    return fail(OURO_EINVAL, "ledger views: k outside 1 .. OURO_EPOCHS_MAX");
  if (!v->first_slot || !v->d_num || !v->d_den || !v->pool_begin)
    return fail(OURO_EINVAL, "ledger views: null array");
  if (v->first_slot[0] != 0) return fail(OURO_EINVAL, "ledger views: first_slot[0] must be 0");
  if (v->pool_begin[0] != 0) return fail(OURO_EINVAL, "ledger views: pool_begin[0] must be 0");
  for (size_t j = 0; j < v->k; j++) {
    const std::string at = "ledger views: entry " + std::to_string(j);
    if (j && v->first_slot[j] <= v->first_slot[j - 1])
      return fail(OURO_EINVAL, at + ": first_slot not strictly increasing");
    if (v->pool_begin[j + 1] < v->pool_begin[j])
      return fail(OURO_EINVAL, at + ": pool_begin decreasing");
    if (v->pool_begin[j + 1] > OURO_LV_ROWS_MAX)
      return fail(OURO_EINVAL, at + ": more than OURO_LV_ROWS_MAX rows");
    if (v->d_den[j] == 0 || v->d_num[j] > v->d_den[j])
      return fail(OURO_EINVAL, at + ": d outside [0, 1]");
  }
  const size_t rows = v->pool_begin[v->k];
  if (rows && (!v->pool_id || !v->vrf_hash || !v->sigma_num || !v->sigma_den))
    return fail(OURO_EINVAL, "ledger views: null pool array");
  for (size_t j = 0; j < v->k; j++)
    for (size_t r = v->pool_begin[j]; r < v->pool_begin[j + 1]; r++) {
      if (v->sigma_den[r] == 0 || v->sigma_num[r] > v->sigma_den[r])
        return fail(OURO_EINVAL, "ledger views: row " + std::to_string(r) + ": sigma outside [0, 1]");
      if (r > v->pool_begin[j] && cmp28(v->pool_id + 28 * (r - 1), v->pool_id + 28 * r) >= 0)
        return fail(OURO_EINVAL,
                    "ledger views: row " + std::to_string(r) + ": pool ids not strictly ascending");
    }
  return OURO_OK;
}

int lv_globals_check(const ouro_ledger_globals* g) {
  if (!g) return fail(OURO_EINVAL, "null ledger globals");
  if (g->slots_per_kes_period == 0) return fail(OURO_EINVAL, "zero slots per KES period");
  return OURO_OK;
}

// everything that is OURO_EINVAL in a genesis-delegation schedule beside its
// (checked) views, the counters table's rows excepted (lv_fold_gmap)
int lv_genesis_check(const ouro_genesis_delegs* gd, const ouro_ledger_views& v) {
  if (!gd) return fail(OURO_EINVAL, "null genesis delegations");
  if (gd->k != v.k) return fail(OURO_EINVAL, "genesis delegations: k differs from the views'");
  if (gd->asc_inv == 0) return fail(OURO_EINVAL, "genesis delegations: asc_inv must be >= 1");
  if (!gd->gen_begin) return fail(OURO_EINVAL, "genesis delegations: null array");
  if (gd->gen_begin[0] != 0) return fail(OURO_EINVAL, "genesis delegations: gen_begin[0] must be 0");
  for (size_t j = 0; j < gd->k; j++) {
    const std::string at = "genesis delegations: entry " + std::to_string(j);
    if (gd->gen_begin[j + 1] < gd->gen_begin[j]) return fail(OURO_EINVAL, at + ": gen_begin decreasing");
    if (gd->gen_begin[j + 1] > OURO_LV_GEN_ROWS_MAX)
      return fail(OURO_EINVAL, at + ": more than OURO_LV_GEN_ROWS_MAX rows");
    if (v.d_num[j] > 0 && gd->gen_begin[j + 1] == gd->gen_begin[j])
      return fail(OURO_EINVAL, at + ": d > 0 and no genesis keys");
  }
  const size_t rows = gd->gen_begin[gd->k];
  if (rows && (!gd->genesis_id || !gd->delegate_id || !gd->delegate_vrf))
    return fail(OURO_EINVAL, "genesis delegations: null row array");
  for (size_t j = 0; j < gd->k; j++)
    for (size_t r = gd->gen_begin[j] + (size_t)1; r < gd->gen_begin[j + 1]; r++)
      if (cmp28(gd->genesis_id + 28 * (r - 1), gd->genesis_id + 28 * r) >= 0)
        return fail(OURO_EINVAL, "genesis delegations: row " + std::to_string(r) +
                                     ": genesis ids not strictly ascending");
  return OURO_OK;
}

// a counters table and its outputs (t may be null: no fold)
int lv_counters_check(const ouro_ocert_counters* t, const uint64_t* counter_out,
                      const uint8_t* present_out) {
  if (!t) return OURO_OK;
  if (!counter_out || !present_out) return fail(OURO_EINVAL, "null counter_out or present_out");
  if (t->m && (!t->pool_id || !t->counter || !t->present))
    return fail(OURO_EINVAL, "counters: null array");
  for (size_t i = 1; i < t->m; i++)
    if (cmp28(t->pool_id + 28 * (i - 1), t->pool_id + 28 * i) >= 0)
      return fail(OURO_EINVAL, "counters: pool ids not strictly ascending at " + std::to_string(i));
  return OURO_OK;
}

// the host path: ledger_check_lane over the rows on the worker pool
int lv_host_rows(size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk, const uint64_t* slot,
                 const uint8_t* leader_output, const uint64_t* c0, const ouro_ledger_views& v,
                 const ouro_ledger_globals& g, const ouro_genesis_delegs* gd, uint8_t* ledger,
                 uint32_t* pool_row) {
  return host_rows(n, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      ledger[i] = gd ? lv::ledger_check_lane<true>(v, g, *gd, issuer_vk + 32 * i, vrf_vk + 32 * i,
                                                   slot[i], leader_output + 64 * i, c0[i],
                                                   &pool_row[i])
                     : lv::ledger_check_lane(v, g, issuer_vk + 32 * i, vrf_vk + 32 * i, slot[i],
                                             leader_output + 64 * i, c0[i], &pool_row[i]);
  });
}

// a checked schedule (and genesis-delegation schedule, or null) packed and
// uploaded as one block on `st` (not synchronised; *host must stay alive until
// the copy has completed)
int lv_upload(hipStream_t st, const ouro_ledger_views& v, const ouro_genesis_delegs* gd, Buf* buf,
              std::vector<uint8_t>* host, ouro_ledger_views* d, ouro_genesis_delegs* dgd) {
  lv_pack(v, gd, host, nullptr, nullptr, nullptr);
  if (int rc = ensure(*buf, host->size())) return rc;
  OURO_HIP(hipMemcpyAsync(buf->p, host->data(), host->size(), hipMemcpyHostToDevice, st));
  lv_pack(v, gd, nullptr, d, dgd, static_cast<const uint8_t*>(buf->p));
  return OURO_OK;
}

// k_ledger_checks, or with a schedule k_ledger_checks_overlay
int lv_launch(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
              const uint64_t* slot, const uint8_t* leader_output, const uint64_t* ocert_kes_period,
              const ouro_ledger_views& v, const ouro_ledger_globals& g,
              const ouro_genesis_delegs* gd, uint8_t* ledger, uint32_t* pool_row) {
  return gd ? launch_ledger_overlay(st, n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period,
                                    v, g, *gd, ledger, pool_row)
            : launch_ledger(st, n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, v, g,
                            ledger, pool_row);
}

// map[r] = the table index of view row r: each entry's sorted rows merged
// with the sorted table; a row whose id the table lacks is OURO_EINVAL
int lv_fold_map(const ouro_ledger_views& v, const ouro_ocert_counters& t,
                std::vector<uint32_t>* map) {
  map->assign(v.pool_begin[v.k], 0);
  for (size_t j = 0; j < v.k; j++) {
    size_t q = 0;
    for (size_t r = v.pool_begin[j]; r < v.pool_begin[j + 1]; r++) {
      const uint8_t* id = v.pool_id + 28 * r;
      while (q < t.m && cmp28(t.pool_id + 28 * q, id) < 0) q++;
      if (q == t.m || cmp28(t.pool_id + 28 * q, id) != 0)
        return fail(OURO_EINVAL, "counters: no row for the pool id of view row " + std::to_string(r));
      (*map)[r] = (uint32_t)q;
    }
  }
  return OURO_OK;
}

// gmap[r] = the table index of genesis row r's delegate_id.  The delegates of
// an entry are in their genesis keys' order, so each entry's rows are sorted by
// delegate id first and then merged with the sorted table like the pools'.
int lv_fold_gmap(const ouro_genesis_delegs& gd, const ouro_ocert_counters& t,
                 std::vector<uint32_t>* gmap) {
  gmap->assign(gd.gen_begin[gd.k], 0);
  std::vector<uint32_t> order;
  for (size_t j = 0; j < gd.k; j++) {
    order.clear();
    for (uint32_t r = gd.gen_begin[j]; r < gd.gen_begin[j + 1]; r++) order.push_back(r);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return cmp28(gd.delegate_id + 28 * (size_t)a, gd.delegate_id + 28 * (size_t)b) < 0;
    });
    size_t q = 0;
    for (const uint32_t r : order) {
      const uint8_t* id = gd.delegate_id + 28 * (size_t)r;
      while (q < t.m && cmp28(t.pool_id + 28 * q, id) < 0) q++;
      if (q == t.m || cmp28(t.pool_id + 28 * q, id) != 0)
        return fail(OURO_EINVAL,
                    "counters: no row for the delegate id of genesis row " + std::to_string(r));
      (*gmap)[r] = (uint32_t)q;
    }
  }
  return OURO_OK;
}

void lv_fold_begin(LvFold* f, const ouro_ocert_counters& t, const std::vector<uint32_t>* map,
                   const std::vector<uint32_t>* gmap, uint64_t* counter_out, uint8_t* present_out) {
  f->map = map;
  f->gmap = gmap;
  f->counter = counter_out;
  f->present = present_out;
  if (t.m && counter_out != t.counter) memmove(counter_out, t.counter, 8 * t.m);
  if (t.m && present_out != t.present) memmove(present_out, t.present, t.m);
}

void lv_fold_run(LvFold* f, size_t n, const uint32_t* pool_row, const uint64_t* counter,
                 uint8_t* ledger) {
  for (size_t i = 0; i < n; i++) {
    if (!(ledger[i] & OURO_LV_POOL_KNOWN)) continue;
    // an overlay row's row is a genesis row: its key is the delegate's id
    const std::vector<uint32_t>* m = (ledger[i] & OURO_LV_OVERLAY) ? f->gmap : f->map;
    if (!m || pool_row[i] >= m->size()) continue;  // (never with POOL_KNOWN from the rule)
    const uint32_t q = (*m)[pool_row[i]];
    const uint64_t m0 = f->present[q] ? f->counter[q] : 0;  // currentIssueNo
    if (m0 <= counter[i]) ledger[i] |= OURO_LV_COUNTER_OK;
    else ledger[i] &= (uint8_t)~OURO_LV_COUNTER_OK;
    f->counter[q] = counter[i];
    f->present[q] = 1;
  }
}

}  // namespace ouro_rt

extern "C" {

// ledger-specs OCERT rule, CounterTooSmallOCERT: the counter never goes back
// per pool, in stream order
int ouro_ocert_counter_fold_overlay(size_t n, const uint32_t* pool_row,
                                    const uint64_t* ocert_counter, const ouro_ledger_views* views,
                                    const ouro_genesis_delegs* genesis,
                                    const ouro_ocert_counters* in, uint64_t* counter_out,
                                    uint8_t* present_out, uint8_t* ledger) {
  int rc;
  if (!in) return fail(OURO_EINVAL, "null counters");
  if ((rc = lv_views_check(views)) || (genesis && (rc = lv_genesis_check(genesis, *views))) ||
      (rc = lv_counters_check(in, counter_out, present_out)))
    return rc;
  if (n && (!pool_row || !ocert_counter || !ledger)) return fail(OURO_EINVAL, "null argument");
  std::vector<uint32_t> map, gmap;
  if ((rc = lv_fold_map(*views, *in, &map))) return rc;
  if (genesis && (rc = lv_fold_gmap(*genesis, *in, &gmap))) return rc;
  LvFold f;
  lv_fold_begin(&f, *in, &map, genesis ? &gmap : nullptr, counter_out, present_out);
  lv_fold_run(&f, n, pool_row, ocert_counter, ledger);
  return OURO_OK;
}

int ouro_ocert_counter_fold(size_t n, const uint32_t* pool_row, const uint64_t* ocert_counter,
                            const ouro_ledger_views* views, const ouro_ocert_counters* in,
                            uint64_t* counter_out, uint8_t* present_out, uint8_t* ledger) {
  return ouro_ocert_counter_fold_overlay(n, pool_row, ocert_counter, views, nullptr, in, counter_out,
                                         present_out, ledger);
}

// ledger-specs OVERLAY (vrfChecks: VRFKeyUnknown, VRFKeyWrongVRFKey,
// VRFLeaderValueTooBig) and OCERT (KESBeforeStartOCERT, KESAfterEndOCERT,
// CounterTooSmallOCERT) per sliced header row
int ouro_tpraos_ledger_checks(size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                              const uint64_t* slot, const uint8_t* leader_output,
                              const uint64_t* ocert_kes_period, const uint64_t* ocert_counter,
                              const ouro_ledger_views* views, const ouro_ledger_globals* globals,
                              const ouro_ocert_counters* counters, uint64_t* counter_out,
                              uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row) {
  const RowArgs r{n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, ocert_counter};
  return rows_call(r, views, nullptr, globals, counters, counter_out, present_out, ledger, pool_row,
                   false);
}

int ouro_tpraos_ledger_checks_host(size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                                   const uint64_t* slot, const uint8_t* leader_output,
                                   const uint64_t* ocert_kes_period, const uint64_t* ocert_counter,
                                   const ouro_ledger_views* views,
                                   const ouro_ledger_globals* globals,
                                   const ouro_ocert_counters* counters, uint64_t* counter_out,
                                   uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row) {
  const RowArgs r{n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, ocert_counter};
  return rows_call(r, views, nullptr, globals, counters, counter_out, present_out, ledger, pool_row,
                   true);
}

// the same with the OVERLAY rule's genesis-delegate branch (lookupInOverlay
// Schedule; pbftVrfChecks: NotActiveSlotOVERLAY, WrongGenesisColdKeyOVERLAY,
// WrongGenesisVRFKeyOVERLAY) on overlay slots
int ouro_tpraos_ledger_checks_overlay(size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                                      const uint64_t* slot, const uint8_t* leader_output,
                                      const uint64_t* ocert_kes_period,
                                      const uint64_t* ocert_counter, const ouro_ledger_views* views,
                                      const ouro_genesis_delegs* genesis,
                                      const ouro_ledger_globals* globals,
                                      const ouro_ocert_counters* counters, uint64_t* counter_out,
                                      uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row) {
  const RowArgs r{n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, ocert_counter};
  return rows_call(r, views, genesis, globals, counters, counter_out, present_out, ledger, pool_row,
                   false);
}

int ouro_tpraos_ledger_checks_overlay_host(size_t n, const uint8_t* issuer_vk,
                                           const uint8_t* vrf_vk, const uint64_t* slot,
                                           const uint8_t* leader_output,
                                           const uint64_t* ocert_kes_period,
                                           const uint64_t* ocert_counter,
                                           const ouro_ledger_views* views,
                                           const ouro_genesis_delegs* genesis,
                                           const ouro_ledger_globals* globals,
                                           const ouro_ocert_counters* counters,
                                           uint64_t* counter_out, uint8_t* present_out,
                                           uint8_t* ledger, uint32_t* pool_row) {
  const RowArgs r{n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, ocert_counter};
  return rows_call(r, views, genesis, globals, counters, counter_out, present_out, ledger, pool_row,
                   true);
}

int ouro_ledger_views_upload_overlay(const ouro_ledger_views* views,
                                     const ouro_genesis_delegs* genesis,
                                     ouro_ledger_views_dev** out) {
  if (!out) return fail(OURO_EINVAL, "null out");
  *out = nullptr;
  if (int rc = lv_views_check(views)) return rc;
  if (genesis)
    if (int rc = lv_genesis_check(genesis, *views)) return rc;
  DeviceState* ds;
  int dev, rc = device_state(&ds);
  if (rc || (rc = current_device(&dev))) return rc;
  std::vector<uint8_t> blk;
  const size_t bytes = lv_pack(*views, genesis, &blk, nullptr, nullptr, nullptr);
  ouro_ledger_views_dev* dv =
      new (std::nothrow) ouro_ledger_views_dev{dev, nullptr, {}, genesis != nullptr, {}};
  if (!dv) return fail(OURO_EDEVICE, "out of host memory");
  if (hipMalloc(&dv->block, bytes) != hipSuccess ||
      hipMemcpy(dv->block, blk.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (dv->block) (void)hipFree(dv->block);
    delete dv;
    return fail(OURO_EDEVICE, "ledger views: upload failed");
  }
  lv_pack(*views, genesis, nullptr, &dv->d, &dv->g, static_cast<const uint8_t*>(dv->block));
  *out = dv;
  return OURO_OK;
}

int ouro_ledger_views_upload(const ouro_ledger_views* views, ouro_ledger_views_dev** out) {
  return ouro_ledger_views_upload_overlay(views, nullptr, out);
}

void ouro_ledger_views_free(ouro_ledger_views_dev* dv) {
  if (!dv) return;
  (void)hipFree(dv->block);
  delete dv;
}

int ouro_tpraos_ledger_checks_device(void* stream, size_t n, const uint8_t* issuer_vk,
                                     const uint8_t* vrf_vk, const uint64_t* slot,
                                     const uint8_t* leader_output, const uint64_t* ocert_kes_period,
                                     const ouro_ledger_views_dev* views,
                                     const ouro_ledger_globals* globals, uint8_t* ledger,
                                     uint32_t* pool_row) {
  if (!views) return fail(OURO_EINVAL, "null ledger views");
  if (int rc = lv_globals_check(globals)) return rc;
  if (n == 0) return OURO_OK;
  const RowArgs r{n, issuer_vk, vrf_vk, slot, leader_output, ocert_kes_period, nullptr};
  if (int rc = rows_check(r, ledger, false)) return rc;
  if (!pool_row) return fail(OURO_EINVAL, "null pool_row");
  if (misaligned(issuer_vk, 4) || misaligned(vrf_vk, 4) || misaligned(pool_row, 4))
    return fail(OURO_EINVAL, "issuer_vk, vrf_vk and pool_row must be 4-byte aligned");
  if (misaligned(slot, 8) || misaligned(ocert_kes_period, 8))
    return fail(OURO_EINVAL, "slot and ocert_kes_period must be 8-byte aligned");
  DeviceState* ds;
  int dev, rc = device_state(&ds);
  if (rc || (rc = current_device(&dev))) return rc;
  if (dev != views->dev) return fail(OURO_EINVAL, "ledger views were uploaded to another device");
  return lv_launch(static_cast<hipStream_t>(stream), n, issuer_vk, vrf_vk, slot, leader_output,
                   ocert_kes_period, views->d, *globals, views->has_genesis ? &views->g : nullptr,
                   ledger, pool_row);
}

}  // extern "C"
