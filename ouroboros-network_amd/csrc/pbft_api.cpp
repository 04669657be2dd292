// pbft_api.cpp -- the Byron ledger-view checks (include/ouro_verify.h
// OURO_PBFT_*; pbft_view.h): the argument checks, the schedule packed for the
// device, the host path, the signing-window fold and the C entries.  Host code
// only: the kernels are reached through launches.h (launch_pbft,
// launch_byron_key_hash).
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <array>
#include <cstring>
#include <deque>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "host_util.h"
#include "launch.h"
#include "launches.h"
#include "pbft_view.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

struct ouro_pbft_views_dev {
  int dev;
  void* block;
  ouro_pbft_views d;  // device pointers into block (genesis_id stays null: the fold's)
};

namespace {
int cmp28(const uint8_t* a, const uint8_t* b) { return memcmp(a, b, 28); }
using Id = std::array<uint8_t, 28>;
Id id_at(const uint8_t* p) {
  Id x;
  memcpy(x.data(), p, 28);
  return x;
}

// everything that is OURO_EINVAL in a delegation schedule, before anything runs
int views_check(const ouro_pbft_views* v) {
  if (!v) return fail(OURO_EINVAL, "null pbft views");
  if (v->k < 1 || v->k > OURO_EPOCHS_MAX)
    return fail(OURO_EINVAL, "pbft views: k outside 1 .. OURO_EPOCHS_MAX");
  if (v->window == 0) return fail(OURO_EINVAL, "pbft views: window must be >= 1");
  if (!v->first_slot || !v->dlg_begin) return fail(OURO_EINVAL, "pbft views: null array");
  if (v->first_slot[0] != 0) return fail(OURO_EINVAL, "pbft views: first_slot[0] must be 0");
  if (v->dlg_begin[0] != 0) return fail(OURO_EINVAL, "pbft views: dlg_begin[0] must be 0");
  for (size_t j = 0; j < v->k; j++) {
    const std::string at = "pbft views: entry " + std::to_string(j);
    if (j && v->first_slot[j] <= v->first_slot[j - 1])
      return fail(OURO_EINVAL, at + ": first_slot not strictly increasing");
    if (v->dlg_begin[j + 1] < v->dlg_begin[j]) return fail(OURO_EINVAL, at + ": dlg_begin decreasing");
    if (v->dlg_begin[j + 1] > OURO_LV_GEN_ROWS_MAX)
      return fail(OURO_EINVAL, at + ": more than OURO_LV_GEN_ROWS_MAX rows");
  }
  const size_t rows = v->dlg_begin[v->k];
  if (rows && (!v->delegate_id || !v->genesis_id))
    return fail(OURO_EINVAL, "pbft views: null row array");
  std::vector<const uint8_t*> gen;
  for (size_t j = 0; j < v->k; j++) {
    const size_t b = v->dlg_begin[j], e = v->dlg_begin[j + 1];
    for (size_t r = b + 1; r < e; r++)
      if (cmp28(v->delegate_id + 28 * (r - 1), v->delegate_id + 28 * r) >= 0)
        return fail(OURO_EINVAL,
                    "pbft views: row " + std::to_string(r) + ": delegate ids not strictly ascending");
    gen.clear();
    for (size_t r = b; r < e; r++) gen.push_back(v->genesis_id + 28 * r);
    std::sort(gen.begin(), gen.end(), [](const uint8_t* x, const uint8_t* y) { return cmp28(x, y) < 0; });
    for (size_t r = 1; r < gen.size(); r++)
      if (cmp28(gen[r - 1], gen[r]) == 0)
        return fail(OURO_EINVAL, "pbft views: entry " + std::to_string(j) + ": a genesis id twice");
  }
  return OURO_OK;
}

// a state and its outputs beside (checked) views; st may be null: genesis
int state_check(const ouro_pbft_state* st, const ouro_pbft_views& v, const uint8_t* id_out,
                const uint64_t* slot_out, const size_t* n_out) {
  if (!id_out || !slot_out || !n_out)
    return fail(OURO_EINVAL, "null signer_id_out, signer_slot_out or n_out");
  if (!st) return OURO_OK;
  if (st->n > v.window) return fail(OURO_EINVAL, "pbft state: more signers than the window holds");
  if (st->n && (!st->signer_id || !st->signer_slot))
    return fail(OURO_EINVAL, "pbft state: null array");
  return OURO_OK;
}

// what the kernel reads of a (checked) schedule packed as one block; *d: the
// same schedule with its pointers at `base` + the block's offsets
size_t views_pack(const ouro_pbft_views& v, std::vector<uint8_t>* blk, ouro_pbft_views* d,
                  const uint8_t* base) {
  const size_t k = v.k, rows = v.dlg_begin[k];
  const size_t o_fs = 0, o_db = o_fs + a16(8 * k), o_id = o_db + a16(4 * (k + 1));
  const size_t total = o_id + a16(28 * rows) + 16;
  if (blk) {
    blk->assign(total, 0);
    uint8_t* p = blk->data();
    memcpy(p + o_fs, v.first_slot, 8 * k);
    memcpy(p + o_db, v.dlg_begin, 4 * (k + 1));
    if (rows) memcpy(p + o_id, v.delegate_id, 28 * rows);
  }
  if (d) {
    *d = v;
    d->first_slot = reinterpret_cast<const uint64_t*>(base + o_fs);
    d->dlg_begin = reinterpret_cast<const uint32_t*>(base + o_db);
    d->delegate_id = base + o_id;
    d->genesis_id = nullptr;
  }
  return total;
}

// the host path: pbft_check_lane over the rows on the worker pool
int host_checks(size_t n, const uint8_t* delegate_vk, const uint64_t* slot, const uint8_t* status,
                const ouro_pbft_views& v, uint8_t* pbft, uint32_t* genesis_row) {
  return host_rows(n, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      pbft[i] = pbft::pbft_check_lane(v, delegate_vk + 64 * i, slot[i], status[i], &genesis_row[i]);
  });
}

int dev_checks(size_t n, const uint8_t* delegate_vk, const uint64_t* slot, const uint8_t* status,
               const ouro_pbft_views& v, uint8_t* pbft, uint32_t* genesis_row) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  std::vector<uint8_t> blk;
  views_pack(v, &blk, nullptr, nullptr);
  Stager sg{st};
  const uint8_t* dblk = sg.up(blk.data(), blk.size());
  auto dvk = sg.up(delegate_vk, 64 * n);
  auto dsl = sg.up(slot, n);
  auto dst = sg.up(status, n);
  auto dp = sg.out<uint8_t>(n);
  auto dr = sg.out<uint32_t>(n);
  if (sg.rc) return sg.rc;
  ouro_pbft_views d;
  views_pack(v, nullptr, &d, dblk);
  if ((rc = launch_pbft(st, n, dvk, dsl, dst, d, dp, dr))) return rc;
  std::vector<uint8_t> tp(n);
  std::vector<uint32_t> tr(n);
  if ((rc = download(st, tp.data(), dp, n))) return rc;
  if ((rc = download(st, tr.data(), dr, 4 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(pbft, tp.data(), n);
  memcpy(genesis_row, tr.data(), 4 * n);
  return OURO_OK;
}

int host_key_hash(size_t n, const uint8_t* xpub, uint8_t* out) {
  return host_rows(n, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) pbft::key_hash_lane(out + 28 * i, xpub + 64 * i);
  });
}

int dev_key_hash(size_t n, const uint8_t* xpub, uint8_t* out) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Stager sg{st};
  auto dx = sg.up(xpub, 64 * n);
  auto dout = sg.out<uint8_t>(28 * n);
  if (sg.rc) return sg.rc;
  if ((rc = launch_byron_key_hash(st, n, dx, dout))) return rc;
  std::vector<uint8_t> t(28 * n);
  if ((rc = download(st, t.data(), dout, 28 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(out, t.data(), 28 * n);
  return OURO_OK;
}

}  // namespace

namespace ouro_rt {
// The signing window (PBFT/State.hs PBftState): the signers oldest first and
// the count per genesis id.  Ids are interned once per call -- every genesis id
// of the schedule (row_key: schedule row -> key) and every id of the incoming
// state, known to an entry or not -- so a folded row is one ring step and two
// counter updates, no id compared.  begin() copies the incoming state, so the
// outputs may alias it; run() is one append per folded row; end() writes the
// window out.
struct PbftFold {
  uint64_t window = 1, threshold = 0;
  std::map<Id, uint32_t> key_of;
  std::vector<Id> ids;            // key -> id
  std::vector<uint64_t> counts;   // key -> signatures in the window
  std::vector<uint32_t> row_key;  // schedule row -> key
  std::deque<std::pair<uint64_t, uint32_t>> in_window;  // (slot, key)

  uint32_t intern(const uint8_t* p) {
    const Id x = id_at(p);
    const auto it = key_of.find(x);
    if (it != key_of.end()) return it->second;
    const uint32_t key = (uint32_t)ids.size();
    key_of.emplace(x, key);
    ids.push_back(x);
    counts.push_back(0);
    return key;
  }
  void begin(const ouro_pbft_views& v, const ouro_pbft_state* st) {
    window = v.window;
    threshold = v.threshold;
    key_of.clear();
    ids.clear();
    counts.clear();
    in_window.clear();
    const size_t rows = v.dlg_begin[v.k];
    row_key.resize(rows);
    for (size_t r = 0; r < rows; r++) row_key[r] = intern(v.genesis_id + 28 * r);
    for (size_t i = 0; st && i < st->n; i++) {
      const uint32_t key = intern(st->signer_id + 28 * i);
      in_window.emplace_back(st->signer_slot[i], key);
      counts[key]++;
    }
  }
  void run(size_t n, const uint32_t* genesis_row, const uint64_t* slot, uint8_t* pbft,
           uint64_t* signed_count) {
    for (size_t i = 0; i < n; i++) {
      if (signed_count) signed_count[i] = 0;
      if (!(pbft[i] & OURO_PBFT_DELEGATE_KNOWN) || (pbft[i] & OURO_PBFT_BOUNDARY)) continue;
      uint32_t bits = pbft[i] & ~(OURO_PBFT_SLOT_OK | OURO_PBFT_WINDOW_OK);
      if (genesis_row[i] >= row_key.size()) {  // (never from the rule: a caller's own row)
        pbft[i] = (uint8_t)bits;  // no signer to append: both bits clear, the window as it was
        continue;
      }
      // lastSignedSlot: Origin for the empty window
      if (in_window.empty() || slot[i] >= in_window.back().first) bits |= OURO_PBFT_SLOT_OK;
      // append: to the right, then the oldest off the left if the window was full
      const bool full = in_window.size() == window;
      const uint32_t gk = row_key[genesis_row[i]];
      in_window.emplace_back(slot[i], gk);
      counts[gk]++;
      if (full) {
        counts[in_window.front().second]--;
        in_window.pop_front();
      }
      const uint64_t c = counts[gk];  // countSignedBy
      if (signed_count) signed_count[i] = c;
      if (c <= threshold) bits |= OURO_PBFT_WINDOW_OK;
      pbft[i] = (uint8_t)bits;
    }
  }
  void end(uint8_t* id_out, uint64_t* slot_out, size_t* n_out) const {
    size_t i = 0;
    for (const auto& s : in_window) {
      slot_out[i] = s.first;
      memcpy(id_out + 28 * i, ids[s.second].data(), 28);
      i++;
    }
    *n_out = i;
  }
};

}  // namespace ouro_rt

namespace {
using Fold = ouro_rt::PbftFold;

int checks_call(size_t n, const uint8_t* delegate_vk, const uint64_t* slot, const uint8_t* status,
                const ouro_pbft_views* v, const ouro_pbft_state* st, uint8_t* id_out,
                uint64_t* slot_out, size_t* n_out, uint8_t* pbft, uint32_t* genesis_row,
                uint64_t* signed_count, bool host) {
  int rc;
  if ((rc = views_check(v)) || (st && (rc = state_check(st, *v, id_out, slot_out, n_out))))
    return rc;
  std::vector<uint32_t> rows;
  if (n) {
    if (!delegate_vk || !slot || !status || !pbft) return fail(OURO_EINVAL, "null argument");
    if (!genesis_row) {
      rows.resize(n);
      genesis_row = rows.data();
    }
    auto on_host = [&] { return host_checks(n, delegate_vk, slot, status, *v, pbft, genesis_row); };
    rc = host ? on_host()
              : or_host(dev_checks(n, delegate_vk, slot, status, *v, pbft, genesis_row), on_host);
    if (rc) return rc;
  }
  if (st) {
    Fold f;
    f.begin(*v, st);
    f.run(n, genesis_row, slot, pbft, signed_count);
    f.end(id_out, slot_out, n_out);
  } else if (signed_count) {
    for (size_t i = 0; i < n; i++) signed_count[i] = 0;
  }
  return OURO_OK;
}
}  // namespace

namespace ouro_rt {
PbftFold* pbft_fold_new() { return new (std::nothrow) PbftFold; }
void pbft_fold_free(PbftFold* f) { delete f; }
void pbft_fold_begin(PbftFold* f, const ouro_pbft_views& v, const ouro_pbft_state* st) {
  f->begin(v, st);
}
void pbft_fold_run(PbftFold* f, size_t n, const uint32_t* genesis_row, const uint64_t* slot,
                   uint8_t* pbft, uint64_t* signed_count) {
  f->run(n, genesis_row, slot, pbft, signed_count);
}
void pbft_fold_end(const PbftFold* f, uint8_t* id_out, uint64_t* slot_out, size_t* n_out) {
  f->end(id_out, slot_out, n_out);
}
int pbft_views_check(const ouro_pbft_views* v) { return views_check(v); }
int pbft_state_check(const ouro_pbft_state* st, const ouro_pbft_views& v, const uint8_t* id_out,
                     const uint64_t* slot_out, const size_t* n_out) {
  return state_check(st, v, id_out, slot_out, n_out);
}
int pbft_host_rows(size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                   const uint8_t* status, const ouro_pbft_views& v, uint8_t* pbft,
                   uint32_t* genesis_row) {
  return host_checks(n, delegate_vk, slot, status, v, pbft, genesis_row);
}
int pbft_upload(hipStream_t st, const ouro_pbft_views& v, Buf* buf, std::vector<uint8_t>* host,
                ouro_pbft_views* d) {
  views_pack(v, host, nullptr, nullptr);
  if (int rc = ensure(*buf, host->size())) return rc;
  OURO_HIP(hipMemcpyAsync(buf->p, host->data(), host->size(), hipMemcpyHostToDevice, st));
  views_pack(v, nullptr, d, static_cast<const uint8_t*>(buf->p));
  return OURO_OK;
}
}  // namespace ouro_rt

extern "C" {

int ouro_byron_key_hash_batch_host(size_t n, const uint8_t* xpub, uint8_t* out) {
  if (n && (!xpub || !out)) return fail(OURO_EINVAL, "null argument");
  return host_key_hash(n, xpub, out);
}

int ouro_byron_key_hash_batch(size_t n, const uint8_t* xpub, uint8_t* out) {
  if (n && (!xpub || !out)) return fail(OURO_EINVAL, "null argument");
  if (n == 0) return OURO_OK;
  return or_host(dev_key_hash(n, xpub, out), [&] { return host_key_hash(n, xpub, out); });
}

int ouro_byron_key_hash_batch_device(void* stream, size_t n, const uint8_t* xpub, uint8_t* out) {
  if (n == 0) return OURO_OK;
  if (!xpub || !out) return fail(OURO_EINVAL, "null argument");
  if (misaligned(xpub, 4) || misaligned(out, 4))
    return fail(OURO_EINVAL, "xpub and out must be 4-byte aligned");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_byron_key_hash(st, n, xpub, out);
}

// PBFT/State.hs:207-229 (append) under PBFT.hs:340-357, in stream order
int ouro_pbft_window_fold(size_t n, const uint32_t* genesis_row, const uint64_t* slot,
                          const ouro_pbft_views* views, const ouro_pbft_state* in,
                          uint8_t* signer_id_out, uint64_t* signer_slot_out, size_t* n_out,
                          uint8_t* pbft, uint64_t* signed_count) {
  int rc;
  if ((rc = views_check(views)) ||
      (rc = state_check(in, *views, signer_id_out, signer_slot_out, n_out)))
    return rc;
  if (n && (!genesis_row || !slot || !pbft)) return fail(OURO_EINVAL, "null argument");
  Fold f;
  f.begin(*views, in);
  f.run(n, genesis_row, slot, pbft, signed_count);
  f.end(signer_id_out, signer_slot_out, n_out);
  return OURO_OK;
}

int ouro_pbft_ledger_checks(size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                            const uint8_t* status, const ouro_pbft_views* views,
                            const ouro_pbft_state* state_in, uint8_t* signer_id_out,
                            uint64_t* signer_slot_out, size_t* n_out, uint8_t* pbft,
                            uint32_t* genesis_row, uint64_t* signed_count) {
  return checks_call(n, delegate_vk, slot, status, views, state_in, signer_id_out, signer_slot_out,
                     n_out, pbft, genesis_row, signed_count, false);
}

int ouro_pbft_ledger_checks_host(size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                                 const uint8_t* status, const ouro_pbft_views* views,
                                 const ouro_pbft_state* state_in, uint8_t* signer_id_out,
                                 uint64_t* signer_slot_out, size_t* n_out, uint8_t* pbft,
                                 uint32_t* genesis_row, uint64_t* signed_count) {
  return checks_call(n, delegate_vk, slot, status, views, state_in, signer_id_out, signer_slot_out,
                     n_out, pbft, genesis_row, signed_count, true);
}

int ouro_pbft_views_upload(const ouro_pbft_views* views, ouro_pbft_views_dev** out) {
  if (!out) return fail(OURO_EINVAL, "null out");
  *out = nullptr;
  if (int rc = views_check(views)) return rc;
  DeviceState* ds;
  int dev, rc = device_state(&ds);
  if (rc || (rc = current_device(&dev))) return rc;
  std::vector<uint8_t> blk;
  const size_t bytes = views_pack(*views, &blk, nullptr, nullptr);
  ouro_pbft_views_dev* dv = new (std::nothrow) ouro_pbft_views_dev{dev, nullptr, {}};
  if (!dv) return fail(OURO_EDEVICE, "out of host memory");
  if (hipMalloc(&dv->block, bytes) != hipSuccess ||
      hipMemcpy(dv->block, blk.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (dv->block) (void)hipFree(dv->block);
    delete dv;
    return fail(OURO_EDEVICE, "pbft views: upload failed");
  }
  views_pack(*views, nullptr, &dv->d, static_cast<const uint8_t*>(dv->block));
  *out = dv;
  return OURO_OK;
}

void ouro_pbft_views_free(ouro_pbft_views_dev* dv) {
  if (!dv) return;
  (void)hipFree(dv->block);
  delete dv;
}

int ouro_pbft_ledger_checks_device(void* stream, size_t n, const uint8_t* delegate_vk,
                                   const uint64_t* slot, const uint8_t* status,
                                   const ouro_pbft_views_dev* views, uint8_t* pbft,
                                   uint32_t* genesis_row) {
  if (!views) return fail(OURO_EINVAL, "null pbft views");
  if (n == 0) return OURO_OK;
  if (!delegate_vk || !slot || !status || !pbft || !genesis_row)
    return fail(OURO_EINVAL, "null argument");
  if (misaligned(delegate_vk, 4) || misaligned(genesis_row, 4))
    return fail(OURO_EINVAL, "delegate_vk and genesis_row must be 4-byte aligned");
  if (misaligned(slot, 8)) return fail(OURO_EINVAL, "slot must be 8-byte aligned");
  DeviceState* ds;
  int dev, rc = device_state(&ds);
  if (rc || (rc = current_device(&dev))) return rc;
  if (dev != views->dev) return fail(OURO_EINVAL, "pbft views were uploaded to another device");
  return launch_pbft(static_cast<hipStream_t>(stream), n, delegate_vk, slot, status, views->d, pbft,
                     genesis_row);
}

}  // extern "C"
