// chain_api.cpp -- the C entries over the raw-CBOR pipeline (include/
// ouro_verify.h *_verify_cbor, ouro_chain_*): each builds a RawCall
// (raw_call.h), checks what the engine's own checks do not cover, and runs it
// on the device pipeline (raw_pipe.cpp raw_verify) or on the host path alone
// (raw_verify_host).  Host code only: kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <new>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "host_util.h"
#include "launch.h"
#include "launches.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

// The arguments of an ouro_chain_* entry, in the entry's order: the chain
// kind's, then what a validating call adds (EnvIn), then what a ledger call
// adds (LedgerIn).
struct ChainIn {
  const uint8_t* raw;
  size_t raw_bytes;
  const uint64_t* off;
  const uint32_t* len;
  size_t n;
  uint64_t spkp;
  int64_t magic;
  const ouro_epoch_nonces* epochs;
  const uint8_t *ea, *la;
  uint8_t *proto, *status, *verdict, *be, *bl, *nonce;
};
struct EnvIn {
  const ouro_envelope_cfg* cfg;
  const ouro_chain_tip* tip_in;
  uint8_t *header_hash, *envelope;
  ouro_chain_tip* tip_out;
};
struct LedgerIn {
  const ouro_ledger_views* views;
  const ouro_genesis_delegs* genesis;
  const ouro_ledger_globals* globals;
  const ouro_ocert_counters* counters;
  uint64_t* counter_out;
  uint8_t* present_out;
  uint8_t* ledger;
  uint32_t* pool_row;
};

// A raw header stream across eras and epochs in one call (include/
// ouro_verify.h): every header classified (cbor.h era_class) while the
// pipeline gathers it, PBFT headers through the Byron slicer + ByronDSIGN
// kernel, TPraos headers through the TPraos slicer + header kernel with mkSeed
// under the epoch schedule, a mixed chunk through both on one upload.
struct ChainArgs {
  RawCall c;
  std::vector<uint64_t> tab;
};
int chain_call(ChainArgs* a, const ChainIn& in) {
  a->c = RawCall::of(kRawChain, in.raw, in.raw_bytes, in.off, in.len, in.n, in.status, in.verdict);
  a->c.spkp = in.spkp;
  a->c.ea = in.ea;
  a->c.la = in.la;
  a->c.be = in.be;
  a->c.bl = in.bl;
  a->c.nonce = in.nonce;
  a->c.magic = in.magic;
  a->c.proto = in.proto;
  if (in.n == 0) return OURO_OK;
  if (in.epochs) {
    if (int rc = epoch_tab_build(in.epochs, &a->tab)) return rc;
    a->c.epochs = reinterpret_cast<const uint8_t*>(a->tab.data());
    a->c.epochs_bytes = 8 * a->tab.size();
  }
  return raw_check(a->c);
}

// validateHeader's two halves over a raw chain in one call (ouroboros-consensus/
// src/Ouroboros/Consensus/HeaderValidation.hs:413-432): the chain kind's crypto
// as ouro_chain_verify_cbor runs it, and per chunk, on the same stream and over
// the bytes already uploaded, the envelope kernels (RawCall env).
int validate_call(ChainArgs* a, RawEnv* e, const EnvIn& in) {
  const RawCall& c = a->c;
  if (int rc = env_args(in.cfg, in.tip_in, &e->tip)) return rc;
  if (c.n == 0) {  // nothing to link: the checked tip passes through
    if (in.tip_out) env::tip_of_rec(in.tip_out, e->tip);
    return OURO_OK;
  }
  if (!in.header_hash || !in.envelope) return fail(OURO_EINVAL, "null header_hash or envelope");
  e->cfg = *in.cfg;
  e->prev = e->tip;
  e->hash = in.header_hash;
  e->envelope = in.envelope;
  e->tip_out = in.tip_out;
  a->c.env = e;
  // every span before anything runs: the call's one pass over them
  if (int rc = spans_check("header", "raw_bytes", c.raw_bytes, c.off, c.len, c.n)) return rc;
  a->c.spans_checked = true;
  if (in.cfg->byron_epoch_slots == 0) return env_needs_epoch_slots(c.raw, c.off, c.len, c.n);
  return OURO_OK;
}

// validateHeader with the ledger-view checks of SL.updateChainDepState
// (Shelley/Protocol.hs:433-442; ledger-specs OVERLAY and OCERT) in the same
// call: the validating call above with RawCall ledger set.
struct LedgerArgs {
  RawLedger l{};
  LvFold fold;
  std::vector<uint32_t> map, gmap, rows;
  // the table as the call found it (RawLedger table0 points here): the
  // ledger stage begins the fold from it, a device error recomputes from it
  std::vector<uint64_t> counter0;
  std::vector<uint8_t> present0;
};
int ledger_call(ChainArgs* a, LedgerArgs* g, const LedgerIn& in) {
  const size_t n = a->c.n;
  const ouro_ocert_counters* counters = in.counters;
  uint32_t* pool_row = in.pool_row;
  int rc;
  if ((rc = lv_views_check(in.views)) || (rc = lv_globals_check(in.globals))) return rc;
  if (in.genesis && (rc = lv_genesis_check(in.genesis, *in.views))) return rc;
  if (in.globals->slots_per_kes_period != a->c.spkp)
    return fail(OURO_EINVAL, "globals: slots_per_kes_period differs from the call's");
  if (n && !in.ledger) return fail(OURO_EINVAL, "null ledger");
  if ((rc = lv_counters_check(counters, in.counter_out, in.present_out))) return rc;
  if (counters && (rc = lv_fold_map(*in.views, *counters, &g->map))) return rc;
  if (counters && in.genesis && (rc = lv_fold_gmap(*in.genesis, *counters, &g->gmap))) return rc;
  try {  // (no exception crosses the C ABI)
    if (!pool_row) {
      g->rows.resize(n);
      pool_row = g->rows.data();
    }
    if (counters) {
      g->counter0.assign(counters->counter, counters->counter + counters->m);
      g->present0.assign(counters->present, counters->present + counters->m);
    }
  } catch (const std::bad_alloc&) {
    return fail(OURO_EDEVICE, "ledger call: out of host memory");
  }
  g->l.views = in.views;
  g->l.genesis = in.genesis;
  g->l.g = *in.globals;
  g->l.ledger = in.ledger;
  g->l.pool_row = pool_row;
  if (counters) {
    g->l.table0 = ouro_ocert_counters{counters->m, counters->pool_id, g->counter0.data(),
                                      g->present0.data()};
    g->fold.map = &g->map;
    g->fold.gmap = in.genesis ? &g->gmap : nullptr;
    g->fold.counter = in.counter_out;
    g->fold.present = in.present_out;
    g->l.fold = &g->fold;
    g->l.fold_begin();  // (n = 0 runs no ledger stage: the table passes through)
  }
  a->c.ledger = &g->l;
  return OURO_OK;
}

// The ledger call above with the Byron ledger-view checks (PBFT.hs:340-357;
// pbft_view.h) in the same call: RawCall pbft set.
struct PbftIn {
  const ouro_pbft_views* views;
  const ouro_pbft_state* state_in;
  uint8_t* signer_id_out;
  uint64_t* signer_slot_out;
  size_t* n_out;
  uint8_t* pbft;
  uint32_t* genesis_row;
  uint64_t* signed_count;
};
struct PbftArgs {
  RawPbft p{};
  std::vector<uint32_t> rows;
  // the window as the call found it (RawPbft state0 points here)
  std::vector<uint8_t> id0;
  std::vector<uint64_t> slot0;
  ~PbftArgs() { pbft_fold_free(p.fold); }
};
int pbft_call(ChainArgs* a, PbftArgs* g, const PbftIn& in) {
  const size_t n = a->c.n;
  int rc;
  if ((rc = pbft_views_check(in.views))) return rc;
  if (in.state_in &&
      (rc = pbft_state_check(in.state_in, *in.views, in.signer_id_out, in.signer_slot_out, in.n_out)))
    return rc;
  if (n && !in.pbft) return fail(OURO_EINVAL, "null pbft");
  uint32_t* rows = in.genesis_row;
  try {  // (no exception crosses the C ABI)
    if (!rows) {
      g->rows.resize(n);
      rows = g->rows.data();
    }
    if (in.state_in) {
      const size_t m = in.state_in->n;
      g->id0.assign(in.state_in->signer_id, in.state_in->signer_id + 28 * m);
      g->slot0.assign(in.state_in->signer_slot, in.state_in->signer_slot + m);
    }
  } catch (const std::bad_alloc&) {
    return fail(OURO_EDEVICE, "pbft call: out of host memory");
  }
  g->p.views = in.views;
  g->p.pbft = in.pbft;
  g->p.genesis_row = rows;
  g->p.signed_count = in.signed_count;
  if (in.state_in) {
    g->p.state0 = ouro_pbft_state{in.state_in->n, g->id0.data(), g->slot0.data()};
    if (!(g->p.fold = pbft_fold_new())) return fail(OURO_EDEVICE, "pbft call: out of host memory");
    g->p.fold_begin();  // (n = 0 runs no stage: the window passes through)
  }
  a->c.pbft = &g->p;
  return OURO_OK;
}

// The ouro_chain_* entries, each device / _host pair once: the chain
// arguments, then the ledger call's, then the validating call's and the
// spans, then the byron_epoch_slots scan; then the device pipeline or the
// host path alone.  (n = 0: the tip passes through, nothing is written.)
int chain_entry(const ChainIn& in, const EnvIn* env, const LedgerIn* ledger, bool host,
                const PbftIn* pbft = nullptr) {
  ChainArgs a;
  RawEnv e{};
  LedgerArgs g;
  PbftArgs pg;
  if (int rc = chain_call(&a, in)) return rc;
  if (ledger)
    if (int rc = ledger_call(&a, &g, *ledger)) return rc;
  if (pbft)
    if (int rc = pbft_call(&a, &pg, *pbft)) return rc;
  if (env)
    if (int rc = validate_call(&a, &e, *env)) return rc;
  const int rc = host ? raw_verify_host(a.c) : raw_verify(a.c);
  // the window after the call's last header
  if (!rc && pbft && pg.p.fold)
    pbft_fold_end(pg.p.fold, pbft->signer_id_out, pbft->signer_slot_out, pbft->n_out);
  return rc;
}

}  // namespace

extern "C" {

// ---- storage integrity (KES only) over raw headers ----
// verifyHeaderIntegrity (ouroboros-consensus-shelley/src/Ouroboros/Consensus/
// Shelley/Ledger/Integrity.hs:20-44): Sum6KES of the raw header body under the
// opcert's hot key at t = kesPeriod(slot) - c0 (0 below c0) -- the check the
// VolatileDB parser runs on every block at open
// (ouroboros-consensus/src/Ouroboros/Consensus/Storage/VolatileDB/Impl/Parser.hs:66-85)
// and ImmutableDB chunk validation on every block of a chunk
// (.../ImmutableDB/Impl/Validation.hs:358-365).  The raw-CBOR pipeline of
// raw_pipe.cpp: the device slicer (cbor.h, kes_t_of = Integrity.hs:38-44),
// then the Sum6KES kernel on its rows; a header the slicer rejects is 0.
int ouro_integrity_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                               const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                               uint8_t* status, uint8_t* verdict) {
  RawCall c = RawCall::of(kRawKes, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = slots_per_kes_period;
  return raw_verify(c);
}

// Raw TPraos headers -> the full header check (ouroboros-consensus-shelley/
// src/Ouroboros/Consensus/Shelley/Protocol.hs:433-442 over each decoded
// header) in one call through the raw-CBOR pipeline.
int ouro_tpraos_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                            const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                            const uint8_t* epoch_nonce, const uint8_t* eta_alpha,
                            const uint8_t* leader_alpha, uint8_t* status, uint8_t* verdict,
                            uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce) {
  RawCall c = RawCall::of(kRawHdr, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = slots_per_kes_period;
  c.eta0 = epoch_nonce;
  c.ea = eta_alpha;
  c.la = leader_alpha;
  c.be = beta_eta;
  c.bl = beta_leader;
  c.nonce = eta_nonce;
  return raw_verify(c);
}

// Raw Byron headers -> PBFT's block-signature verdicts (ouroboros-consensus/
// src/Ouroboros/Consensus/Protocol/PBFT.hs:332-338; the storage integrity
// check ouroboros-consensus-byron/src/Ouroboros/Consensus/Byron/Ledger/
// Integrity.hs:24-35) through the raw-CBOR pipeline: chunks gathered
// into pinned NUMA-local staging, the device Byron slicer (k_byron_pack, the
// host slicer's cbor_byron.h parse), then the Ed25519 kernel with ByronDSIGN
// acceptance, five chunks in flight.  An epoch-boundary header is 1 (status
// OURO_PACK_EBB); a rejected one 0.
int ouro_byron_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                           const uint32_t* len, size_t n, int64_t protocol_magic,
                           uint8_t* status, uint8_t* verdict) {
  RawCall c = RawCall::of(kRawByron, raw, raw_bytes, off, len, n, status, verdict);
  c.magic = protocol_magic;
  return raw_verify(c);
}

int ouro_chain_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                           const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                           int64_t protocol_magic, const ouro_epoch_nonces* epochs,
                           const uint8_t* eta_alpha, const uint8_t* leader_alpha, uint8_t* proto,
                           uint8_t* status, uint8_t* verdict, uint8_t* beta_eta,
                           uint8_t* beta_leader, uint8_t* eta_nonce) {
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     nullptr, nullptr, false);
}

int ouro_chain_verify_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                                int64_t protocol_magic, const ouro_epoch_nonces* epochs,
                                const uint8_t* eta_alpha, const uint8_t* leader_alpha,
                                uint8_t* proto, uint8_t* status, uint8_t* verdict,
                                uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce) {
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     nullptr, nullptr, true);
}

int ouro_chain_validate_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                             const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                             int64_t protocol_magic, const ouro_epoch_nonces* epochs,
                             const uint8_t* eta_alpha, const uint8_t* leader_alpha,
                             const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in,
                             uint8_t* proto, uint8_t* status, uint8_t* verdict, uint8_t* beta_eta,
                             uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
                             uint8_t* envelope, ouro_chain_tip* tip_out) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, nullptr, false);
}

int ouro_chain_validate_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                  const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                                  int64_t protocol_magic, const ouro_epoch_nonces* epochs,
                                  const uint8_t* eta_alpha, const uint8_t* leader_alpha,
                                  const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in,
                                  uint8_t* proto, uint8_t* status, uint8_t* verdict,
                                  uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce,
                                  uint8_t* header_hash, uint8_t* envelope,
                                  ouro_chain_tip* tip_out) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, nullptr, true);
}

int ouro_chain_validate_ledger_overlay_cbor(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_genesis_delegs* genesis, const ouro_ledger_globals* globals,
    const ouro_ocert_counters* counters, uint64_t* counter_out, uint8_t* present_out,
    uint8_t* ledger, uint32_t* pool_row) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  const LedgerIn l{views, genesis, globals, counters, counter_out, present_out, ledger, pool_row};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, &l, false);
}

// the overlay entry with the Byron ledger-view checks (a NULL schedule: the
// overlay entry itself)
int ouro_chain_validate_ledger_pbft_cbor(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_genesis_delegs* genesis, const ouro_ledger_globals* globals,
    const ouro_ocert_counters* counters, uint64_t* counter_out, uint8_t* present_out,
    uint8_t* ledger, uint32_t* pool_row, const ouro_pbft_views* pbft_views,
    const ouro_pbft_state* pbft_state_in, uint8_t* signer_id_out, uint64_t* signer_slot_out,
    size_t* n_out, uint8_t* pbft, uint32_t* genesis_row_pbft, uint64_t* signed_count) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  const LedgerIn l{views, genesis, globals, counters, counter_out, present_out, ledger, pool_row};
  const PbftIn p{pbft_views, pbft_state_in, signer_id_out, signer_slot_out, n_out, pbft,
                 genesis_row_pbft, signed_count};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, &l, false, pbft_views ? &p : nullptr);
}

int ouro_chain_validate_ledger_pbft_cbor_host(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_genesis_delegs* genesis, const ouro_ledger_globals* globals,
    const ouro_ocert_counters* counters, uint64_t* counter_out, uint8_t* present_out,
    uint8_t* ledger, uint32_t* pool_row, const ouro_pbft_views* pbft_views,
    const ouro_pbft_state* pbft_state_in, uint8_t* signer_id_out, uint64_t* signer_slot_out,
    size_t* n_out, uint8_t* pbft, uint32_t* genesis_row_pbft, uint64_t* signed_count) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  const LedgerIn l{views, genesis, globals, counters, counter_out, present_out, ledger, pool_row};
  const PbftIn p{pbft_views, pbft_state_in, signer_id_out, signer_slot_out, n_out, pbft,
                 genesis_row_pbft, signed_count};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, &l, true, pbft_views ? &p : nullptr);
}

int ouro_chain_validate_ledger_cbor(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_ledger_globals* globals, const ouro_ocert_counters* counters,
    uint64_t* counter_out, uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row) {
  return ouro_chain_validate_ledger_overlay_cbor(
      raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs, eta_alpha,
      leader_alpha, cfg, tip_in, proto, status, verdict, beta_eta, beta_leader, eta_nonce,
      header_hash, envelope, tip_out, views, nullptr, globals, counters, counter_out, present_out,
      ledger, pool_row);
}

int ouro_chain_validate_ledger_overlay_cbor_host(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_genesis_delegs* genesis, const ouro_ledger_globals* globals,
    const ouro_ocert_counters* counters, uint64_t* counter_out, uint8_t* present_out,
    uint8_t* ledger, uint32_t* pool_row) {
  const EnvIn e{cfg, tip_in, header_hash, envelope, tip_out};
  const LedgerIn l{views, genesis, globals, counters, counter_out, present_out, ledger, pool_row};
  return chain_entry({raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs,
                      eta_alpha, leader_alpha, proto, status, verdict, beta_eta, beta_leader,
                      eta_nonce},
                     &e, &l, true);
}

int ouro_chain_validate_ledger_cbor_host(
    const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces* epochs,
    const uint8_t* eta_alpha, const uint8_t* leader_alpha, const ouro_envelope_cfg* cfg,
    const ouro_chain_tip* tip_in, uint8_t* proto, uint8_t* status, uint8_t* verdict,
    uint8_t* beta_eta, uint8_t* beta_leader, uint8_t* eta_nonce, uint8_t* header_hash,
    uint8_t* envelope, ouro_chain_tip* tip_out, const ouro_ledger_views* views,
    const ouro_ledger_globals* globals, const ouro_ocert_counters* counters,
    uint64_t* counter_out, uint8_t* present_out, uint8_t* ledger, uint32_t* pool_row) {
  return ouro_chain_validate_ledger_overlay_cbor_host(
      raw, raw_bytes, off, len, n, slots_per_kes_period, protocol_magic, epochs, eta_alpha,
      leader_alpha, cfg, tip_in, proto, status, verdict, beta_eta, beta_leader, eta_nonce,
      header_hash, envelope, tip_out, views, nullptr, globals, counters, counter_out, present_out,
      ledger, pool_row);
}

// Storage integrity on raw headers already in device memory (raw, off, len,
// arena, status, verdict: device pointers; arena >= ouro_tpraos_pack_bytes(n)):
// the device slicer and the Sum6KES kernel enqueued on `stream`, not
// synchronised.  A rejected header's zeroed row (OURO_PACK_*) cannot verify.
int ouro_integrity_verify_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                      const uint64_t* off, const uint32_t* len, size_t n,
                                      uint64_t slots_per_kes_period, void* arena,
                                      size_t arena_bytes, uint8_t* status, uint8_t* verdict) {
  if (n == 0) return OURO_OK;
  if (!verdict) return fail(OURO_EINVAL, "null verdict");
  ouro_tpraos_batch b{};
  int rc = ouro_tpraos_pack_cbor_device(stream, raw, raw_bytes, off, len, n,
                                        slots_per_kes_period, arena, arena_bytes, &b, nullptr,
                                        nullptr, status);
  if (rc) return rc;
  hipStream_t st;
  if ((rc = device_entry(stream, &st))) return rc;
  return launch_kes(st, n, b.hot_vk, b.kes_t, b.body, b.body_off, b.body_len, b.kes_sig, verdict);
}

}  // extern "C"
