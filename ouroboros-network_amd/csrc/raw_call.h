// raw_call.h -- one raw-CBOR call (RawCall) and what a validating or a ledger
// call adds to it (RawEnv, RawLedger), shared by the pipeline engine
// (raw_pipe.cpp), its host path (raw_host.cpp), the entries over them
// (chain_api.cpp, block_api.cpp, multi.cpp) and the stages a call runs
// (envelope_api.cpp, ledger_api.cpp).  Host units only; internal to the
// library (hidden visibility), like runtime.h.
#pragma once
#include <vector>

#include "../../include/ouro_verify.h"
#include "envelope.h"
#include "runtime.h"

#pragma GCC visibility push(hidden)
namespace ouro_rt {

// (kRawChain: Byron and TPraos headers in one stream, classified per header)
// (kRawBlock: whole Shelley-family blocks, KES + body hash; block_api.cpp)
enum RawKind { kRawHdr = 0, kRawKes = 1, kRawByron = 2, kRawChain = 3, kRawBlock = 4 };
// What a validating call (ouro_chain_validate_cbor) adds to the chain kind:
// the envelope of every header (envelope.h).  prev: the record the next
// drained chunk's first header links to (the tip, then each chunk's last).
struct RawEnv {
  ouro_envelope_cfg cfg;
  ouro::env::Rec tip, prev;
  uint8_t *hash, *envelope;  // OUT: n x 32, n
  ouro_chain_tip* tip_out;   // OUT, or null
};
// ---- the ledger-view checks (ledger_api.cpp; ledger_view.h) ----
// the OCERT counter fold's state: the view-row -> table-index map and the
// table being updated (the caller's counter_out / present_out); gmap: the
// same map for the genesis rows of a call with a genesis-delegation schedule
// (keyed by delegate_id), or null: overlay rows are skipped
struct LvFold {
  const std::vector<uint32_t>* map = nullptr;
  const std::vector<uint32_t>* gmap = nullptr;
  uint64_t* counter = nullptr;
  uint8_t* present = nullptr;
};
int lv_views_check(const ouro_ledger_views* v);
int lv_globals_check(const ouro_ledger_globals* g);
int lv_genesis_check(const ouro_genesis_delegs* gd, const ouro_ledger_views& v);
int lv_counters_check(const ouro_ocert_counters* t, const uint64_t* counter_out,
                      const uint8_t* present_out);
int lv_host_rows(size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk, const uint64_t* slot,
                 const uint8_t* leader_output, const uint64_t* c0, const ouro_ledger_views& v,
                 const ouro_ledger_globals& g, const ouro_genesis_delegs* gd, uint8_t* ledger,
                 uint32_t* pool_row);
int lv_upload(hipStream_t st, const ouro_ledger_views& v, const ouro_genesis_delegs* gd, Buf* buf,
              std::vector<uint8_t>* host, ouro_ledger_views* d, ouro_genesis_delegs* dgd);
int lv_launch(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
              const uint64_t* slot, const uint8_t* leader_output, const uint64_t* ocert_kes_period,
              const ouro_ledger_views& v, const ouro_ledger_globals& g,
              const ouro_genesis_delegs* gd, uint8_t* ledger, uint32_t* pool_row);
int lv_fold_map(const ouro_ledger_views& v, const ouro_ocert_counters& t,
                std::vector<uint32_t>* map);
int lv_fold_gmap(const ouro_genesis_delegs& gd, const ouro_ocert_counters& t,
                 std::vector<uint32_t>* gmap);
void lv_fold_begin(LvFold* f, const ouro_ocert_counters& t, const std::vector<uint32_t>* map,
                   const std::vector<uint32_t>* gmap, uint64_t* counter_out, uint8_t* present_out);
void lv_fold_run(LvFold* f, size_t n, const uint32_t* pool_row, const uint64_t* counter,
                 uint8_t* ledger);
// What ouro_chain_validate_ledger_cbor adds to a validating call: the views
// (uploaded once per call: dviews, `uploaded` for the chunks' streams to wait
// on), the genesis-delegation schedule (or null; uploaded in the views' block:
// dgenesis), the fold (or null) and the outputs.
struct RawLedger {
  const ouro_ledger_views* views;
  const ouro_genesis_delegs* genesis = nullptr;
  ouro_genesis_delegs dgenesis{};
  ouro_ledger_globals g;
  LvFold* fold;        // null: no counters given
  // the counters table as the call found it (a copy of the call's own, so the
  // caller's outputs may alias the caller's table)
  ouro_ocert_counters table0{};
  uint8_t* ledger;     // OUT: n
  uint32_t* pool_row;  // OUT: n
  ouro_ledger_views dviews{};
  std::vector<uint8_t> packed;
  hipEvent_t uploaded = nullptr;
  // The fold at table0, where the ledger stage starts: the device pipeline
  // (raw_run), and again the host path (raw_host_ledger) -- after a device
  // error the chunks that drained have moved the outputs.  Idempotent.
  void fold_begin() {
    if (fold) lv_fold_begin(fold, table0, fold->map, fold->gmap, fold->counter, fold->present);
  }
};
// ---- the Byron ledger-view checks (pbft_api.cpp; pbft_view.h) ----
// the signing-window fold's state (pbft_api.cpp): begin copies the incoming
// state (null: the empty window), run folds rows in stream order, end writes
// the window out
struct PbftFold;
PbftFold* pbft_fold_new();
void pbft_fold_free(PbftFold* f);
void pbft_fold_begin(PbftFold* f, const ouro_pbft_views& v, const ouro_pbft_state* st);
void pbft_fold_run(PbftFold* f, size_t n, const uint32_t* genesis_row, const uint64_t* slot,
                   uint8_t* pbft, uint64_t* signed_count);
void pbft_fold_end(const PbftFold* f, uint8_t* id_out, uint64_t* slot_out, size_t* n_out);
int pbft_views_check(const ouro_pbft_views* v);
int pbft_state_check(const ouro_pbft_state* st, const ouro_pbft_views& v, const uint8_t* id_out,
                     const uint64_t* slot_out, const size_t* n_out);
int pbft_host_rows(size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                   const uint8_t* status, const ouro_pbft_views& v, uint8_t* pbft,
                   uint32_t* genesis_row);
// a checked schedule packed and uploaded as one block on `st` (not
// synchronised; *host must stay alive until the copy has completed)
int pbft_upload(hipStream_t st, const ouro_pbft_views& v, Buf* buf, std::vector<uint8_t>* host,
                ouro_pbft_views* d);
// What ouro_chain_validate_ledger_pbft_cbor adds to a ledger call: the
// delegation schedule (uploaded once per call behind the ledger views' event:
// dviews), the fold (begun from state0, the window as the call found it -- a
// copy, so the caller's outputs may alias it) and the outputs.
struct RawPbft {
  const ouro_pbft_views* views;
  ouro_pbft_views dviews{};
  std::vector<uint8_t> packed;
  PbftFold* fold;           // null: no state given
  ouro_pbft_state state0{};
  uint8_t* pbft;            // OUT: n
  uint32_t* genesis_row;    // OUT: n
  uint64_t* signed_count;   // OUT: n, or null
  // the fold at state0, where the stage starts: the device pipeline, and again
  // the host path after a device error.  Idempotent.
  void fold_begin() {
    if (fold) pbft_fold_begin(fold, *views, &state0);
  }
};
struct RawCall {
  RawKind kind = kRawHdr;
  const uint8_t* raw = nullptr;
  size_t raw_bytes = 0;
  const uint64_t* off = nullptr;
  const uint32_t* len = nullptr;
  size_t n = 0;
  uint64_t spkp = 0;
  const uint8_t* eta0 = nullptr;                // epoch nonce (32 B), or null = NeutralNonce
  const uint8_t *ea = nullptr, *la = nullptr;   // explicit VRF inputs (n x 32 each), or null: mkSeed
  uint8_t* status = nullptr;
  uint8_t* verdict = nullptr;
  uint8_t *be = nullptr, *bl = nullptr, *nonce = nullptr;  // optional outputs (header kind)
  int64_t magic = -1;            // Byron: the configured ProtocolMagicId (-1: each header's)
  uint8_t* proto = nullptr;      // chain kind: OUT, OURO_PROTO_* per header
  // an epoch-nonce schedule block (epoch_tab_build), or null; header / chain kinds
  const uint8_t* epochs = nullptr;
  size_t epochs_bytes = 0;
  uint8_t* body_hash = nullptr;  // block kind: OUT, the computed bbHash (n x 32), or null
  RawEnv* env = nullptr;         // chain kind: also the header envelope (validate), or null
  RawLedger* ledger = nullptr;   // chain kind: also the ledger-view checks, or null
  RawPbft* pbft = nullptr;       // a ledger call: also the Byron ledger-view checks, or null
  // every span was checked by the entry (between its other argument checks):
  // raw_verify / raw_verify_host do not walk them again
  bool spans_checked = false;

  // the members every kind has; the others are set by name
  static RawCall of(RawKind kind, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                    const uint32_t* len, size_t n, uint8_t* status, uint8_t* verdict) {
    RawCall c;
    c.kind = kind;
    c.raw = raw;
    c.raw_bytes = raw_bytes;
    c.off = off;
    c.len = len;
    c.n = n;
    c.status = status;
    c.verdict = verdict;
    return c;
  }
};
// the argument checks of a raw call that need no pass over the headers
int raw_check(const RawCall& c);
// the device pipeline (raw_pipe.cpp), after a device error the host path
int raw_verify(const RawCall& c);
// the same call on the host path alone (ouro_chain_verify_cbor_host)
int raw_verify_host(const RawCall& c);
// raw_host.cpp: the host path over a checked call
int raw_host(const RawCall& c);
// block_api.cpp: the block kind's device sequence on one stream (a: the
// 64-byte aligned arena of cbor::block_layout(n)) and its host path
int block_launch(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                 const uint32_t* dlen, size_t n, uint64_t spkp, uint8_t* a, uint8_t* dstatus,
                 uint8_t* dverdict, uint8_t* dbody_hash);
int block_host(const RawCall& c);
// envelope_api.cpp: the envelope of n raw host headers on the host path
// (status may be null); and the checks / conversion of a cfg and a tip
int env_host_run(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n,
                 const ouro_envelope_cfg& cfg, const ouro::env::Rec& tip, uint8_t* status,
                 uint8_t* hash, uint8_t* envelope, ouro::env::Rec* last);
int env_args(const ouro_envelope_cfg* cfg, const ouro_chain_tip* tip_in, ouro::env::Rec* tip);
int env_needs_epoch_slots(const uint8_t* raw, const uint64_t* off, const uint32_t* len, size_t n);

}  // namespace ouro_rt
#pragma GCC visibility pop
