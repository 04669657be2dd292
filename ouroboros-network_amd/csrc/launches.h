// launches.h -- what the kernel unit (kernels.hip) offers the host runtime:
// one launch function per kernel or kernel sequence.  The host units reach the
// kernels only through these; no host unit holds a kernel or a launch
// (tests/test_abi.py::test_no_getenv_on_call_paths).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ouro_verify.h"
#include "cbor.h"
#include "cbor_block.h"
#include "cbor_byron.h"
#include "forge_args.h"

// the byte ranges of a plan window's copy kernel (kernels.hip
// k_plan_stage_ranges), filled by ouro_tpraos_plan_submit (plan.cpp)
constexpr int kPlanMaxRanges = 24;
struct PlanRanges {
  uint32_t count;
  uint32_t start16[kPlanMaxRanges];
  uint32_t len16[kPlanMaxRanges];
};

int lat_fused_items_host();  // kernels_lat.hip: waves per header of the fused launch
int lat_stamps_read(unsigned long long* out);  // kernels_lat.hip: the latency probe's stamps

#pragma GCC visibility push(hidden)
namespace ouro_rt {

struct DeviceState;  // runtime.h

enum KernelId { kEd = 0, kVrf = 1, kKes = 2, kHdr = 3, kP2H = 4, kCores = 5, kFinish = 6,
                kLeader = 7, kHdrPre = 8, kHdrDsm = 9, kHdrPost = 10, kEdPre = 11, kKesPre = 12,
                kOcertUnique = 13, kNumKernels = 14 };
const void* kernel_ptr(int id);

// byron = 1: ByronDSIGN acceptance (cardano-crypto)
int launch_ed(hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
              const uint64_t* off, const uint32_t* len, uint8_t* verdict, uint32_t byron = 0);
int launch_vrf(hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* proof,
               const uint8_t* alpha, const uint64_t* off, const uint32_t* len, uint8_t* beta,
               uint8_t* verdict, uint32_t flags = 0);
int launch_kes(hipStream_t st, size_t n, const uint8_t* vk, const uint32_t* t, const uint8_t* msg,
               const uint64_t* off, const uint32_t* len, const uint8_t* sig, uint8_t* verdict);
// epochs: a device epoch-nonce schedule (tpraos.h epoch_tab_*), or null
int launch_hdr(hipStream_t st, const ouro_tpraos_batch& b, uint8_t* verdict, uint8_t* be,
               uint8_t* bl, const uint8_t* epochs = nullptr);
int launch_leader(hipStream_t st, size_t n, const uint8_t* beta, const uint64_t* num,
                  const uint64_t* den, int64_t lhi, uint64_t llo, int f_is_one,
                  uint8_t* verdict);

// the ledger-view checks (ledger_view.h k_ledger_checks) over n sliced header
// rows; v: a schedule whose pointers are device pointers, 8-byte aligned
int launch_ledger(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                  const uint64_t* slot, const uint8_t* leader_output,
                  const uint64_t* ocert_kes_period, const ouro_ledger_views& v,
                  const ouro_ledger_globals& g, uint8_t* ledger, uint32_t* pool_row);
// the same with a genesis-delegation schedule of device pointers
// (k_ledger_checks_overlay)
int launch_ledger_overlay(hipStream_t st, size_t n, const uint8_t* issuer_vk, const uint8_t* vrf_vk,
                          const uint64_t* slot, const uint8_t* leader_output,
                          const uint64_t* ocert_kes_period, const ouro_ledger_views& v,
                          const ouro_ledger_globals& g, const ouro_genesis_delegs& gd,
                          uint8_t* ledger, uint32_t* pool_row);

// the Byron ledger-view checks (kernels_pbft.hip; pbft_view.h): k_pbft_checks
// over n Byron header rows (delegate_vk n x 64, 4-byte aligned; v: a schedule
// whose pointers are device pointers) and k_byron_key_hash over n XPubs.  Both
// cap their grid at launch_ledger's block count (kPbftBlocksMax) and stride over the rest.
constexpr size_t kPbftBlocksMax = 4096;
int launch_pbft(hipStream_t st, size_t n, const uint8_t* delegate_vk, const uint64_t* slot,
                const uint8_t* status, const ouro_pbft_views& v, uint8_t* pbft,
                uint32_t* genesis_row);
int launch_byron_key_hash(hipStream_t st, size_t n, const uint8_t* xpub, uint8_t* out);
// k_pbft_checks_chain: the same rule over a chunk's n PBFT rows in the Byron
// slicer's arena, the slot of row j read from the envelope record (envelope.h
// Rec) idx[j] of `rec` (idx null: record j); slot_out[j] receives it
int launch_pbft_chain(hipStream_t st, size_t n, const uint8_t* delegate_vk, const uint8_t* status,
                      const void* rec, const uint32_t* idx, const ouro_pbft_views& v,
                      uint8_t* pbft, uint32_t* genesis_row, uint64_t* slot_out);

// latency mode: eight cores per header (x4 lanes in quad mode), then the
// finish; n and the option bits read from d_n[0..1].
// Lanes used <= the kBlock-rounded count lowlat_scratch_words provides for.
// The launch shape (grids, option bits: the OURO_LAT_* switches) is fixed per
// capacity; a plan computes it once at build (lat_shape) and issues it per
// window (lat_issue) when it launches without a graph.
struct LatShape {
  int g1 = 0, g2 = 0, blk = 0, quad = 0, wide_lanes = 0;
  bool fused = false;
  uint32_t flags = 0;
  const int32_t* btab = nullptr;
};

int lat_shape(size_t n_cap, LatShape* s);
// (win_ctr / done: a plan's window counter and done word, or null)
void lat_issue(hipStream_t st, const LatShape& s, const ouro_tpraos_batch& b, const uint32_t* d_n,
               int32_t* res_buf, int32_t* scratch, uint8_t* verdict, uint8_t* be, uint8_t* bl,
               uint32_t* win_ctr = nullptr, uint32_t* done = nullptr);
int launch_lowlat(hipStream_t st, const ouro_tpraos_batch& b, const uint32_t* d_n, size_t n_cap,
                  int32_t* res_buf, int32_t* scratch, uint8_t* verdict, uint8_t* be,
                  uint8_t* bl);
size_t lowlat_scratch_words(DeviceState* ds, size_t n_cap);

// the kernels the runtime launches itself (grid of `blocks` workgroups; the
// caller checks the launch, runtime.h launch_check)
void launch_tpraos_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                        const uint64_t* off, const uint32_t* len, size_t n, uint64_t spkp,
                        const ouro::cbor::Out& o, uint8_t* status);
void launch_byron_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                       const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
                       const ouro::cbor::ByronOut& o, uint8_t* status);
// whole-block storage integrity (cbor_block.h): the block slicer, the batched
// Blake2b-256 (work: cbor::b2b_work_bytes(m) bytes of device memory, 64-byte
// aligned; checks its own launches) and the body-hash finish
void launch_block_pack(hipStream_t st, unsigned blocks, const uint8_t* raw, size_t raw_bytes,
                       const uint64_t* off, const uint32_t* len, size_t n, uint64_t spkp,
                       const ouro::cbor::Out& o, const ouro::cbor::BlockOut& bo, uint8_t* status);
int launch_blake2b(hipStream_t st, size_t m, const uint8_t* msg, size_t msg_bytes,
                   const uint64_t* off, const uint32_t* len, uint8_t* out, void* work);
void launch_block_finish(hipStream_t st, unsigned blocks, size_t n, const uint8_t* status,
                         const uint8_t* digest, const uint8_t* claimed, const uint8_t* kes,
                         uint8_t* verdict, uint8_t* body_hash);
// the header envelope (envelope.h): k_envelope_slice, k_header_hash and
// k_envelope_link over n raw headers; rec: n records, 64-byte aligned; raw
// 4-byte aligned, header_hash 16-byte aligned (checks its own launches);
// ends (optional, device): receives the first and the last record
int launch_envelope(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                    const uint32_t* len, size_t n, const ouro_envelope_cfg& cfg,
                    const ouro::env::Rec& tip, ouro::env::Rec* rec, uint8_t* status,
                    uint8_t* header_hash, uint8_t* envelope, ouro_chain_tip* tip_out,
                    ouro::env::Rec* ends = nullptr);
void launch_vrf03_proof_to_hash(hipStream_t st, unsigned blocks, size_t n, const uint8_t* proof,
                                uint8_t* beta, uint8_t* verdict);
void launch_plan_stage(hipStream_t st, unsigned blocks, const uint4* src, uint4* dst, size_t n16,
                       uint64_t* stamp);
void launch_plan_stage_ranges(hipStream_t st, unsigned blocks, const uint4* src, uint4* dst,
                              const PlanRanges& r, uint64_t* stamp);

// ---- the two-level exclusive scan (scan_excl.h), as the host units size it ----
// a tile is kScanTile consecutive items; the work of a scan of `vals` count
// arrays over n items: vals * scan_tiles(n) words of tile sums, then
// scan_rows_words(vals) words: rows[q] = min(total, capacity), rows[vals + q] =
// the total
constexpr size_t kScanTile = 1024;
inline size_t scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }
constexpr size_t scan_rows_words(int vals) { return 2 * (size_t)vals; }

// ---- the transaction-witness kernels, Shelley (kernels_witness.hip;
// cbor_witness.h) and Byron (kernels_byron_witness.hip; cbor_byron_witness.h),
// each checking its own launches.  Every pointer is device memory.  One
// sequence over n blocks (witness_flow.h lays it out): ----
constexpr int kWitnessVals = 2;  // the scanned count arrays: ntx, nwit
struct WitnessDev {
  uint32_t *ntx, *nwit;   // n each: the count pass
  uint64_t *sums, *rows;  // kWitnessVals * scan_tiles(n); scan_rows_words(kWitnessVals)
  uint64_t* magic;        // n: the magic block i's messages use (Byron; null for Shelley)
  // tx_cap spans for launch_blake2b; vk (wit_cap x 32, Byron x 64: a redeem key
  // then 32 zero bytes) and sig (wit_cap x 64), 16-byte aligned; b2b:
  // launch_blake2b's work (tx_cap items)
  uint64_t* tx_off;
  uint32_t* tx_len;
  uint8_t *vk, *sig;
  void* b2b;
  // the call's rows (ouro_block_witness_out): block i owns the rows from
  // tx_begin[i] / wit_begin[i] (n + 1 each, [n] = the totals) as far as the
  // capacities hold them; wit_tx = tx_base + the transaction's row of tx_id
  size_t tx_cap, wit_cap;
  uint64_t *tx_begin, *wit_begin;
  uint64_t tx_base;
  uint8_t* tx_id;
  uint32_t* wit_tx;
  uint8_t *kind, *wit_ok;
};
// count: status, ntx and nwit per block (zeros unless the status is OURO_PACK_OK)
// scan: both count arrays into tx_begin / wit_begin, cut at tx_cap / wit_cap;
//   rows[1] = min(total, wit_cap) is the row count the later kernels read
// emit: every row to "not written", then the emit pass of the blocks that fit
//   (status OURO_PACK_ECAP for a sliced one that does not); magic_cfg: the
//   configured magic, or -1: each header's own field (Byron; Shelley ignores it)
// verify: per witness row, Ed25519 over its transaction id / ByronDSIGN under
//   vk[0:32] over tag || CBOR(magic) || 58 20 || tx id, the message built in
//   the lane; rows nothing was emitted to and rows past the count get zeros
// finish: n_bad[i] and verdict[i] = OURO_WIT_ALL_OK / OURO_BYW_ALL_OK (Byron:
//   for an EBB too)
// The two families have one shape, so that witness_flow.h names either.
int launch_witness_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                         const uint32_t* len, size_t n, uint8_t* status, uint32_t* ntx,
                         uint32_t* nwit);
int launch_witness_scan(hipStream_t st, size_t n, const WitnessDev& d);
int launch_witness_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off, const uint32_t* len,
                        size_t n, int64_t magic_cfg, const WitnessDev& d, uint8_t* status);
int launch_witness_verify(hipStream_t st, size_t n, const WitnessDev& d);
int launch_witness_finish(hipStream_t st, size_t n, const uint8_t* status, const WitnessDev& d,
                          uint8_t* verdict, uint32_t* n_bad);
int launch_byron_witness_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes,
                               const uint64_t* off, const uint32_t* len, size_t n, uint8_t* status,
                               uint32_t* ntx, uint32_t* nwit);
int launch_byron_witness_scan(hipStream_t st, size_t n, const WitnessDev& d);
int launch_byron_witness_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off,
                              const uint32_t* len, size_t n, int64_t magic_cfg, const WitnessDev& d,
                              uint8_t* status);
int launch_byron_witness_verify(hipStream_t st, size_t n, const WitnessDev& d);
int launch_byron_witness_finish(hipStream_t st, size_t n, const uint8_t* status,
                                const WitnessDev& d, uint8_t* verdict, uint32_t* n_bad);

// the Byron whole-block integrity kernels (kernels_byron_block.hip;
// cbor_byron_block.h), each checking its own launches.  Every pointer is device
// memory.  The rows of one sequence over n blocks (byron_block_api.cpp lays
// them out; each array 64-byte aligned):
struct ByronBlockDev {
  uint32_t *ntx, *gather_n, *msg_n;  // n each: the count pass
  uint64_t *sums, *rows;             // 3 * scan_tiles(n); 6: capped totals, totals
  // n + 1 each ([n] = the totals); msg_off is the third.  msg_off is a scan only
  // until the emit pass: emit leaves a block's own begin where it wrote a
  // message and puts 0 where it wrote none (an EBB, a block that does not
  // slice or does not fit), so that the signature launch reads inside the
  // message area; [n] stays the total.  tx_begin and g_begin stay scans.
  uint64_t *tx_begin, *g_begin;
  // the Byron rows of the blocks (cbor_byron.h ByronOut; msg_off n + 1, msg: msg_cap bytes)
  uint8_t *pk, *sig, *genesis_vk, *delegate_vk, *msg;
  uint64_t *msg_off, *magic;
  uint32_t* msg_len;
  // per block: claimed hashes (n x 128), txpNumber, the dlg / upd spans (2n),
  // the gathered witness list's span; per tx row: the tx span; the gather
  // area (gather_cap bytes, allocated up to the next multiple of 4)
  uint8_t* claimed;
  uint32_t* tx_num;
  uint64_t* seg_off;
  uint32_t* seg_len;
  uint64_t* g_off;
  uint32_t* g_len;
  uint64_t* tx_off;
  uint32_t* tx_len;
  uint8_t* gather;
  // digests: leaves (tx_cap x 32), roots and witness lists (n x 32 each), dlg
  // and upd (2n x 32); the signature verdicts (n); launch_blake2b's work (2n items)
  uint8_t *leaf, *root, *wit_digest, *seg_digest, *sig_ok;
  void* b2b;
};
// count: status, ntx, gathered witness bytes and message bytes per block
// (zeros unless the status is OURO_PACK_OK); magic: the configured
// ProtocolMagicId or -1 (it decides the message's length)
int launch_byron_block_count(hipStream_t st, const uint8_t* raw, size_t raw_bytes,
                             const uint64_t* off, const uint32_t* len, size_t n, int64_t magic,
                             uint8_t* status, uint32_t* ntx, uint32_t* gather, uint32_t* msg);
// the exclusive scan of the three count arrays (n + 1 each, [n] = the totals);
// rows[q] = min(total, capacity), rows[3 + q] = total
int launch_byron_block_scan(hipStream_t st, size_t n, const uint32_t* ntx, const uint32_t* gather,
                            const uint32_t* msg, uint64_t* sums, uint64_t* tx_begin,
                            uint64_t* g_begin, uint64_t* msg_begin, size_t tx_cap,
                            size_t gather_cap, size_t msg_cap, uint64_t* rows);
// every tx row to "not written", then the emit pass of the blocks that fit
// (OURO_PACK_ECAP for a regular one that does not; zero rows for every block
// nothing is emitted for)
int launch_byron_block_emit(hipStream_t st, const uint8_t* raw, const uint64_t* off,
                            const uint32_t* len, size_t n, int64_t magic, const uint32_t* ntx,
                            const uint32_t* gather, const uint32_t* msg, const uint64_t* tx_begin,
                            const uint64_t* g_begin, size_t tx_cap, size_t gather_cap,
                            size_t msg_cap, const ByronBlockDev& d, uint8_t* status);
// leaf digests of the tx rows (the row count read from rows[0]; raw 4-byte aligned)
int launch_byron_leaf_hash(hipStream_t st, size_t tx_cap, const uint64_t* rows, const uint8_t* raw,
                           size_t raw_bytes, const uint64_t* tx_off, const uint32_t* tx_len,
                           uint8_t* digest);
// root[i] = the Merkle root of block i's leaf digests (reduced in place)
int launch_byron_merkle(hipStream_t st, size_t n, const uint8_t* status, const uint32_t* ntx,
                        const uint64_t* tx_begin, uint8_t* digest, uint8_t* root);
// verdict[i] = OURO_BYB_* bits; tx_root (optional): n x 32, 16-byte aligned
int launch_byron_block_finish(hipStream_t st, size_t n, int64_t magic, const uint8_t* status,
                              const uint32_t* ntx, const uint32_t* tx_num,
                              const uint64_t* hdr_magic, const uint8_t* claimed,
                              const uint8_t* root, const uint8_t* wit, const uint8_t* seg,
                              const uint8_t* sig_ok, uint8_t* verdict, uint8_t* tx_root);

// the forging-side kernels (kernels_forge.hip; forge.h), each checking its own
// launch, on k_ed25519_verify's launch shape and scratch slots.  Every pointer
// is device memory, 16-byte aligned.
// checkIsLeader for slots first_slot .. first_slot + n - 1: cls (n bytes),
// gen_index (n, optional), beta (n x 64, optional); s travels with the launch
int launch_leader_schedule(hipStream_t st, const OuroForgeSched& s, uint64_t first_slot, size_t n,
                           uint8_t* cls, uint32_t* gen_index, uint8_t* beta);
// n certified VRFs: sk n x 64, or one row when shared_key.  slot null: alpha
// spans (off / len; the buffer allocated up to the next multiple of 4).  Else
// item i proves mkSeed(seedEta for even i, seedL for odd i, slot[i / 2], eta0)
// (eta0: 32 bytes, null = NeutralNonce).  proof n x 80; beta n x 64, optional
int launch_vrf_prove(hipStream_t st, size_t n, const uint8_t* sk, bool shared_key,
                     const uint8_t* alpha, const uint64_t* off, const uint32_t* len,
                     const uint64_t* slot, const uint8_t* eta0, uint8_t* proof, uint8_t* beta);

}  // namespace ouro_rt
#pragma GCC visibility pop
