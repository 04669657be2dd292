// envelope.h -- the header envelope (ouroboros-consensus/src/Ouroboros/
// Consensus/HeaderValidation.hs:297-344, validateEnvelope): the per-header
// record the slicers fill (cbor.h pack_fields, cbor_byron.h byron_pack_one)
// and the ONE link rule that the link kernel (kernels.hip k_envelope_link),
// the host path and the chaining of calls (ouro_chain_tip) all use.
// envelope.py restates the rule from the reference; tests/test_envelope_rule.py
// pins the two against each other.  Plain C++: host and device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouro_verify.h"
#if defined(__HIPCC__)
#include "common.h"
#elif !defined(OURO_HD)
#define OURO_HD
#endif

namespace ouro {
namespace env {

// headerPrevHash: GenesisHash, BlockHash h, or a field that is neither (TPraos
// field 2 other than null / bytes(32): the previous-hash bit is then clear)
enum { kPrevGenesis = 0, kPrevBlock = 1, kPrevBad = 2 };

// One header as validateEnvelope sees it.  `sliced`: the slicer accepted the
// header AND its envelope fields have their shape (an epoch-boundary header is
// accepted without a look inside; its fields are read here only).  A record
// with sliced = 0 is all zero.  hdr_off / hdr_len: the span the header hash
// covers, inside the raw buffer the slicer ran over.
struct Rec {
  uint64_t slot, block_no;
  uint64_t body_size, prot_major;  // TPraos header body fields 7 and 13
  uint64_t hdr_off;
  uint32_t hdr_len;
  uint32_t header_size;  // TPraos: bytes of the [header_body, kes_sig] item
  uint8_t sliced, proto, is_ebb, prev_kind;
  uint8_t origin;     // a tip only: no header yet (WithOrigin's Origin)
  uint8_t limits_ok;  // TPraos: fields 7 and 13 are uints
  uint8_t pad[10];
  uint8_t prev_hash[32];
  uint8_t hash[32];
};
static_assert(sizeof(Rec) == 128, "Rec is 128 bytes: 16 qwords");

OURO_HD inline void rec_clear(Rec* r) {
  uint64_t* q = reinterpret_cast<uint64_t*>(r);
  for (int k = 0; k < 16; k++) q[k] = 0;
}

// the two prefix bytes of a Byron header hash, 0x82 then the kind (1 regular,
// 0 epoch boundary): wrapBoundaryBytes / the regular header's twin
// (ouroboros-consensus-byron/src/Ouroboros/Consensus/Byron/Ledger/Orphans.hs:101,
// Block.hs:74); a TPraos header hash has none (Shelley/Ledger/Block.hs:106,142)
OURO_HD inline uint32_t hash_prefix(const Rec& r, uint32_t* npre) {
  if (r.proto != OURO_PROTO_PBFT) {
    *npre = 0;
    return 0;
  }
  *npre = 2;
  return 0x82u | ((r.is_ebb ? 0u : 1u) << 8);
}

OURO_HD inline Rec rec_of_tip(const ouro_chain_tip* t) {
  Rec r;
  rec_clear(&r);
  if (!t || t->origin) {
    r.origin = 1;
    return r;
  }
  r.sliced = 1;
  r.proto = t->proto;
  r.is_ebb = t->is_ebb;
  r.slot = t->slot;
  r.block_no = t->block_no;
  for (int k = 0; k < 32; k++) r.hash[k] = t->hash[k];
  return r;
}
// the tip after `r` was the last header of a call: an unusable header leaves
// a tip nothing links to (proto 0xff; every successor's link bits are clear)
OURO_HD inline void tip_of_rec(ouro_chain_tip* t, const Rec& r) {
  uint8_t* b = reinterpret_cast<uint8_t*>(t);
  for (size_t k = 0; k < sizeof(ouro_chain_tip); k++) b[k] = 0;
  if (r.origin) {
    t->origin = 1;
    return;
  }
  t->proto = r.sliced ? r.proto : 0xff;
  t->is_ebb = r.is_ebb;
  t->slot = r.slot;
  t->block_no = r.block_no;
  for (int k = 0; k < 32; k++) t->hash[k] = r.hash[k];
}

// validateEnvelope of `cur` on top of `prev` (a header's record, a tip's, or
// Origin), as OURO_ENV_* bits -- all four, where the reference stops at the
// first failure.  prev.proto > OURO_PROTO_TPRAOS: an unusable predecessor.
OURO_HD inline uint8_t envelope_link(const Rec& prev, const Rec& cur, const ouro_envelope_cfg& cfg) {
  if (!cur.sliced) return 0;
  uint8_t bits = 0;
  // additionalEnvelopeChecks
  bool extra = true;
  if (cur.proto == OURO_PROTO_PBFT) {
    // Byron/Ledger/HeaderValidation.hs:61-72: an EBB only at an epoch's first slot
    if (cur.is_ebb) extra = cfg.byron_epoch_slots != 0 && cur.slot % cfg.byron_epoch_slots == 0;
  } else if (cfg.has_limits) {
    // ledger-specs chainChecks (Shelley/Ledger/Ledger.hs:395-396)
    extra = cur.limits_ok && cur.header_size <= cfg.max_header_size &&
            cur.body_size <= cfg.max_body_size && cur.prot_major <= cfg.max_major_pv;
  }
  if (extra) bits |= OURO_ENV_EXTRA_OK;
  if (prev.origin) {
    // expectedFirstBlockNo = 0, minimumPossibleSlotNo = 0, Origin <-> GenesisHash
    if (cur.block_no == 0) bits |= OURO_ENV_BLOCKNO_OK;
    bits |= OURO_ENV_SLOT_OK;
    if (cur.prev_kind == kPrevGenesis) bits |= OURO_ENV_PREVHASH_OK;
    return bits;
  }
  if (!prev.sliced || prev.proto > OURO_PROTO_TPRAOS) return bits;
  // Byron/Ledger/HeaderValidation.hs:46-56: an EBB shares its block number
  // with its predecessor and its slot with its successor; everything else,
  // a change of era included (HardFork/Combinator/Block.hs:235-252), is succ
  const bool byron = prev.proto == OURO_PROTO_PBFT && cur.proto == OURO_PROTO_PBFT;
  const bool same_no = byron && !prev.is_ebb && cur.is_ebb;
  const bool same_slot = byron && prev.is_ebb && !cur.is_ebb;
  // (succ of the largest Word64 has no value: nothing is accepted after it)
  if (same_no ? cur.block_no == prev.block_no
              : prev.block_no != ~0ull && cur.block_no == prev.block_no + 1)
    bits |= OURO_ENV_BLOCKNO_OK;
  if (same_slot ? cur.slot >= prev.slot : prev.slot != ~0ull && cur.slot >= prev.slot + 1)
    bits |= OURO_ENV_SLOT_OK;
  if (cur.prev_kind == kPrevBlock) {
    bool eq = true;
    for (int k = 0; k < 32; k++) eq = eq && cur.prev_hash[k] == prev.hash[k];
    if (eq) bits |= OURO_ENV_PREVHASH_OK;
  }
  return bits;
}

}  // namespace env
}  // namespace ouro
