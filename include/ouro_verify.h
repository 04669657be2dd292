/*
 * ouro_verify.h -- C-ABI drop-in boundary of the MI355X (gfx950) batch verifier
 * for the Ouroboros Praos/TPraos header-crypto hot path.
 *
 * The reference (dizgotti/ouroboros-network) reaches this arithmetic through
 * cardano-crypto-class / cardano-crypto-praos, whose Haskell instances bind C
 * symbols with `foreign import ccall`.  Each entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only;
 * no HIP or torch types cross this boundary.
 *
 * Semantics shared by every call:
 *   - Return 0 = valid / OURO_OK, -1 = invalid (single-item calls), or a
 *     negative OURO_E* status for a call that could not run.  A device or
 *     runtime failure NEVER reports "valid" without a verification: a
 *     host-buffer call (single item, ouro_*_batch, header batches, plans)
 *     whose device run fails is recomputed on the library's host path -- the
 *     same lane routines the kernels run, compiled for the CPU -- and returns
 *     OURO_OK with those verdicts (ouro_last_error then says what failed);
 *     with OURO_ON_DEVICE_ERROR=fail in the environment it returns
 *     OURO_EDEVICE instead and leaves the verdicts untouched.  Device-pointer
 *     calls (*_batch_device) cannot be recomputed on the host and return
 *     OURO_EDEVICE.
 *   - Verdict bytes carry several bits: test them with masks, e.g.
 *     (v & OURO_HDR_ALL_OK) == OURO_HDR_ALL_OK, never with equality (a valid
 *     header may also carry OURO_HDR_*_CLAIM_OK or OURO_HDR_*_S_UNREDUCED).
 *   - The caller owns every buffer; nothing is retained after return.
 *   - All calls are thread-safe and reentrant: each calling thread gets its own
 *     HIP stream and staging buffers on the current device, borrowed from a
 *     per-device pool and returned when the thread exits (threads that come
 *     and go reuse them; nothing leaks per thread).
 *   - Byte layouts are the raw encodings of cardano-crypto-class:
 *     VerKeyDSIGN/VerKeyVRF/VerKeyKES 32 B, SigDSIGN 64 B, CertVRF (proof) 80 B,
 *     OutputVRF 64 B, SigKES (Sum6KES Ed25519DSIGN Blake2b_256) 448 B.
 */
#ifndef OURO_VERIFY_H
#define OURO_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OURO_OK 0
#define OURO_INVALID (-1)
#define OURO_EDEVICE (-2) /* HIP/runtime error; nothing was verified      */
#define OURO_EINVAL (-3)  /* bad arguments (NULL with n > 0, sizes, ...)  */
#define OURO_ENODEV (-4)  /* no usable gfx950 device                      */

/* Per-header verdict bits (ouro_tpraos_verify_batch). */
#define OURO_HDR_OCERT_OK 0x01u      /* Ed25519 over OCertSignable            */
#define OURO_HDR_KES_OK 0x02u        /* Sum6KES over the header body          */
#define OURO_HDR_VRF_ETA_OK 0x04u    /* nonce VRF proof                       */
#define OURO_HDR_VRF_LEADER_OK 0x08u /* leader VRF proof                      */
/* The header's claimed certifiedOutput equals the output computed from the
 * proof (set only when the proof verified and the batch carries the claimed
 * outputs).  The reference ("ref2020") accepts on the proof alone and then
 * uses the CLAIMED output downstream: the leader check
 * (ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:484-486,
 * SL.checkLeaderValue (VRF.certifiedOutput certNat)), the nonce update and the
 * chain-selection tiebreak (.../Shelley/Ledger/TPraos.hs:40).  "strict"
 * callers require these bits too (OURO_HDR_STRICT_OK). */
#define OURO_HDR_ETA_CLAIM_OK 0x10u
#define OURO_HDR_LEADER_CLAIM_OK 0x20u
#define OURO_HDR_ALL_OK 0x0fu    /* ref2020: every proof / signature valid    */
#define OURO_HDR_STRICT_OK 0x3fu /* strict: and both claimed outputs correct  */
/* Test verdicts with MASKS, never equality: valid(v) = (v & OURO_HDR_ALL_OK)
 * == OURO_HDR_ALL_OK, strict(v) = (v & OURO_HDR_STRICT_OK) == OURO_HDR_STRICT_OK
 * (a valid header may carry further bits, e.g. OURO_HDR_*_S_UNREDUCED). */
/* The VRF proof's s is NOT below L (set from the proof bytes alone, whatever
 * the verdict).  Draft-03 leaves s's range to the implementation; this
 * library, like the libsodium fork as SURVEY.md App. B.3 recalls it, reduces
 * s mod L and accepts (the default; parity of that choice is unpinned: no
 * reference fixture has s >= L).  A caller that must reject unreduced s
 * ("strict s") requires these bits CLEAR:
 *   valid_strict_s(v) = (v & (OURO_HDR_ALL_OK | OURO_HDR_S_UNREDUCED))
 *                       == OURO_HDR_ALL_OK */
#define OURO_HDR_ETA_S_UNREDUCED 0x40u
#define OURO_HDR_LEADER_S_UNREDUCED 0x80u
#define OURO_HDR_S_UNREDUCED 0xc0u

/* ------------------------------------------------------------------ setup */

/* Select the HIP device used by the calling thread (default: current device).
 * Returns OURO_OK or OURO_ENODEV. */
int ouro_set_device(int device);

/* Human-readable last error of the calling thread ("" if none). */
const char *ouro_last_error(void);

/* ----------------------------------------- single item (ABI-identical) --- */

/* Replaces libsodium 1.0.18 crypto_sign_ed25519_verify_detached, the symbol
 * cardano-crypto-class Ed25519DSIGN.verifyDSIGN binds (callers
 * ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:435 via
 * the OCERT rule, ouroboros-consensus-cardano/src/Ouroboros/Consensus/Cardano/
 * CanHardFork.hs:360).  0 = valid, -1 = invalid, <= -2 = error. */
int ouro_ed25519_verify(const unsigned char *sig, const unsigned char *m,
                        unsigned long long mlen, const unsigned char *pk);

/* Replaces the donna-derived Ed25519 verify of cardano-crypto
 * (cardano_crypto_ed25519_sign_open(m, mlen, pk, sig) [recalled], argument
 * order kept) that ByronDSIGN.verifyDSIGN reaches through verifySignatureRaw
 * (ouroboros-consensus-byron/src/Ouroboros/Consensus/Byron/Crypto/DSIGN.hs:110-113;
 * callers ouroboros-consensus/src/Ouroboros/Consensus/Protocol/PBFT.hs:332 and
 * ouroboros-consensus-byron/src/Ouroboros/Consensus/Byron/Ledger/Integrity.hs:32-35).
 * pk = the first 32 bytes of the 64-byte XPub; m = signTag || signable bytes.
 * Acceptance differs from ouro_ed25519_verify: rejects only
 * sig[63] & 0xE0 and an undecodable A -- no S < L, canonicity or small-order
 * checks.  0 = valid, -1 = invalid, <= -2 = error. */
int ouro_byron_ed25519_verify(const unsigned char *m, size_t mlen, const unsigned char *pk,
                              const unsigned char *sig);

/* Replaces crypto_vrf_ietfdraft03_verify (cardano-crypto-praos, bound by
 * PraosVRF.verifyVRF / verifyCertified; caller: OVERLAY vrfChecks via
 * Shelley/Protocol.hs:435).  On success writes the 64-byte output. */
int ouro_vrf03_verify(unsigned char *output, const unsigned char *pk,
                      const unsigned char *proof, const unsigned char *msg,
                      unsigned long long msglen);

/* Replaces crypto_vrf_ietfdraft03_proof_to_hash (VRF.certifiedOutput,
 * Shelley/Ledger/TPraos.hs:40).  Does not verify the proof. */
int ouro_vrf03_proof_to_hash(unsigned char *output, const unsigned char *proof);

/* Routing of single items.  The single-item calls above run on the library's
 * HOST path (the kernels' own lane routines compiled for the CPU; round 4):
 * one GPU round trip (H2D, one wave, D2H) costs about 220 us for Ed25519 and
 * 420 us for a VRF proof on MI355X, the host path about 1.5x libsodium's
 * ~32 us per Ed25519 on one core (bench.py "single_item" has both routes).
 * OURO_SINGLE_ITEM=gpu in the environment sends them to the device instead.
 * Windows of headers (ChainSync's 64-300, ouro_tpraos_plan_*) and bulk
 * batches (ouro_*_batch) are what the GPU path is for.  The names the
 * reference's Haskell binds are NOT exported by this library; two OPT-IN link
 * shims provide them, with these exact signatures, for a maintainer who
 * wants the drop-in by link order instead of a Haskell edit:
 *   lib/libouro_vrf_shim.so (PraosVRF's foreign imports; the version-less
 *   names are the fork's aliases of draft-03):
 *     int crypto_vrf_ietfdraft03_verify(unsigned char *output, const unsigned char *pk,
 *                                       const unsigned char *proof, const unsigned char *m,
 *                                       unsigned long long mlen);
 *     int crypto_vrf_ietfdraft03_proof_to_hash(unsigned char *output,
 *                                              const unsigned char *proof);
 *     int crypto_vrf_verify(...);         same as crypto_vrf_ietfdraft03_verify
 *     int crypto_vrf_proof_to_hash(...);  same as crypto_vrf_ietfdraft03_proof_to_hash
 *   lib/libouro_sodium_shim.so (Ed25519DSIGN.verifyDSIGN's libsodium symbol):
 *     int crypto_sign_ed25519_verify_detached(const unsigned char *sig,
 *                                             const unsigned char *m,
 *                                             unsigned long long mlen,
 *                                             const unsigned char *pk);
 * Those names follow libsodium's convention (any nonzero = invalid), so a
 * device error must not be passed through: the shims abort with the error on
 * stderr by default, or return -1 with OURO_SHIM_ON_ERROR=invalid. */

/* Replaces SumKES.verifyKES (Sum6KES Ed25519DSIGN Blake2b_256), called via
 * SL.verifySignedKES at ouroboros-consensus-shelley/src/Ouroboros/Consensus/
 * Shelley/Ledger/Integrity.hs:27.  t = KES period relative to the opcert.
 * The reference's Period is a 64-bit Word; every t >= 63 selects leaf 63, so
 * callers saturate larger periods at 2^32 - 1 (kes.py periods_u32). */
int ouro_sum6kes_verify(const unsigned char *vk, unsigned int t, const unsigned char *m,
                        unsigned long long mlen, const unsigned char *sig);

/* --------------------------------------------- batch, host buffers ------ */
/* H2D + kernel + D2H on the calling thread's stream; blocks until done.
 * Messages are addressed by (offset, length) into one buffer.
 * verdict[i] = 1 (valid) / 0 (invalid). */

int ouro_ed25519_verify_batch(size_t n, const uint8_t *pk /* n x 32 */,
                              const uint8_t *sig /* n x 64 */, const uint8_t *msg,
                              const uint64_t *msg_off, const uint32_t *msg_len,
                              uint8_t *verdict);

/* ByronDSIGN acceptance (see ouro_byron_ed25519_verify), pk = XPub[0:32] */
int ouro_byron_ed25519_verify_batch(size_t n, const uint8_t *pk /* n x 32 */,
                                    const uint8_t *sig /* n x 64 */, const uint8_t *msg,
                                    const uint64_t *msg_off, const uint32_t *msg_len,
                                    uint8_t *verdict);

/* beta[i] = 64-byte output on success, zeros otherwise */
int ouro_vrf03_verify_batch(size_t n, const uint8_t *pk /* n x 32 */,
                            const uint8_t *proof /* n x 80 */, const uint8_t *alpha,
                            const uint64_t *alpha_off, const uint32_t *alpha_len,
                            uint8_t *beta /* n x 64 */, uint8_t *verdict);
/* The same with option flags: OURO_VRF_STRICT_S rejects a proof whose s is
 * not below L (verdict 0, beta zeroed) instead of reducing it (the default,
 * see OURO_HDR_S_UNREDUCED). */
#define OURO_VRF_STRICT_S 0x1u
int ouro_vrf03_verify_batch_flags(size_t n, const uint8_t *pk, const uint8_t *proof,
                                  const uint8_t *alpha, const uint64_t *alpha_off,
                                  const uint32_t *alpha_len, uint8_t *beta, uint8_t *verdict,
                                  uint32_t flags);

int ouro_sum6kes_verify_batch(size_t n, const uint8_t *vk /* n x 32 */,
                              const uint32_t *t, const uint8_t *msg, const uint64_t *msg_off,
                              const uint32_t *msg_len, const uint8_t *sig /* n x 448 */,
                              uint8_t *verdict);

/* The crypto subset of SL.updateChainDepState for a batch of TPraos headers,
 * reached in the reference via TPraos.updateChainDepState
 * (ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Protocol.hs:433-442):
 * OCERT (Ed25519 over hotVk || BE64(counter) || BE64(kesPeriod), then Sum6KES
 * over the raw header body) and OVERLAY (the eta and leader VRFs over
 * mkSeed seedEta/seedL slot eta0).  Structure-of-arrays, one entry per header.
 *
 * The first 16 members are required (eta_alpha / leader_alpha only when
 * `slot` is NULL).  The last five are optional -- NULL = not used; a caller
 * that zero-initialises the struct gets the round-1 behaviour:
 *   eta_output / leader_output: the header's claimed certifiedOutputs (the
 *     first element of bheaderEta / bheaderL); enables the *_CLAIM_OK bits.
 *   slot + epoch_nonce: the VRF inputs are derived on the device exactly as
 *     the OVERLAY rule does (Shelley/Protocol.hs:409-410, ledger-specs mkSeed):
 *       alpha = Blake2b-256(BE64(slot) || eta0) XOR seed,
 *       seedEta = Blake2b-256(BE64(0)), seedL = Blake2b-256(BE64(1))
 *     (mkNonceFromNumber 0 / 1); epoch_nonce = NULL is NeutralNonce (nothing
 *     appended after the slot).  eta_alpha / leader_alpha are then ignored.
 *     These single-nonce members serve ONE epoch: every header of the call
 *     is seeded with the same eta0.  A batch that crosses an epoch boundary
 *     goes to ouro_tpraos_verify_batch_epochs (below) with an epoch-nonce
 *     schedule, a raw stream to ouro_chain_verify_cbor; neither is split.
 *   eta_nonce (OUTPUT, n x 32): mkNonceFromOutputVRF of the eta output the
 *     nonce update consumes = Blake2b-256(claimed eta output) when
 *     eta_output is given (the reference's choice), else of the computed
 *     beta_eta.  ouro_nonce_fold folds these into eta_v / eta_c.
 *
 * Shared OCERT checks (deployment knob OURO_OCERT_SHARE, default 1): an
 * operational certificate is issued once per KES key rotation, so the headers
 * of a bulk batch carry a handful of distinct ones per pool.  Every GPU header
 * batch (host buffers, device buffers, raw CBOR) groups its headers by the 144
 * bytes issuer_vk || hot_vk || ocert_counter || ocert_kes_period ||
 * ocert_sigma -- equality over all of them, never a hash alone -- and runs the
 * Ed25519 check once per distinct record; the verdict bits are the ones a
 * check per header gives (Ed25519 verification is a pure function of key,
 * message and signature).  The verdict of each distinct record is kept per
 * stream for the next calls (OURO_KEY_CACHE, below), so a call verifies only
 * the records its stream has not seen.  A batch of mostly distinct certificates
 * (more than 7/8 of n) runs the check per header as before and keeps nothing.  OURO_OCERT_SHARE=0 in
 * the environment turns the sharing off.  The latency plans and the host path
 * never share.
 * Footprint: the workspace belongs to the calling thread's pooled context, is
 * kept per stream for its next call and grows with the largest batch seen:
 * 4 x (the next power of two >= 2n) + 9n bytes, about 17 MB at 1M headers and
 * 1.1 MB per 65,536-header chunk of the pipelined paths; and the certificate
 * directory, 157 bytes per certificate for as many as the largest batch had
 * headers, 65,536 at the most (10 MB).
 *
 * Shared VRF key tables (deployment knob OURO_VRFKEY_SHARE, default 1): a
 * pool's VRF key is the same 32 bytes in every header it forges.  The same
 * GPU header batches group their headers by vrf_vk -- equality over all 32
 * bytes -- run the key checks once per distinct key, build a fixed-base table
 * of -Y for it, and compute both U = [s]B - [c]Y of every header from that
 * table by additions alone.  U is a group element determined by (Y, c, s) and
 * its encoding is canonical, so verdicts and outputs are bit for bit those of
 * the per-header chains.  A key's table is built by the first call on a
 * stream that carries the key and kept for that stream's next calls
 * (OURO_KEY_CACHE, below).  A batch with fewer than 16
 * headers per distinct key, or with more distinct keys than the table budget
 * holds, runs the per-header chains as before.  OURO_VRFKEY_SHARE=0 turns the
 * sharing off.  The latency plans, the host path and the standalone VRF entry
 * never share.
 * Footprint: per stream of the calling thread's pooled context, kept for its
 * next call: the grouping buffer, 4 x (the next power of two >= 2n) + 12n
 * bytes (about 21 MB at 1M headers), and the tables, 90,752 bytes per key for
 * min(n / 16, budget) keys -- at most OURO_VRFKEY_TAB_MB megabytes (default
 * 512: 5,900 keys; a 65,536-header chunk of the pipelined paths sizes for
 * 4,096 keys, 372 MB per slot in flight).  Lower the budget to trade memory
 * for speed; a batch whose keys do not fit loses nothing but the saving.  The
 * tables' directory adds under 60 bytes per key.
 *
 * Kept between calls (deployment knob OURO_KEY_CACHE, default 1): a pool's VRF
 * key lasts for the life of the pool and its certificate for months, so the
 * two workspaces above keep, per stream, a directory of the keys seen: VRF key
 * -> table and flag, certificate record -> verdict.  A call looks its headers
 * up first -- the full key bytes are compared, a hash only picks where to look
 * -- and builds or verifies only what is new.  Whether a call shares is still
 * decided by the distinct keys of its own batch.  Nothing is shared between
 * streams, threads or devices, and every access is ordered by the stream.  A
 * directory is emptied when its workspace has to grow, when
 * ouro_debug_reload_knobs() is called, and -- inside the call, with the same
 * results -- when a batch's new keys do not fit beside the ones it holds.
 * OURO_KEY_CACHE=0 empties both at every call: the behaviour before there was
 * anything kept, for an A/B in one process. */
typedef struct ouro_tpraos_batch {
  size_t n;
  const uint8_t *issuer_vk;        /* n x 32  bheaderVk (cold key)            */
  const uint8_t *vrf_vk;           /* n x 32  bheaderVrfVk                    */
  const uint8_t *eta_proof;        /* n x 80  bheaderEta proof                */
  const uint8_t *leader_proof;     /* n x 80  bheaderL proof                  */
  const uint8_t *eta_alpha;        /* n x 32  mkSeed seedEta slot eta0        */
  const uint8_t *leader_alpha;     /* n x 32  mkSeed seedL   slot eta0        */
  const uint8_t *hot_vk;           /* n x 32  ocertVkHot (Sum6KES root)       */
  const uint64_t *ocert_counter;   /* n       ocertN                          */
  const uint64_t *ocert_kes_period;/* n       ocertKESPeriod (c0)             */
  const uint8_t *ocert_sigma;      /* n x 64  ocertSigma                      */
  const uint32_t *kes_t;           /* n       kesPeriod(slot) - c0, clamped   */
  const uint8_t *kes_sig;          /* n x 448 header KES signature            */
  const uint8_t *body;             /* concatenated raw header-body CBOR       */
  const uint64_t *body_off;        /* n                                       */
  const uint32_t *body_len;        /* n                                       */
  /* optional (NULL = not used) */
  const uint8_t *eta_output;       /* n x 64  claimed certifiedOutput (eta)   */
  const uint8_t *leader_output;    /* n x 64  claimed certifiedOutput (leader)*/
  const uint64_t *slot;            /* n       bheaderSlotNo: seeds on device  */
  const uint8_t *epoch_nonce;      /* 32      eta0 (NULL: NeutralNonce)       */
  uint8_t *eta_nonce;              /* n x 32  OUT: Blake2b-256(eta output)    */
} ouro_tpraos_batch;

/* verdict[i] = OURO_HDR_* bits; beta_eta / beta_leader (n x 64, may be NULL)
 * receive the computed VRF outputs (zeros where a proof fails). */
int ouro_tpraos_verify_batch(const ouro_tpraos_batch *b, uint8_t *verdict,
                             uint8_t *beta_eta, uint8_t *beta_leader);

/* An epoch-nonce schedule: which eta0 seeds the VRF inputs of which slots, so
 * that one call verifies a batch spanning several epochs (ChainDB's
 * re-validation of a stored suffix, ouroboros-consensus/src/Ouroboros/
 * Consensus/Storage/ChainDB/Impl/LgrDB.hs:350-368, ImmutableDB / VolatileDB
 * replay, a ChainSync window across a boundary).  Entry j applies to
 * first_slot[j] <= slot < first_slot[j + 1], the last entry to every slot from
 * its first_slot up.  first_slot[0] must be 0, so every slot has an entry (a
 * caller with nothing to say about early -- Byron -- slots puts any row
 * there).  The kernels find a header's entry by binary search on its slot, at
 * most 12 steps, inside the out-of-line mkSeed routine; the schedule is
 * uploaded with the call (with each chunk of a pipelined call; 41 bytes per
 * entry, about 170 KB at the cap) and nothing of it is kept afterwards.
 * OURO_EINVAL before anything runs: k outside 1 .. OURO_EPOCHS_MAX,
 * first_slot[0] != 0, first_slot not strictly increasing, first_slot or nonce
 * NULL.  The schedule is an INPUT: computing the next epoch's nonce (TICKN)
 * stays with the caller (ouro_nonce_fold is the tool). */
#define OURO_EPOCHS_MAX 4096
typedef struct ouro_epoch_nonces {
  size_t k;                   /* 1 .. OURO_EPOCHS_MAX entries                      */
  const uint64_t *first_slot; /* k, strictly increasing, first_slot[0] == 0        */
  const uint8_t *nonce;       /* k x 32: eta0 of entry j                           */
  const uint8_t *neutral;     /* k, may be NULL: 1 = NeutralNonce (row j ignored)  */
} ouro_epoch_nonces;
/* ouro_tpraos_verify_batch with mkSeed under the schedule: b->slot is
 * required; b->epoch_nonce, b->eta_alpha and b->leader_alpha must be NULL
 * (OURO_EINVAL otherwise).  Everything else -- OCERT sharing, the claimed
 * outputs, eta_nonce, the host-path recompute after a device error -- is as
 * ouro_tpraos_verify_batch; a one-entry schedule gives byte-identical results
 * to that call with the entry's nonce as epoch_nonce (NULL for a neutral
 * entry).  _host (declared with the host path below) is the same on the CPU.
 * Out of scope: the latency plans (ouro_tpraos_plan_*, _lowlat) still take one
 * eta0 -- a window through a plan is split at an epoch boundary -- and there
 * is no device-pointer form. */
int ouro_tpraos_verify_batch_epochs(const ouro_tpraos_batch *b, const ouro_epoch_nonces *e,
                                    uint8_t *verdict, uint8_t *beta_eta, uint8_t *beta_leader);

/* Raw header CBOR -> the SoA above.  Replaces the
 * per-header decode the reference runs on every header ChainSync receives
 * (ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Ledger/Block.hs:216-217,
 * the Annotator keeping the raw header_body bytes; N2N wrapping at
 * .../Shelley/Node/Serialisation.hs:88-90) with one host call per batch.
 * Header i is raw[off[i] .. off[i] + len[i]) as it came off the wire:
 *   #6.24(bytes .cbor [header_body, kes_sig])             (N2N v1), or
 *   [era, #6.24(bytes .cbor [header_body, kes_sig])]      (Cardano HFC, era >= 1)
 * header_body = [blockNo, slot, prevHash, issuerVk, vrfVk, [etaOut, etaProof],
 * [leaderOut, leaderProof], bodySize, bodyHash, hotVk, counter, kesPeriod,
 * sigma, protMajor, protMinor] (ouroboros-network/test/messages.cddl:27-34).
 * The fixed-size fields are copied into `arena` (ouro_tpraos_pack_bytes(n)
 * bytes, any alignment) and *out's required members and eta_output /
 * leader_output (the claimed outputs) are pointed at them; body = raw and
 * body_off / body_len are the header_body spans inside raw (the KES message,
 * not copied); kes_t = kesPeriod(slot) - kesPeriod, clamped at 0 and saturated
 * at 2^32 - 1 (Integrity.hs:38-44).  eta_alpha / leader_alpha / slot /
 * epoch_nonce / eta_nonce are left to the caller (set out->slot = slot and
 * epoch_nonce to have the device derive the VRF inputs).  slot / era (n
 * each, may be NULL) receive bheaderSlotNo and the HFC era (1 if unwrapped).
 * status[i] = OURO_PACK_*; a rejected header's rows are zero (every verdict
 * bit then fails).  nthreads <= 0: one per hardware thread (at least 4096
 * headers each).  Host-only.  Returns OURO_OK, or OURO_EINVAL for bad
 * arguments (a span outside raw_bytes, a short arena, NULLs). */
#define OURO_PACK_OK 0u
#define OURO_PACK_ECBOR 1u  /* malformed or truncated CBOR                    */
#define OURO_PACK_ESHAPE 2u /* not the header shape (tag 24, [body, sig], 15
                               fields, [output, proof] certs, uint/bytes types) */
#define OURO_PACK_ESIZE 3u  /* a fixed-size crypto field has the wrong length  */
#define OURO_PACK_EBYRON 4u /* HFC era 0: a Byron header, not TPraos          */
#define OURO_PACK_ESPAN 5u  /* (device slicer) span outside raw_bytes          */
#define OURO_PACK_EBB 6u    /* (Byron slicers) an epoch-boundary header: PBFT
                               checks no signature on it (PBFT.hs:327-328);
                               an epoch-boundary block (HFC block tag 0)       */
#define OURO_PACK_ESHELLEY 7u /* (Byron slicers) HFC era >= 1: not a Byron header;
                                 HFC block tag >= 2: not a Byron block          */
#define OURO_PACK_ECAP 8u   /* (witness slicer, Byron block _device entry) the
                               block's rows pass a capacity                    */
size_t ouro_tpraos_pack_bytes(size_t n);
int ouro_tpraos_pack_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                          const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                          void *arena, size_t arena_bytes, ouro_tpraos_batch *out,
                          uint64_t *slot, uint8_t *era, uint8_t *status, int nthreads);
/* The same slicer on the GPU, one lane per header, for raw headers already in
 * device memory (raw, off, len, arena, slot, era, status: device pointers;
 * slot / era may be NULL): enqueued on `stream` and returns at once; *out
 * receives device pointers into the arena, ready for
 * ouro_tpraos_verify_batch_device on the same stream.  A span outside
 * raw_bytes is per-header status OURO_PACK_ESPAN.  Same parse code as the
 * host slicer (csrc/cbor.h); tests/test_gpu_pack.py checks the two agree. */
int ouro_tpraos_pack_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                 const uint64_t *off, const uint32_t *len, size_t n,
                                 uint64_t slots_per_kes_period, void *arena, size_t arena_bytes,
                                 ouro_tpraos_batch *out, uint64_t *slot, uint8_t *era,
                                 uint8_t *status);

/* Storage integrity, KES only, straight from raw header CBOR: replaces
 * verifyHeaderIntegrity (ouroboros-consensus-shelley/src/Ouroboros/Consensus/
 * Shelley/Ledger/Integrity.hs:20-44) as the storage layer runs it on every
 * block -- the VolatileDB parser at open
 * (ouroboros-consensus/src/Ouroboros/Consensus/Storage/VolatileDB/Impl/Parser.hs:66-85)
 * and ImmutableDB chunk validation
 * (.../Storage/ImmutableDB/Impl/Validation.hs:358-365).  Headers as for
 * ouro_tpraos_pack_cbor; verdict[i] = 1 iff header i slices (status
 * OURO_PACK_OK) and its Sum6KES signature verifies over the raw header body
 * under the opcert's hot key at t = kesPeriod(slot) - c0 (0 when the slot's
 * period is below c0; Integrity.hs:38-44).  Host buffers (pageable is fine),
 * synchronous; runs on the raw-CBOR pipeline described at
 * ouro_tpraos_verify_cbor (a device error recomputes on the host path).
 * OURO_EINVAL for a span outside raw_bytes, NULLs or a zero period. */
int ouro_integrity_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                               const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                               uint8_t *status, uint8_t *verdict);
/* Raw TPraos headers in host memory -> the full header check in ONE call:
 * the crypto of TPraos.updateChainDepState (ouroboros-consensus-shelley/src/
 * Ouroboros/Consensus/Shelley/Protocol.hs:433-442) over every header of a
 * batch the caller holds as the raw bytes it received or stored -- ChainSync
 * windows (ouroboros-consensus/src/Ouroboros/Consensus/MiniProtocol/ChainSync/
 * Client.hs:792) and ChainDB's re-validation of a stored chain suffix
 * (.../Storage/ChainDB/Impl/LgrDB.hs:350-368).  Headers as for
 * ouro_tpraos_pack_cbor (raw may be pageable, any offsets and order).
 * VRF inputs: eta_alpha / leader_alpha (n x 32 each) when both are given,
 * otherwise derived on the device from each header's slot as the OVERLAY rule
 * does (mkSeed seedEta / seedL slot eta0, see ouro_tpraos_batch), with
 * epoch_nonce = eta0 (32 B; NULL = NeutralNonce; one eta0 per call: a stream
 * over several epochs goes to ouro_chain_verify_cbor with a schedule).  The
 * headers' claimed certifiedOutputs are compared (OURO_HDR_*_CLAIM_OK).
 * Outputs: status[i] = OURO_PACK_*; verdict[i] = OURO_HDR_* bits, 0 for a
 * header that does not slice; beta_eta / beta_leader (n x 64) and eta_nonce
 * (n x 32, Blake2b-256 of the claimed eta output) may be NULL.
 * How it runs: the batch is cut into chunks of whole headers; the library's
 * worker pool gathers each chunk's spans into pinned, NUMA-local staging,
 * and per chunk one stream uploads the raw bytes, runs the device slicer
 * and the header kernel and copies the results back, several chunks in
 * flight so the host copies and PCIe hide behind the kernels
 * (OURO_CBOR_CHUNK headers per chunk, default 65536; OURO_CBOR_SLOTS chunks
 * in flight, default 6 -- 4 for ouro_integrity_verify_cbor --, at most 8;
 * OURO_CBOR_COPY_THREADS gather threads, default 8).  Synchronous; a device error recomputes the batch on the host
 * path.  OURO_EINVAL for a span outside raw_bytes, NULLs, a zero period or
 * only one of the two alpha arrays.
 * Footprint: the pipeline's buffers belong to the calling
 * thread's pooled context and are kept for its next call -- per slot pinned
 * staging of ~1.125 x the chunk's raw bytes, device buffers for the raw
 * bytes, the slicer's arena and the results, and the kernel's scratch; at the
 * default 65,536-header chunk of ~1 KB headers about 75 MB pinned and 180 MB
 * of device memory per slot in use (6 slots for headers, 4 for integrity),
 * once per context that has made such a call.  OURO_CBOR_CHUNK and
 * OURO_CBOR_SLOTS shrink it. */
int ouro_tpraos_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                            const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                            const uint8_t *epoch_nonce, const uint8_t *eta_alpha,
                            const uint8_t *leader_alpha, uint8_t *status, uint8_t *verdict,
                            uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce);
/* The same on raw headers already in device memory (device pointers; arena
 * of ouro_tpraos_pack_bytes(n) bytes): the device slicer and the Sum6KES
 * kernel enqueued on `stream`, not synchronised.  A rejected header's row is
 * zeroed by the slicer, so its verdict is 0. */
int ouro_integrity_verify_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                      const uint64_t *off, const uint32_t *len, size_t n,
                                      uint64_t slots_per_kes_period, void *arena,
                                      size_t arena_bytes, uint8_t *status, uint8_t *verdict);

/* Batched Blake2b-256 (RFC 7693, unkeyed, 32-byte digest) over arbitrary
 * spans: out[i] = Blake2b-256(msg[off[i] .. off[i] + len[i])), spans of any
 * length up to 2^32 - 1, any byte alignment, overlapping or identical spans
 * allowed.  The hash of the reference's HASH Blake2b_256: the block body hash
 * below (ledger-specs bbHash behind blockMatchesHeader,
 * ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/Ledger/Block.hs:127-130),
 * and header / prev hashes (ShelleyHash, .../Shelley/Ledger/Block.hs:63).
 * One lane per message on the device, the messages ordered by length class
 * (the bit length of their compression count) so that a wave's lanes run
 * alike; OURO_BLOCK_SORT=0 turns the ordering off (A/B).
 *   ouro_blake2b256_batch: host buffers; one upload, launch and copy-back on
 *     the calling thread's stream, synchronous; a device error recomputes on
 *     the host path.
 *   ouro_blake2b256_batch_host: the host path alone (the same lane routine
 *     compiled for the host, split over the worker pool).
 *   Both return OURO_EINVAL, before any work, for NULLs or a span outside
 *   msg_bytes.
 *   ouro_blake2b256_batch_device: device pointers, enqueued on `stream`, not
 *     synchronised.  A lane reads the aligned dwords its span touches and
 *     no other, so msg must be 4-byte aligned and its allocation must extend
 *     to the next multiple of 4 above msg_bytes (the dword holding the last
 *     byte is read whole; hipMalloc'd buffers always do).  out must be
 *     16-byte aligned; work: ouro_blake2b256_work_bytes(n) bytes of device
 *     memory.  A
 *     span outside msg_bytes is not read; its digest is 32 zero bytes. */
int ouro_blake2b256_batch(size_t n, const uint8_t *msg, size_t msg_bytes, const uint64_t *off,
                          const uint32_t *len, uint8_t *out);
int ouro_blake2b256_batch_host(size_t n, const uint8_t *msg, size_t msg_bytes,
                               const uint64_t *off, const uint32_t *len, uint8_t *out);
size_t ouro_blake2b256_work_bytes(size_t n);
int ouro_blake2b256_batch_device(void *stream, size_t n, const uint8_t *msg, size_t msg_bytes,
                                 const uint64_t *off, const uint32_t *len, uint8_t *out,
                                 void *work, size_t work_bytes);

/* Whole-block storage integrity straight from raw block CBOR: replaces
 * verifyBlockIntegrity (ouroboros-consensus-shelley/src/Ouroboros/Consensus/
 * Shelley/Ledger/Integrity.hs:45-51) = verifyHeaderIntegrity hdr &&
 * blockMatchesHeader hdr blk, as the storage layer runs it on every block --
 * the VolatileDB parser (ouroboros-consensus/src/Ouroboros/Consensus/Storage/
 * VolatileDB/Impl/Parser.hs:66-85), ImmutableDB chunk validation
 * (.../ImmutableDB/Impl/Validation.hs:358-365) and GetVerifiedBlock -- and
 * blockMatchesHeader alone as the BlockFetch client runs it on every block it
 * downloads (ouroboros-network/src/Ouroboros/Network/BlockFetch/Client.hs:280).
 * Block i is raw[off[i] .. off[i] + len[i]) in any of the forms
 *   [header, txBodies, txWitnesses, txMetadata]             Shelley on disk
 *   #6.24(bytes .cbor block)                                Shelley on the wire
 *   [tag, block]                                            Cardano on disk
 *   #6.24(bytes .cbor [tag, block])                         Cardano on the wire
 * with header = [header_body, kes_sig] (plain, not tag-24 wrapped).  The HFC
 * block tag is 0 = Byron EBB, 1 = Byron regular (both status OURO_PACK_EBYRON:
 * Byron's body proof is out of scope), 2 and up = Shelley family.  The block
 * must be a definite array(4) that ends exactly where its span (the tag-24
 * payload) ends.  blockMatchesHeader (.../Shelley/Ledger/Block.hs:127-130):
 *   bbHash = Blake2b-256(Blake2b-256(txBodies) || Blake2b-256(txWitnesses)
 *                        || Blake2b-256(txMetadata))  ==  header_body field 8
 * each inner hash over the item's bytes exactly as they stand in the block.
 * Outputs: status[i] = OURO_PACK_*; verdict[i] = OURO_BLK_* bits, 0 for a
 * block that does not slice; body_hash (n x 32, may be NULL) the computed
 * bbHash, zeros for a block that does not slice.
 *   ouro_block_integrity_verify_cbor: host buffers (pageable is fine),
 *     synchronous, on the raw-CBOR pipeline described at
 *     ouro_tpraos_verify_cbor: chunks of whole blocks gathered into pinned
 *     staging, uploaded once; slicer, segment hashes, Sum6KES and finish on
 *     the slot's stream; 4 chunks in flight; a device error recomputes the
 *     batch on the host path.
 *   ouro_block_integrity_verify_cbor_host: the host path alone.
 *   Both return OURO_EINVAL, before any work, for a span outside raw_bytes,
 *   NULLs or a zero period.
 *   ouro_block_integrity_verify_cbor_device: device pointers (raw 4-byte
 *     aligned and allocated up to the next multiple of 4 above raw_bytes,
 *     see ouro_blake2b256_batch_device; arena of
 *     ouro_block_pack_bytes(n) bytes), enqueued on `stream`, not synchronised;
 *     a span outside raw_bytes is per-block status OURO_PACK_ESPAN.
 * Out of scope: _multi forms, the latency plans.  Byron blocks (their body
 * proof and block signature): ouro_byron_block_integrity_verify_cbor below. */
#define OURO_BLK_KES_OK 0x01u  /* verifyHeaderIntegrity                       */
#define OURO_BLK_BODY_OK 0x02u /* blockMatchesHeader: bbHash == bodyHash      */
#define OURO_BLK_ALL_OK 0x03u  /* verifyBlockIntegrity; test with the mask    */
size_t ouro_block_pack_bytes(size_t n);
int ouro_block_integrity_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                     const uint32_t *len, size_t n,
                                     uint64_t slots_per_kes_period, uint8_t *status,
                                     uint8_t *verdict, uint8_t *body_hash);
int ouro_block_integrity_verify_cbor_host(const uint8_t *raw, size_t raw_bytes,
                                          const uint64_t *off, const uint32_t *len, size_t n,
                                          uint64_t slots_per_kes_period, uint8_t *status,
                                          uint8_t *verdict, uint8_t *body_hash);
int ouro_block_integrity_verify_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                            const uint64_t *off, const uint32_t *len, size_t n,
                                            uint64_t slots_per_kes_period, void *arena,
                                            size_t arena_bytes, uint8_t *status, uint8_t *verdict,
                                            uint8_t *body_hash);

/* Transaction key witnesses straight from raw block CBOR: the Ed25519
 * verification of every transaction's key witnesses over its transaction id,
 * the crypto call of ledger-specs' UTXOW rule (verifiedWits), and the largest
 * one of a ChainDB replay.  Block i is raw[off[i] .. off[i] + len[i]) in any of
 * the four forms of ouro_block_integrity_verify_cbor; Byron blocks are status
 * OURO_PACK_EBYRON.  The block must be a definite array(4) that ends exactly at
 * its span.  Item 0 (the header) and item 3 (the metadata) are skipped, not
 * examined: ouro_block_integrity_verify_cbor checks the header.
 *   txBodies    = [* map], definite or indefinite; tx id = Blake2b-256 of the
 *                 element's bytes as they stand in the block
 *   txWitnesses = [* {uint => any}], as many elements as bodies; of each map
 *     key 0: [* [vkey: bytes(32), sig: bytes(64)]]
 *     key 2: [* [vkey: bytes(32), sig: bytes(64), chain_code: bytes(32),
 *                attributes]]   (bootstrap: its address check needs ledger
 *                                state and is out of scope)
 *     any other key: skipped; a repeated key is walked again.
 * Witnesses are numbered in the order the walk meets them; each one's message
 * is its transaction's 32-byte id, verified as plain Ed25519 with libsodium
 * 1.0.18's rules (both kinds).  Rows: block i owns the tx rows
 * [tx_begin[i], tx_begin[i + 1]) and the witness rows [wit_begin[i],
 * wit_begin[i + 1]); a block that does not slice owns none.  A sliced block
 * whose rows would pass a capacity (tx_begin[i] + ntx > tx_cap, or the same
 * for witnesses) writes nothing and has status OURO_PACK_ECAP; the blocks
 * that fit -- always a prefix of the sliced ones -- are processed in full,
 * and tx_begin[n] / wit_begin[n] are the totals whether they fit or not.
 * Outputs: status[i] = OURO_PACK_*; n_bad[i] = the block's witnesses that do
 * not verify; verdict[i] = OURO_WIT_ALL_OK iff the block sliced, fit, and
 * n_bad[i] == 0 (so also for a block without witnesses), else 0.
 *   ouro_block_witness_count_cbor[_host]: the slicer's count pass alone:
 *     status, ntx[i] and nwit[i] (zeros where the block does not slice) -- what
 *     a caller sizes the capacities from.
 *   ouro_block_witness_verify_cbor: host buffers, synchronous, on the calling
 *     thread's stream, in consecutive groups of whole blocks under a byte
 *     budget (OURO_WITNESS_GROUP_BYTES); a device error recomputes the call on
 *     the host path.  Rows past the blocks that fit are left untouched.
 *   ouro_block_witness_verify_cbor_host: the host path alone.
 *   All four return OURO_EINVAL, before any work, for NULLs or a span outside
 *   raw_bytes.
 *   ouro_block_witness_verify_cbor_device: device pointers (raw as for
 *     ouro_blake2b256_batch_device; tx_begin / wit_begin 8-byte, tx_id and
 *     wit_vk 16-byte, wit_tx 4-byte aligned; work of
 *     ouro_block_witness_work_bytes(n, tx_cap, wit_cap) bytes), enqueued on
 *     `stream`, not synchronised, no host round trip between slicing and
 *     verifying; a span outside raw_bytes is per-block status OURO_PACK_ESPAN;
 *     rows past the blocks that fit are zero.
 * Out of scope: the bootstrap address check and every other UTXOW rule, _multi
 * forms, the chunked raw pipeline.  Byron blocks' witnesses:
 * ouro_byron_block_witness_verify_cbor below. */
#define OURO_WIT_ALL_OK 0x01u
typedef struct {
  size_t tx_cap, wit_cap;
  uint64_t *tx_begin, *wit_begin; /* n + 1 each; [n] = totals, also when they pass the caps */
  uint8_t *tx_id;                 /* tx_cap x 32 */
  uint32_t *wit_tx;               /* wit_cap: global tx row */
  uint8_t *wit_kind, *wit_ok;     /* wit_cap each: 0 or 2; 1 = verifies */
  uint8_t *wit_vk;                /* wit_cap x 32, may be NULL */
} ouro_block_witness_out;
int ouro_block_witness_count_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                  const uint32_t *len, size_t n, uint8_t *status, uint32_t *ntx,
                                  uint32_t *nwit);
int ouro_block_witness_count_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                       const uint32_t *len, size_t n, uint8_t *status,
                                       uint32_t *ntx, uint32_t *nwit);
int ouro_block_witness_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                   const uint32_t *len, size_t n,
                                   const ouro_block_witness_out *out, uint8_t *status,
                                   uint8_t *verdict, uint32_t *n_bad);
int ouro_block_witness_verify_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                        const uint32_t *len, size_t n,
                                        const ouro_block_witness_out *out, uint8_t *status,
                                        uint8_t *verdict, uint32_t *n_bad);
size_t ouro_block_witness_work_bytes(size_t n, size_t tx_cap, size_t wit_cap);
int ouro_block_witness_verify_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                          const uint64_t *off, const uint32_t *len, size_t n,
                                          const ouro_block_witness_out *out, void *work,
                                          size_t work_bytes, uint8_t *status, uint8_t *verdict,
                                          uint32_t *n_bad);

/* Raw Byron header CBOR -> the inputs of its PBFT block-signature check
 * (SURVEY.md §8(f) row 4).  Replaces the per-header decode + message assembly
 * in front of ByronDSIGN.verifyDSIGN: Byron/Ledger/PBFT.hs:47-73 builds
 * PBftFields and recoverSignedBytes from the decoded header, PBFT.hs:332-337
 * verifies them (caller: ChainSync's validateHeader; Integrity.hs:32-35 from
 * storage).  Header i is raw[off[i] .. off[i] + len[i]) in any of the forms
 * the reference sends (Byron/Node/Serialisation.hs:87-101, 197-210):
 *   #6.24(bytes .cbor [kind, header])                      Byron / Cardano N2N v1
 *   [[kind, size], #6.24(bytes .cbor header)]              Byron N2N v2
 *   [0, [[kind, size], #6.24(bytes .cbor header)]]         Cardano N2N v2+
 * kind 1 = regular, 0 = epoch boundary (status OURO_PACK_EBB: no signature,
 * fields unchecked).  For a regular header the batch receives pk =
 * delegateXPub[0:32] (pbftIssuer), sig, genesis_vk = the delegation
 * certificate's issuer XPub (pbftGenKey), delegate_vk, the header's
 * protocol magic, and the signed message
 *   "01" || genesis_vk || 0x09 || CBOR(magic) || 0x85 || prevHash || bodyProof
 *   || slotId || difficulty || extraData                    (raw field bytes)
 * at msg + msg_off[i] (msg_len[i] bytes), magic = protocol_magic (the node's
 * ProtocolMagicId, mkByronContextDSIGN at Byron/Ledger/PBFT.hs:43-44) or,
 * for protocol_magic = -1, each header's own field.  The arena holds all of
 * it: ouro_byron_pack_bytes(n, len) bytes, any alignment.  status[i] =
 * OURO_PACK_* (OK, ECBOR, ESHAPE, ESIZE, EBB, ESHELLEY); rows of other
 * statuses are zero with msg_len 0.  nthreads as for ouro_tpraos_pack_cbor.
 * Host-only.  OURO_EINVAL for a span outside raw_bytes, a short arena, a
 * protocol_magic outside -1 .. 2^32 - 1, NULLs. */
typedef struct {
  size_t n;
  const uint8_t *pk;          /* n x 32  delegate XPub[0:32]                  */
  const uint8_t *sig;         /* n x 64  block signature                      */
  const uint8_t *msg;         /* signed messages                              */
  const uint64_t *msg_off;    /* n       offsets into msg                     */
  const uint32_t *msg_len;    /* n                                            */
  const uint8_t *genesis_vk;  /* n x 64  delegation certificate issuer XPub   */
  const uint8_t *delegate_vk; /* n x 64  delegate XPub                        */
  const uint64_t *magic;      /* n       the header's protocolMagic field     */
} ouro_byron_batch;
size_t ouro_byron_pack_bytes(size_t n, const uint32_t *len);
int ouro_byron_pack_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                         const uint32_t *len, size_t n, int64_t protocol_magic, void *arena,
                         size_t arena_bytes, ouro_byron_batch *out, uint8_t *status,
                         int nthreads);
/* Raw Byron headers -> verdicts in one call: ouro_byron_pack_cbor, then the
 * ByronDSIGN batch verify of the packed rows on the calling thread's stream.
 * verdict[i] = 1 for a regular header whose block signature verifies and for
 * an epoch-boundary header (PBftValidateBoundary checks nothing), else 0;
 * status[i] as above.  The delegation lookup, the slot check and the
 * signing-window threshold (PBFT.hs:340-357) are not part of this call:
 * ouro_pbft_ledger_checks below evaluates them over the sliced rows
 * (ouro_byron_pack_cbor's delegate_vk and status, and the slots). */
int ouro_byron_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                           const uint32_t *len, size_t n, int64_t protocol_magic,
                           uint8_t *status, uint8_t *verdict);
/* Byron whole-block storage integrity straight from raw block CBOR: replaces
 * verifyBlockIntegrity cfg blk = verifyHeaderIntegrity cfg hdr &&
 * blockMatchesHeader hdr blk (ouroboros-consensus-byron/src/Ouroboros/
 * Consensus/Byron/Ledger/Integrity.hs:63-68) for the callers listed at
 * ouro_block_integrity_verify_cbor, over the Byron prefix of a Cardano chain.
 * Block i is raw[off[i] .. off[i] + len[i]) in either form
 *   [tag, block]                        on disk (Byron-only and Cardano alike)
 *   #6.24(bytes .cbor [tag, block])     on the wire
 * tag 0 = EBB (status OURO_PACK_EBB, verdict OURO_BYB_ALL_OK, zero tx_root: the
 * reference checks nothing of an EBB; it must end where its span ends), 1 =
 * regular, 2 and up = Shelley family (OURO_PACK_ESHELLEY, verdict 0).
 *   regular = [header, body, extra]           a definite array(3), ending at its span
 *   header  = [magic, prevHash, proof, consensusData, extraData], as
 *             ouro_byron_pack_cbor reads it after unwrapping
 *   proof   = [[txpNumber, txpRoot, txpWitnessesHash], [sscTag, sscHash],
 *              dlgHash, updHash]
 *   body    = [txPayload, sscPayload, dlgPayload, updPayload]   definite array(4)
 *   txPayload = [* [tx, witnesses]]   definite or indefinite; each element a
 *               definite array(2) of two arrays, recorded as they stand
 * verifyHeaderIntegrity (OURO_BYB_HDR_OK): the block signature under ByronDSIGN
 * over the message of ouro_byron_pack_cbor built with protocol_magic, and the
 * header's own magic field == protocol_magic (Integrity.hs:46-56);
 * protocol_magic = -1: each header's own field for both.
 * blockMatchesHeader (OURO_BYB_BODY_OK; CC.abobMatchesBody, Byron/Ledger/
 * Block.hs:167-168) = the five bits below, every hash Blake2b-256 over bytes as
 * they stand in the block:
 *   TXNUM   txpNumber == the number n of transactions
 *   TXROOT  txpRoot == the Merkle root: leaf_k = H(0x00 || tx_k), node(l, r) =
 *           H(0x01 || l || r); H("") for n = 0, the leaf for n = 1, else
 *           node(root(first i), root(rest)), i the largest power of two < n
 *   TXWIT   txpWitnessesHash == H(0x9f || witnesses_0 || ... || 0xff)
 *   DLG     dlgHash == H(dlgPayload)        UPD  updHash == H(updPayload)
 * The SSC proof is not compared (the reference's SscProof is a unit); only
 * [uint, bytes(32)] is demanded of it.
 * Pinned by the reference's golden Byron block: the leaf form, the witnesses
 * list form, the two payload hashes.  NOT pinned by any reference fixture
 * (restated from cardano-ledger's Byron part, outside the reference tree): the
 * tree shape for n >= 2 and the empty root; non-canonical or indefinite
 * encodings inside a witness vector (the reference may re-serialise there;
 * this library hashes the bytes as they stand); that the SSC proof's content
 * is ignored.  The transaction witnesses are not verified here:
 * ouro_byron_block_witness_verify_cbor below.
 * Outputs: status[i] = OURO_PACK_* (OK, ECBOR, ESHAPE, ESIZE, EBB, ESHELLEY;
 * ESPAN and ECAP from the _device form); verdict[i] = OURO_BYB_* bits, 0 for a
 * block that does not slice; tx_root (n x 32, may be NULL) the computed Merkle
 * root, zeros unless the status is OURO_PACK_OK.
 *   ouro_byron_block_count_cbor[_host]: the slicer's count pass alone: status,
 *     ntx[i], gather_bytes[i] (the block's witness vectors + 2) and
 *     msg_bytes[i] (its signed message), zeros unless the status is
 *     OURO_PACK_OK, and totals[0..2] their sums -- what a caller of the _device
 *     form sizes the three capacities from.
 *   ouro_byron_block_integrity_verify_cbor: host buffers, synchronous, on the
 *     calling thread's stream, in consecutive groups of whole blocks under a
 *     byte budget (OURO_BYRON_BLOCK_GROUP_BYTES), each sized from its count
 *     pass; a device error recomputes the call on the host path.
 *   ouro_byron_block_integrity_verify_cbor_host: the host path alone.
 *   All four return OURO_EINVAL, before any work, for NULLs, a span outside
 *   raw_bytes, or a protocol_magic outside -1 .. 2^32 - 1.
 *   ouro_byron_block_integrity_verify_cbor_device: device pointers (raw as for
 *     ouro_blake2b256_batch_device; off 8-byte, len 4-byte, tx_root 16-byte
 *     aligned; work of ouro_byron_block_work_bytes(n, tx_cap, gather_cap,
 *     msg_cap) bytes), enqueued on `stream`, not synchronised, no host round
 *     trip.  A span outside raw_bytes is per-block status OURO_PACK_ESPAN.  A
 *     regular block whose transaction rows, gathered bytes or message would
 *     pass a capacity writes nothing and has status OURO_PACK_ECAP, verdict 0;
 *     the blocks that fit are a prefix of the regular ones.
 * Out of scope: one entry for mixed eras (partition a stream by the block tag),
 * _multi forms, the chunked raw pipeline, the latency plans. */
#define OURO_BYB_HDR_OK 0x01u    /* verifyHeaderIntegrity                 */
#define OURO_BYB_BODY_OK 0x02u   /* blockMatchesHeader: all five below    */
#define OURO_BYB_TXNUM_OK 0x04u
#define OURO_BYB_TXROOT_OK 0x08u
#define OURO_BYB_TXWIT_OK 0x10u
#define OURO_BYB_DLG_OK 0x20u
#define OURO_BYB_UPD_OK 0x40u
#define OURO_BYB_ALL_OK 0x7fu
int ouro_byron_block_count_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                const uint32_t *len, size_t n, int64_t protocol_magic,
                                uint8_t *status, uint32_t *ntx, uint32_t *gather_bytes,
                                uint32_t *msg_bytes, uint64_t *totals);
int ouro_byron_block_count_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                     const uint32_t *len, size_t n, int64_t protocol_magic,
                                     uint8_t *status, uint32_t *ntx, uint32_t *gather_bytes,
                                     uint32_t *msg_bytes, uint64_t *totals);
int ouro_byron_block_integrity_verify_cbor(const uint8_t *raw, size_t raw_bytes,
                                           const uint64_t *off, const uint32_t *len, size_t n,
                                           int64_t protocol_magic, uint8_t *status,
                                           uint8_t *verdict, uint8_t *tx_root);
int ouro_byron_block_integrity_verify_cbor_host(const uint8_t *raw, size_t raw_bytes,
                                                const uint64_t *off, const uint32_t *len,
                                                size_t n, int64_t protocol_magic,
                                                uint8_t *status, uint8_t *verdict,
                                                uint8_t *tx_root);
size_t ouro_byron_block_work_bytes(size_t n, size_t tx_cap, size_t gather_cap, size_t msg_cap);
int ouro_byron_block_integrity_verify_cbor_device(void *stream, const uint8_t *raw,
                                                  size_t raw_bytes, const uint64_t *off,
                                                  const uint32_t *len, size_t n,
                                                  int64_t protocol_magic, size_t tx_cap,
                                                  size_t gather_cap, size_t msg_cap, void *work,
                                                  size_t work_bytes, uint8_t *status,
                                                  uint8_t *verdict, uint8_t *tx_root);

/* Byron transaction witnesses straight from raw block CBOR: the ByronDSIGN
 * verification of every witness of every transaction over its signed message,
 * the crypto call of CC.validateBlock with BlockValidation (ouroboros-consensus-
 * byron/src/Ouroboros/Consensus/Byron/Ledger/Ledger.hs:190,346): one signature
 * per transaction input.  The entries follow ouro_block_witness_* above (rows,
 * capacities and the prefix property, OURO_PACK_ECAP, the row arrays) and
 * ouro_byron_block_integrity_verify_cbor in the block forms and statuses: block
 * i is raw[off[i] .. off[i] + len[i]) in either Byron form; everything outside
 * the witness vectors keeps that entry's acceptance, status for status.  Tag 0
 * (an EBB) is status OURO_PACK_EBB with verdict OURO_BYW_ALL_OK and no rows, a
 * tag >= 2 OURO_PACK_ESHELLEY.  Every txPayload element is [tx, witnesses]:
 *   witnesses = [* [type: uint, #6.24(bytes .cbor [key: bytes, sig: bytes])]]
 *     definite or indefinite; each element a definite array(2); the tag-24
 *     payload a definite byte string whose content is a definite array(2) of
 *     two definite byte strings and ends exactly at the payload's end
 *   type 0 (VKWitness):     key bytes(64) (an XPub), sig bytes(64)
 *   type 2 (RedeemWitness): key bytes(32),           sig bytes(64)
 * Any other type, major type, tag or array length is OURO_PACK_ESHAPE for the
 * block; content malformed inside the payload or not ending at its end
 * OURO_PACK_ECBOR; a wrong string length OURO_PACK_ESIZE -- per witness the
 * content is walked first, then the two types, then the two sizes.  The status
 * is that of the first offending item in byte order; malformed CBOR anywhere
 * inside a [tx, witnesses] element is found by the outer walk before the
 * element's witness vector is read.  A block that does not slice owns no rows.
 * tx id = Blake2b-256 of the tx item's bytes as they stand (no prefix byte: not
 * the Merkle leaf).  The signed message is
 *   tag || CBOR(magic) || 0x58 0x20 || tx_id
 * with tag 0x01 (SignTx) for type 0 and 0x02 (SignRedeemTx) for type 2, and
 * magic the configured protocol_magic, or for -1 each block header's own field
 * (mainnet, type 0: 01 1a 2d 96 4a 09 58 20).  Both kinds verify under
 * ByronDSIGN acceptance (ouro_byron_ed25519_verify_batch's): type 0 under
 * XPub[0:32], type 2 under the 32-byte redeem key.
 * Pinned by the reference's golden Byron block: the witness vector's shape
 * (81 82 00 d8 18 58 85 82 58 40 <64> 58 40 <64>).  NOT pinned by any reference
 * fixture (restated from cardano-ledger's Cardano.Chain.UTxO.TxWitness and
 * Cardano.Crypto.Signing.Tag, outside the reference tree, which only names
 * SignTx at Byron/Crypto/DSIGN.hs:59): the signed message (the tag bytes and
 * the 58 20 wrapped id); that the tx id hashes the bytes as they stand; that
 * the redeem kind uses ByronDSIGN's acceptance rules; that an unknown witness
 * type fails the block's decode.  The golden GenTxId_Byron is the example's
 * input id, not this transaction's, and pins nothing here.
 * Outputs: status[i] = OURO_PACK_*; n_bad[i] = the block's rows that do not
 * verify; verdict[i] = OURO_BYW_ALL_OK iff the block sliced, fit and n_bad[i]
 * == 0 (so also for a regular block without transactions) or is an EBB.
 *   ouro_byron_block_witness_count_cbor[_host]: the count pass alone: status,
 *     ntx[i] and nwit[i], zeros unless the status is OURO_PACK_OK.
 *   ouro_byron_block_witness_verify_cbor: host buffers, synchronous, on the
 *     calling thread's stream, in consecutive groups of whole blocks under a
 *     byte budget (OURO_BYRON_WITNESS_GROUP_BYTES), each sized from its own
 *     count pass; a device error recomputes the call on the host path.  Rows
 *     past the blocks that fit are left untouched.
 *   ouro_byron_block_witness_verify_cbor_host: the host path alone.
 *   All four return OURO_EINVAL, before any work, for NULLs, a span outside
 *   raw_bytes, or a protocol_magic outside -1 .. 2^32 - 1.
 *   ouro_byron_block_witness_verify_cbor_device: device pointers (alignment
 *     and work as for ouro_block_witness_verify_cbor_device, the work of
 *     ouro_byron_block_witness_work_bytes(n, tx_cap, wit_cap) bytes), enqueued
 *     on `stream`, not synchronised, no host round trip; a span outside
 *     raw_bytes is per-block status OURO_PACK_ESPAN; rows past the blocks that
 *     fit are zero.
 * Out of scope: that a witness's key hashes to the spent output's address, that
 * there is one witness per input, and every other UTxO rule (these need ledger
 * state); delegation certificates and update proposals or votes inside the
 * body (ouro_byron_dlg_cert_verify_batch serves a caller that has decoded
 * them); the mempool's standalone GenTx form [0, [tx, witnesses]]; _multi
 * forms; the chunked raw pipeline; fusing with the integrity entry; the latency
 * plans. */
#define OURO_BYW_ALL_OK 0x01u
typedef struct {
  size_t tx_cap, wit_cap;
  uint64_t *tx_begin, *wit_begin; /* n + 1 each; [n] = totals, also when they pass the caps */
  uint8_t *tx_id;                 /* tx_cap x 32 */
  uint32_t *wit_tx;               /* wit_cap: global tx row */
  uint8_t *wit_kind, *wit_ok;     /* wit_cap each: kind 0 = VKWitness, 2 = RedeemWitness; 1 = verifies */
  uint8_t *wit_vk;                /* wit_cap x 64, may be NULL: the XPub; a redeem key then 32 zero bytes */
} ouro_byron_block_witness_out;
int ouro_byron_block_witness_count_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                        const uint32_t *len, size_t n, int64_t protocol_magic,
                                        uint8_t *status, uint32_t *ntx, uint32_t *nwit);
int ouro_byron_block_witness_count_cbor_host(const uint8_t *raw, size_t raw_bytes,
                                             const uint64_t *off, const uint32_t *len, size_t n,
                                             int64_t protocol_magic, uint8_t *status,
                                             uint32_t *ntx, uint32_t *nwit);
int ouro_byron_block_witness_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                         const uint32_t *len, size_t n, int64_t protocol_magic,
                                         const ouro_byron_block_witness_out *out, uint8_t *status,
                                         uint8_t *verdict, uint32_t *n_bad);
int ouro_byron_block_witness_verify_cbor_host(const uint8_t *raw, size_t raw_bytes,
                                              const uint64_t *off, const uint32_t *len, size_t n,
                                              int64_t protocol_magic,
                                              const ouro_byron_block_witness_out *out,
                                              uint8_t *status, uint8_t *verdict, uint32_t *n_bad);
size_t ouro_byron_block_witness_work_bytes(size_t n, size_t tx_cap, size_t wit_cap);
int ouro_byron_block_witness_verify_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                                const uint64_t *off, const uint32_t *len, size_t n,
                                                int64_t protocol_magic,
                                                const ouro_byron_block_witness_out *out, void *work,
                                                size_t work_bytes, uint8_t *status,
                                                uint8_t *verdict, uint32_t *n_bad);
/* A raw header stream across eras and epochs in ONE call: what ChainDB's
 * re-validation of a stored suffix (LgrDB.hs:350-368), ImmutableDB /
 * VolatileDB replay and ChainSync windows of a Cardano chain actually hold --
 * Byron and Shelley-family headers in one buffer, Shelley slots over many
 * epochs.  Headers as for ouro_tpraos_pack_cbor and ouro_byron_pack_cbor.
 * proto[i] (required) = the header's protocol by its first few CBOR heads:
 *   OURO_PROTO_PBFT iff it is a definite array(2) whose first item is the
 *   definite uint 0 (HFC era 0), or a definite array(2) whose first item is an
 *   array (Byron N2N v2), or #6.24 + a definite byte string whose payload
 *   starts with a definite array(2) whose first item is a definite uint
 *   (Byron N2N v1); OURO_PROTO_TPRAOS for everything else (truncated or
 *   unreadable input included: the TPraos slicer's status says why).
 * A header goes to exactly one slicer, so OURO_PACK_EBYRON and
 * OURO_PACK_ESHELLEY never come out of this entry.
 * PBFT rows: status / verdict exactly as ouro_byron_verify_cbor (1 for a
 * verified regular header and for an epoch-boundary header, else 0); their
 * beta_eta / beta_leader / eta_nonce rows are zero.  TPraos rows: everything
 * exactly as ouro_tpraos_verify_cbor.  OURO_CHAIN_VALID(proto[i], verdict[i])
 * is the per-header answer.
 * VRF inputs: both eta_alpha and leader_alpha (n x 32, PBFT rows ignored) =
 * explicit inputs; otherwise mkSeed on the device under `epochs`
 * (ouro_epoch_nonces above), epochs == NULL = NeutralNonce everywhere.
 * epochs together with alphas, or one alpha array only: OURO_EINVAL.  The
 * other argument checks (spans, a zero period, the magic's range, NULLs, the
 * device list) are those of the two single-era entries, before any work.
 * How it runs: the pipeline of ouro_tpraos_verify_cbor; each header is
 * classified while its bytes are gathered into pinned staging (no extra pass
 * over the caller's buffer).  A chunk of one era runs that era's path
 * unchanged; a mixed chunk uploads its bytes once and runs the Byron slicer +
 * ByronDSIGN kernel over its PBFT headers and the TPraos slicer + header
 * kernel over its TPraos headers on the chunk's stream, each through its own
 * offset / length list, and both result sets are scattered back to the
 * caller's order.  Per context only the index lists are kept beside the
 * pipeline's buffers.  _host: the same on the host path, no device touched;
 * _multi: contiguous shards over the listed devices, as the other _multi
 * entries.  Out of scope: device-pointer forms; the latency plans. */
#define OURO_PROTO_PBFT 0u
#define OURO_PROTO_TPRAOS 1u
#define OURO_CHAIN_VALID(proto, v) \
  ((proto) == OURO_PROTO_PBFT ? (v) == 1 : ((v) & OURO_HDR_ALL_OK) == OURO_HDR_ALL_OK)
int ouro_chain_verify_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                           const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                           int64_t protocol_magic, const ouro_epoch_nonces *epochs,
                           const uint8_t *eta_alpha, const uint8_t *leader_alpha,
                           uint8_t *proto, uint8_t *status, uint8_t *verdict,
                           uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce);
int ouro_chain_verify_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                                int64_t protocol_magic, const ouro_epoch_nonces *epochs,
                                const uint8_t *eta_alpha, const uint8_t *leader_alpha,
                                uint8_t *proto, uint8_t *status, uint8_t *verdict,
                                uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce);
int ouro_chain_verify_cbor_multi(const int *devices, int ndev, const uint8_t *raw,
                                 size_t raw_bytes, const uint64_t *off, const uint32_t *len,
                                 size_t n, uint64_t slots_per_kes_period, int64_t protocol_magic,
                                 const ouro_epoch_nonces *epochs, const uint8_t *eta_alpha,
                                 const uint8_t *leader_alpha, uint8_t *proto, uint8_t *status,
                                 uint8_t *verdict, uint8_t *beta_eta, uint8_t *beta_leader,
                                 uint8_t *eta_nonce);

/* The header ENVELOPE of a raw chain, and every header's hash: the first half
 * of validateHeader (ouroboros-consensus/src/Ouroboros/Consensus/
 * HeaderValidation.hs:413-432), validateEnvelope (:297-344), which the crypto
 * entries above leave to the caller -- block number, slot, previous hash and
 * the block type's additional checks of header i against header i - 1, over
 * the same raw headers (Byron and Shelley-family in one buffer, classified as
 * by ouro_chain_verify_cbor).  The header hash is the point ChainSync and the
 * ChainDB ask for next.
 * header_hash[i] (n x 32):
 *   TPraos  Blake2b-256 of the #6.24 payload, the [header_body, kes_sig] item
 *           as it stands (ouroboros-consensus-shelley/src/Ouroboros/Consensus/
 *           Shelley/Ledger/Block.hs:106,142);
 *   Byron   Blake2b-256(0x82, kind, header item), kind 1 regular / 0 epoch
 *           boundary, in all three wire forms (ouroboros-consensus-byron/src/
 *           Ouroboros/Consensus/Byron/Ledger/Block.hs:74, Orphans.hs:101).
 * envelope[i]: OURO_ENV_* bits of header i on top of header i - 1 AS GIVEN
 * (header 0 on top of tip_in, NULL = Origin); OURO_ENV_ALL_OK on every header
 * of a prefix = validateEnvelope accepts that prefix.  All four bits are
 * evaluated, where the reference stops at the first failure.
 *   BLOCKNO  0 at Origin, else succ; unchanged from a Byron non-EBB to a Byron
 *            EBB (Byron/Ledger/HeaderValidation.hs:46-50); succ across eras
 *            (HardFork/Combinator/Block.hs:235-238).
 *   SLOT     slot >= 0 at Origin, else >= succ; >= the same slot from a Byron
 *            EBB to a Byron non-EBB (:52-56); succ across eras (:249-252).
 *   PREVHASH checkPrevHash' (HeaderValidation.hs:313-318): GenesisHash at
 *            Origin, else a block hash equal to header i - 1's header_hash.
 *            TPraos field 2: null = GenesisHash, bytes(32) = a block hash,
 *            anything else clears the bit.  A Byron EBB of epoch 0 has
 *            GenesisHash, every other Byron header a block hash.
 *   EXTRA    Byron: an EBB's slot is a multiple of byron_epoch_slots
 *            (:61-72).  TPraos with cfg->has_limits: header size (the payload's
 *            bytes) <= max_header_size, body field 7 <= max_body_size, field
 *            13 <= max_major_pv (ledger-specs chainChecks, called at
 *            Shelley/Ledger/Ledger.hs:395-396).  Otherwise set.
 * Slots: TPraos field 1; Byron epoch * byron_epoch_slots + slot in epoch
 * (an EBB: epoch * byron_epoch_slots), Word64 arithmetic.
 * status[i]: the slicer's OURO_PACK_* of the header's era, as
 * ouro_chain_verify_cbor reports it.  A header that did not slice, or whose
 * envelope fields have another shape (an EBB is accepted by the slicer
 * without a look inside), has envelope 0 and a zero hash; its successor has
 * the three link bits clear and its own EXTRA bit evaluated.
 * tip_out (optional): the last header as a tip, so that calls chain: passing
 * it as the next call's tip_in gives the bits one call over both batches
 * gives.  (After an unusable last header its proto is 0xff: nothing links.)
 * OURO_EINVAL before anything runs: NULL raw / off / len / cfg / status /
 * header_hash / envelope with n > 0, a span outside raw_bytes, a tip_in with
 * origin set and another field nonzero (or proto / is_ebb out of range), and
 * byron_epoch_slots == 0 when a header of the batch is PBFT.
 * How it runs: one upload, the envelope slicer (both eras' slicers without
 * their rows), the hash kernel (one lane per header) and the link kernel on
 * the calling thread's stream, one copy back; a device error recomputes on
 * the host path.  _host: the host path alone.  _device: raw / off / len /
 * status / header_hash / envelope / tip_out are device pointers (tip_out may
 * be NULL), cfg and tip_in host pointers read before the call returns; raw
 * 4-byte aligned and its allocation extended to the next multiple of 4, as
 * for ouro_block_integrity_verify_cbor_device; header_hash 16-byte aligned and
 * tip_out 8-byte aligned (OURO_EINVAL otherwise); work >=
 * ouro_chain_envelope_work_bytes(n) of device memory; enqueued on `stream`,
 * not synchronised; a span outside raw_bytes is status OURO_PACK_ESPAN, and
 * with byron_epoch_slots == 0 a PBFT header is unusable (envelope 0).
 * n == 0: cfg and tip_in are checked all the same; the host-buffer forms then
 * write tip_in's tip to tip_out, the device form writes nothing. */
#define OURO_ENV_BLOCKNO_OK 0x01u
#define OURO_ENV_SLOT_OK 0x02u
#define OURO_ENV_PREVHASH_OK 0x04u
#define OURO_ENV_EXTRA_OK 0x08u
#define OURO_ENV_ALL_OK 0x0fu
typedef struct ouro_chain_tip {
  uint8_t origin; /* 1 = no header yet; every other field then 0 */
  uint8_t proto;  /* OURO_PROTO_* of the tip's header                */
  uint8_t is_ebb;
  uint8_t reserved[5];
  uint64_t slot;
  uint64_t block_no;
  uint8_t hash[32];
} ouro_chain_tip;
typedef struct ouro_envelope_cfg {
  uint64_t byron_epoch_slots; /* slots of a Byron epoch (mainnet: 21600)  */
  uint64_t has_limits;        /* nonzero: the three TPraos limits apply  */
  uint64_t max_header_size;
  uint64_t max_body_size;
  uint64_t max_major_pv;
} ouro_envelope_cfg;
int ouro_chain_envelope_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                             const uint32_t *len, size_t n, const ouro_envelope_cfg *cfg,
                             const ouro_chain_tip *tip_in, uint8_t *status,
                             uint8_t *header_hash, uint8_t *envelope, ouro_chain_tip *tip_out);
int ouro_chain_envelope_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                  const uint32_t *len, size_t n, const ouro_envelope_cfg *cfg,
                                  const ouro_chain_tip *tip_in, uint8_t *status,
                                  uint8_t *header_hash, uint8_t *envelope,
                                  ouro_chain_tip *tip_out);
size_t ouro_chain_envelope_work_bytes(size_t n);
int ouro_chain_envelope_cbor_device(void *stream, const uint8_t *raw, size_t raw_bytes,
                                    const uint64_t *off, const uint32_t *len, size_t n,
                                    const ouro_envelope_cfg *cfg, const ouro_chain_tip *tip_in,
                                    void *work, size_t work_bytes, uint8_t *status,
                                    uint8_t *header_hash, uint8_t *envelope,
                                    ouro_chain_tip *tip_out);

/* validateHeader (HeaderValidation.hs:413-432) over a raw chain in ONE call:
 * everything ouro_chain_verify_cbor returns (the arguments up to eta_nonce
 * are its arguments, with the same meaning, checks and results) and the
 * envelope of ouro_chain_envelope_cbor (cfg, tip_in, header_hash, envelope,
 * tip_out as there; header_hash and envelope required).  The longest prefix
 * with OURO_ENV_ALL_OK and OURO_CHAIN_VALID on every header is what the
 * reference's sequential fold accepts.
 * How it runs: the pipeline of ouro_chain_verify_cbor, unchanged; after a
 * chunk's slicers and kernels, on the same stream and over the bytes already
 * uploaded, the envelope slicer, the hash kernel and the link kernel run over
 * the chunk in the caller's order (a mixed chunk keeps a second, caller-order
 * offset list for them), and the chunk copies back 33 more bytes per header
 * and its first and last record.  Chunks drain in order: the host links each
 * chunk's first header to the last record of the chunk before it (or to
 * tip_in) with the same envelope_link the kernel runs.  A device error
 * recomputes the batch, envelope included, on the host path.  _host: the host
 * path alone.  byron_epoch_slots == 0 with a PBFT header in the batch is
 * OURO_EINVAL before anything runs.  Out of scope: a _multi form (the link
 * across shards), device pointers, the latency plans.  The checks that need
 * the ledger view (pool stake, VRF key hash, leader value, OCERT period and
 * counter): ouro_chain_validate_ledger_cbor below. */
int ouro_chain_validate_cbor(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                             const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                             int64_t protocol_magic, const ouro_epoch_nonces *epochs,
                             const uint8_t *eta_alpha, const uint8_t *leader_alpha,
                             const ouro_envelope_cfg *cfg, const ouro_chain_tip *tip_in,
                             uint8_t *proto, uint8_t *status, uint8_t *verdict,
                             uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce,
                             uint8_t *header_hash, uint8_t *envelope, ouro_chain_tip *tip_out);
int ouro_chain_validate_cbor_host(const uint8_t *raw, size_t raw_bytes, const uint64_t *off,
                                  const uint32_t *len, size_t n, uint64_t slots_per_kes_period,
                                  int64_t protocol_magic, const ouro_epoch_nonces *epochs,
                                  const uint8_t *eta_alpha, const uint8_t *leader_alpha,
                                  const ouro_envelope_cfg *cfg, const ouro_chain_tip *tip_in,
                                  uint8_t *proto, uint8_t *status, uint8_t *verdict,
                                  uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce,
                                  uint8_t *header_hash, uint8_t *envelope,
                                  ouro_chain_tip *tip_out);

/* ------------------------------------------- ledger-view header checks ----- */
/* What SL.updateChainDepState (ouroboros-consensus-shelley/src/Ouroboros/
 * Consensus/Shelley/Protocol.hs:433-442) checks with the epoch's LedgerView
 * beside the signatures: the ledger-specs OVERLAY and OCERT rules, per TPraos
 * header, as OURO_LV_* bits -- all of them, where the reference stops at the
 * first failure (the OURO_ENV_* convention).  A PBFT or unsliced header gets 0.
 *   POOL_KNOWN      hashKey (Blake2b-224) of the cold key is in the entry's
 *                   pool distribution                      (VRFKeyUnknown)
 *   VRF_KEY_OK      hashVerKeyVRF (Blake2b-256) of the header's VRF key is the
 *                   registered one                         (VRFKeyWrongVRFKey)
 *   LEADER_OK       checkLeaderValue of the header's CLAIMED leader output
 *                   (Protocol.hs:484-485) under that pool's relative stake
 *                                                          (VRFLeaderValueTooBig)
 *   KES_PERIOD_OK   c0 <= kesPeriod(slot) < c0 + max_kes_evo, the sum taken
 *                   without wrapping: c0 > 2^64 - max_kes_evo fails
 *                                    (KESBeforeStartOCERT, KESAfterEndOCERT)
 *   COUNTER_OK      the certificate counter does not go back for the pool
 *                   (CounterTooSmallOCERT): ouro_ocert_counter_fold
 *   OVERLAY         the slot is an overlay slot (ledger-specs isOverlaySlot:
 *                   ceil(s d) < ceil((s + 1) d), s = slot - the entry's
 *                   first_slot, exact integers; d_num == 0: never).  Without
 *                   a genesis-delegation schedule (ouro_genesis_delegs below)
 *                   only KES_PERIOD_OK is evaluated then and the fold skips
 *                   the row; with one, the genesis-delegate branch
 *                   (pbftVrfChecks) is evaluated as the table below says.
 *   OVERLAY_ACTIVE  (with a schedule only) the overlay slot is an active one
 *                                                   (else NotActiveSlotOVERLAY)
 *   BADARG          the leader check's arguments are outside its domain
 *                   (OURO_LEADER_BADARG); LEADER_OK is then clear. */
#define OURO_LV_POOL_KNOWN 0x01u
#define OURO_LV_VRF_KEY_OK 0x02u
#define OURO_LV_LEADER_OK 0x04u
#define OURO_LV_KES_PERIOD_OK 0x08u
#define OURO_LV_COUNTER_OK 0x10u
#define OURO_LV_OVERLAY_ACTIVE 0x20u
#define OURO_LV_OVERLAY 0x40u
#define OURO_LV_BADARG 0x80u
#define OURO_LV_ALL_OK 0x1fu
#define OURO_LV_NO_POOL 0xffffffffu
#define OURO_LV_ROWS_MAX ((size_t)1 << 24)
#define OURO_LV_GEN_ROWS_MAX ((size_t)1 << 16)
/* A ledger-view schedule, shaped like ouro_epoch_nonces: entry j applies to
 * first_slot[j] <= slot (the last such entry; found by the same binary
 * search), and first_slot[j] is taken as the first slot of that epoch.  Entry
 * j's pools are rows pool_begin[j] .. pool_begin[j + 1] of the flat arrays,
 * sorted by the 28 id bytes as unsigned bytes, strictly ascending.
 * OURO_EINVAL before anything runs: k outside 1 .. OURO_EPOCHS_MAX,
 * first_slot[0] != 0 or not strictly increasing, pool_begin[0] != 0 or
 * decreasing, more than OURO_LV_ROWS_MAX rows, rows out of order, d_den == 0,
 * d_num > d_den, sigma_den == 0, sigma_num > sigma_den, a NULL array. */
typedef struct ouro_ledger_views {
  size_t k;
  const uint64_t *first_slot; /* k                                              */
  const uint64_t *d_num;      /* k    decentralisation parameter d = num / den  */
  const uint64_t *d_den;      /* k                                              */
  const uint32_t *pool_begin; /* k + 1                                          */
  const uint8_t *pool_id;     /* rows x 28  hashKey of the pool's cold key      */
  const uint8_t *vrf_hash;    /* rows x 32  hashVerKeyVRF of its VRF key        */
  const uint64_t *sigma_num;  /* rows       relative stake = num / den          */
  const uint64_t *sigma_den;  /* rows                                           */
} ouro_ledger_views;
/* slots_per_kes_period > 0 (OURO_EINVAL); act_log_* / f_is_one as
 * ouro_leader_check_batch */
typedef struct ouro_ledger_globals {
  uint64_t slots_per_kes_period;
  uint64_t max_kes_evo;
  int64_t act_log_hi;
  uint64_t act_log_lo;
  int f_is_one;
} ouro_ledger_globals;
/* The OCERT counters a chain state holds (ChainDepState's csCounters): m pool
 * ids, sorted like a view entry's rows, with counter[i] valid where
 * present[i] != 0.  The table must contain every pool id of every view row
 * (OURO_EINVAL otherwise): a pool in the distribution without a counter yet
 * is a row with present = 0 -- currentIssueNo's "in the pool distribution"
 * case, counter 0. */
typedef struct ouro_ocert_counters {
  size_t m;
  const uint8_t *pool_id;  /* m x 28, strictly ascending */
  const uint64_t *counter; /* m */
  const uint8_t *present;  /* m */
} ouro_ocert_counters;

/* The genesis delegations of a ledger-view schedule, for the overlay slots
 * (ledger-specs OVERLAY rule's other branch: lookupInOverlaySchedule, then
 * pbftVrfChecks; the reference walks it first, Shelley/Protocol.hs:366-399).
 * Entry j belongs to view entry j; its rows are its genesis keys, sorted by
 * the 28 id bytes as Map.keysSet gives them (Protocol.hs:406), each with the
 * GenDelegPair it maps to.  For a TPraos row of entry j on an overlay slot,
 * with s = slot - first_slot[j] and d = d_num[j] / d_den[j], exact integers:
 *   position = ceil(s d);  the slot is ACTIVE iff position mod asc_inv == 0;
 *   then the scheduled genesis key is row (position div asc_inv) mod ngen of
 *   the entry (Set.elemAt: a direct index), and
 *     POOL_KNOWN     active and Blake2b-224(issuer_vk) == delegate_id[row]
 *                                              (else WrongGenesisColdKeyOVERLAY)
 *     VRF_KEY_OK     POOL_KNOWN and Blake2b-256(vrf_vk) == delegate_vrf[row]
 *                                              (else WrongGenesisVRFKeyOVERLAY)
 *     LEADER_OK      = POOL_KNOWN: no threshold on an overlay slot; BADARG never
 *     KES_PERIOD_OK  as on any slot
 *     COUNTER_OK     the fold, keyed by delegate_id[row] in the same counters
 *                    table (currentIssueNo: 0 for a delegate without a counter)
 *   and pool_row[i] is the absolute genesis row when POOL_KNOWN, else
 *   OURO_LV_NO_POOL: OVERLAY tells which table the row indexes.  A valid header
 *   has (bits & OURO_LV_ALL_OK) == OURO_LV_ALL_OK on either kind of slot.
 * asc_inv = floor(1 / f) >= 1 is an input of its own: it cannot be derived
 * exactly from act_log_*.
 * OURO_EINVAL before anything runs: k != views->k, gen_begin[0] != 0 or
 * decreasing, more than OURO_LV_GEN_ROWS_MAX rows, genesis_id not strictly
 * ascending inside an entry, asc_inv == 0, an entry with d_num > 0 and no rows
 * (the reference divides by zero there), a NULL array; with counters, a
 * delegate_id the counters table has no row for. */
typedef struct ouro_genesis_delegs {
  size_t k;
  const uint32_t *gen_begin;   /* k + 1                                         */
  const uint8_t *genesis_id;   /* rows x 28  hashKey of the genesis key         */
  const uint8_t *delegate_id;  /* rows x 28  genDelegKeyHash                    */
  const uint8_t *delegate_vrf; /* rows x 32  genDelegVrfHash                    */
  uint64_t asc_inv;            /* floor(1 / f)                                  */
} ouro_genesis_delegs;

/* The OCERT rule's counter check (CounterTooSmallOCERT) over n headers in
 * stream order, on the host, exact; the sibling of ouro_nonce_fold.  Header i
 * is skipped when OURO_LV_POOL_KNOWN is clear in ledger[i] (a PBFT or unsliced
 * header, an unknown pool) or OURO_LV_OVERLAY is set.  Otherwise, with m0 the
 * pool's counter in the table (0 when not present): OURO_LV_COUNTER_OK is set
 * in ledger[i] iff m0 <= ocert_counter[i]; then ocert_counter[i] is stored and
 * the pool marked present AS GIVEN, whatever the verdict -- the way the
 * envelope links to header i - 1 as given; the caller stops at the first
 * invalid header.  pool_row[i]: the header's view row (ouro_tpraos_ledger_
 * checks).  The updated table goes to counter_out / present_out (m each; may
 * alias the inputs), so calls chain like tip_out.  The row-to-table index map
 * is built once per call by merging the sorted lists. */
int ouro_ocert_counter_fold(size_t n, const uint32_t *pool_row, const uint64_t *ocert_counter,
                            const ouro_ledger_views *views, const ouro_ocert_counters *in,
                            uint64_t *counter_out, uint8_t *present_out, uint8_t *ledger);
/* The same fold with a genesis-delegation schedule (NULL: exactly the fold
 * above): a header with OURO_LV_OVERLAY and OURO_LV_POOL_KNOWN is folded too,
 * its pool_row[i] a genesis row and its key delegate_id[row] -- one table, so
 * a pool row and a delegate row of the same id share a counter. */
int ouro_ocert_counter_fold_overlay(size_t n, const uint32_t *pool_row,
                                    const uint64_t *ocert_counter, const ouro_ledger_views *views,
                                    const ouro_genesis_delegs *genesis,
                                    const ouro_ocert_counters *in, uint64_t *counter_out,
                                    uint8_t *present_out, uint8_t *ledger);

/* The rules above for n sliced TPraos header rows (SoA host buffers: the
 * columns of ouro_tpraos_batch, and the slots): ledger[i] = OURO_LV_* bits,
 * pool_row[i] (may be NULL) = the absolute view row of the issuer, or
 * OURO_LV_NO_POOL.  One lane per header on the GPU (k_ledger_checks); a
 * device error recomputes on the host path; _host is the host path alone.
 * counters (may be NULL, then ocert_counter, counter_out and present_out are
 * unused and OURO_LV_COUNTER_OK stays clear): the fold above runs over the
 * results.  Replaces, per header, the lookups and checkLeaderValue of
 * ledger-specs' OVERLAY rule (vrfChecks) and the period and counter checks
 * of its OCERT rule. */
int ouro_tpraos_ledger_checks(size_t n, const uint8_t *issuer_vk, const uint8_t *vrf_vk,
                              const uint64_t *slot, const uint8_t *leader_output,
                              const uint64_t *ocert_kes_period, const uint64_t *ocert_counter,
                              const ouro_ledger_views *views, const ouro_ledger_globals *globals,
                              const ouro_ocert_counters *counters, uint64_t *counter_out,
                              uint8_t *present_out, uint8_t *ledger, uint32_t *pool_row);
int ouro_tpraos_ledger_checks_host(size_t n, const uint8_t *issuer_vk, const uint8_t *vrf_vk,
                                   const uint64_t *slot, const uint8_t *leader_output,
                                   const uint64_t *ocert_kes_period,
                                   const uint64_t *ocert_counter, const ouro_ledger_views *views,
                                   const ouro_ledger_globals *globals,
                                   const ouro_ocert_counters *counters, uint64_t *counter_out,
                                   uint8_t *present_out, uint8_t *ledger, uint32_t *pool_row);
/* The same with a genesis-delegation schedule (NULL: exactly the entries
 * above, row for row): overlay rows are evaluated by the delegate branch in
 * the same kernel launch and folded against the delegates' ids. */
int ouro_tpraos_ledger_checks_overlay(size_t n, const uint8_t *issuer_vk, const uint8_t *vrf_vk,
                                      const uint64_t *slot, const uint8_t *leader_output,
                                      const uint64_t *ocert_kes_period,
                                      const uint64_t *ocert_counter, const ouro_ledger_views *views,
                                      const ouro_genesis_delegs *genesis,
                                      const ouro_ledger_globals *globals,
                                      const ouro_ocert_counters *counters, uint64_t *counter_out,
                                      uint8_t *present_out, uint8_t *ledger, uint32_t *pool_row);
int ouro_tpraos_ledger_checks_overlay_host(size_t n, const uint8_t *issuer_vk,
                                           const uint8_t *vrf_vk, const uint64_t *slot,
                                           const uint8_t *leader_output,
                                           const uint64_t *ocert_kes_period,
                                           const uint64_t *ocert_counter,
                                           const ouro_ledger_views *views,
                                           const ouro_genesis_delegs *genesis,
                                           const ouro_ledger_globals *globals,
                                           const ouro_ocert_counters *counters,
                                           uint64_t *counter_out, uint8_t *present_out,
                                           uint8_t *ledger, uint32_t *pool_row);
/* Device pointers on the caller's stream, not synchronised.  The views are
 * checked, packed and uploaded once by ouro_ledger_views_upload (synchronous;
 * on the calling thread's device) and released by ouro_ledger_views_free.
 * OURO_LV_COUNTER_OK is not evaluated: pool_row (required) is what
 * ouro_ocert_counter_fold needs once the results are on the host. */
typedef struct ouro_ledger_views_dev ouro_ledger_views_dev;
int ouro_ledger_views_upload(const ouro_ledger_views *views, ouro_ledger_views_dev **out);
/* The views and a genesis-delegation schedule (NULL: the upload above) checked
 * and packed into ONE device block.  ouro_tpraos_ledger_checks_device on such a
 * handle evaluates overlay rows by the delegate branch. */
int ouro_ledger_views_upload_overlay(const ouro_ledger_views *views,
                                     const ouro_genesis_delegs *genesis,
                                     ouro_ledger_views_dev **out);
void ouro_ledger_views_free(ouro_ledger_views_dev *dv);
int ouro_tpraos_ledger_checks_device(void *stream, size_t n, const uint8_t *issuer_vk,
                                     const uint8_t *vrf_vk, const uint64_t *slot,
                                     const uint8_t *leader_output,
                                     const uint64_t *ocert_kes_period,
                                     const ouro_ledger_views_dev *views,
                                     const ouro_ledger_globals *globals, uint8_t *ledger,
                                     uint32_t *pool_row);

/* ouro_chain_validate_cbor with the ledger-view checks in the same call:
 * every argument and result of that entry, unchanged, then the views, the
 * globals (their slots_per_kes_period must equal the call's), the counters in
 * and out (counters may be NULL: no fold) and ledger[n], pool_row[n] (may be
 * NULL).  How it runs: the views are uploaded once per call and every chunk's
 * stream waits on that upload; after a chunk's header kernel, on the chunk's
 * stream, k_ledger_checks runs over the TPraos rows already in the slot's
 * arena; the chunk copies back 13 more bytes per TPraos header (bits, row,
 * counter) and a mixed chunk scatters them through the same index list as
 * the verdicts; the fold runs in order as chunks drain.  A device error
 * recomputes the batch on the host path, this stage included.  _host: the
 * host path alone. */
int ouro_chain_validate_ledger_cbor(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_ledger_globals *globals, const ouro_ocert_counters *counters,
    uint64_t *counter_out, uint8_t *present_out, uint8_t *ledger, uint32_t *pool_row);
int ouro_chain_validate_ledger_cbor_host(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_ledger_globals *globals, const ouro_ocert_counters *counters,
    uint64_t *counter_out, uint8_t *present_out, uint8_t *ledger, uint32_t *pool_row);
/* The same with a genesis-delegation schedule after the views (NULL: exactly
 * the entries above).  The schedule is checked, packed and uploaded once per
 * call in the views' block, behind the same event; nothing more is copied per
 * chunk and the results stay 13 bytes per TPraos header. */
int ouro_chain_validate_ledger_overlay_cbor(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_genesis_delegs *genesis, const ouro_ledger_globals *globals,
    const ouro_ocert_counters *counters, uint64_t *counter_out, uint8_t *present_out,
    uint8_t *ledger, uint32_t *pool_row);
int ouro_chain_validate_ledger_overlay_cbor_host(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_genesis_delegs *genesis, const ouro_ledger_globals *globals,
    const ouro_ocert_counters *counters, uint64_t *counter_out, uint8_t *present_out,
    uint8_t *ledger, uint32_t *pool_row);

/* --------------------------------- Byron ledger-view checks (PBFT) --------- */
/* What the reference's PBFT instance checks per regular Byron header beside
 * the block signature (ouroboros-consensus/src/Ouroboros/Consensus/Protocol/
 * PBFT.hs:322-357), as OURO_PBFT_* bits -- all of them, where the reference
 * stops at the first failure (the OURO_LV_* convention):
 *   DELEGATE_KNOWN  hashVerKey of the header's delegate key is a delegate in
 *                   the entry's delegation map (Bimap.lookupR; else
 *                   PBftNotGenesisDelegate).  hashVerKey is CC.Common.hashKey:
 *                   KH(k) = Blake2b-224(SHA3-256(0x58 0x40 || k)) over the 64
 *                   XPub bytes (ouro_byron_key_hash_batch).
 *   SLOT_OK         the slot does not go back behind the last signed slot; the
 *                   inequality is non-strict (else PBftInvalidSlot)
 *   WINDOW_OK       the delegate's genesis key has signed at most `threshold`
 *                   of the last `window` blocks, this one included
 *                                             (else PBftExceededSignThreshold)
 *   BOUNDARY        an epoch-boundary header (status OURO_PACK_EBB):
 *                   PBftValidateBoundary checks nothing and leaves the state
 *                   alone; the row is BOUNDARY | ALL_OK, so a caller's
 *                   acceptance test is one mask on either kind of row.
 * A TPraos or unsliced row gets 0.  The bits do not depend on the signature
 * verdict.  DELEGATE_KNOWN and BOUNDARY are evaluated per row, in parallel
 * (k_pbft_checks, one row per lane); SLOT_OK and WINDOW_OK by the sequential
 * fold ouro_pbft_window_fold on the host. */
#define OURO_PBFT_DELEGATE_KNOWN 0x01u
#define OURO_PBFT_SLOT_OK 0x02u
#define OURO_PBFT_WINDOW_OK 0x04u
#define OURO_PBFT_BOUNDARY 0x08u
#define OURO_PBFT_ALL_OK 0x07u
/* A delegation schedule, shaped like ouro_ledger_views: entry j applies to
 * first_slot[j] <= slot (the last such entry, by the same binary search).
 * Entry j's delegation map is rows dlg_begin[j] .. dlg_begin[j + 1] of the
 * flat arrays: (delegate id, genesis id) pairs sorted by the 28 delegate id
 * bytes as unsigned bytes, strictly ascending; the genesis ids of an entry are
 * distinct too (the reference's map is a Bimap).  window >= 1 and threshold
 * are the reference's PBftWindowParams; floor(pbftSignatureThreshold * k)
 * (PBFT.hs:396-398, a Double product) is the caller's to compute.
 * OURO_EINVAL before anything runs: k outside 1 .. OURO_EPOCHS_MAX,
 * first_slot[0] != 0 or not strictly increasing, dlg_begin[0] != 0 or
 * decreasing, more than OURO_LV_GEN_ROWS_MAX rows, delegate ids out of order,
 * a genesis id twice in an entry, window == 0, a NULL array. */
typedef struct ouro_pbft_views {
  size_t k;
  const uint64_t *first_slot; /* k                                              */
  const uint32_t *dlg_begin;  /* k + 1                                          */
  const uint8_t *delegate_id; /* rows x 28  KH of the delegate's XPub, sorted   */
  const uint8_t *genesis_id;  /* rows x 28  KH of the genesis key it signs for  */
  uint64_t window;            /* >= 1                                           */
  uint64_t threshold;
} ouro_pbft_views;
/* The signing window a chain state holds (PBftState's inWindow): n <= window
 * signers, oldest first, each the genesis id and the slot it signed in.
 * OURO_EINVAL: n > window, a NULL array with n > 0. */
typedef struct ouro_pbft_state {
  size_t n;
  const uint8_t *signer_id;    /* n x 28  genesis ids */
  const uint64_t *signer_slot; /* n                   */
} ouro_pbft_state;

/* KH of n XPubs (n x 64 -> n x 28): what a caller builds a schedule's ids
 * with.  One key per lane on the GPU (k_byron_key_hash); a device error
 * recomputes on the host path; _host is the host path alone; _device: device
 * pointers (4-byte aligned) on the caller's stream, not synchronised. */
int ouro_byron_key_hash_batch(size_t n, const uint8_t *xpub, uint8_t *out);
int ouro_byron_key_hash_batch_host(size_t n, const uint8_t *xpub, uint8_t *out);
int ouro_byron_key_hash_batch_device(void *stream, size_t n, const uint8_t *xpub, uint8_t *out);

/* The window fold (PBFT/State.hs:207-229 append, PBFT.hs:340-357) over n rows
 * in stream order, on the host, exact; the sibling of ouro_ocert_counter_fold
 * and ouro_nonce_fold.  A row with OURO_PBFT_DELEGATE_KNOWN and without
 * OURO_PBFT_BOUNDARY in pbft[i] is folded, every other row is left as it is
 * (signed_count[i] = 0):
 *   SLOT_OK    iff the window is empty or slot[i] >= the last signer's slot;
 *   then (slot[i], genesis_id[genesis_row[i]]) is appended, and if the window
 *   held `window` signers BEFORE the append the oldest is dropped;
 *   signed_count[i] (may be NULL) = that genesis id's count in the window
 *   after the trim; WINDOW_OK iff signed_count[i] <= threshold.
 * The append happens AS GIVEN, whatever the bits and the signature say -- the
 * way the envelope links to header i - 1 as given; the caller stops at the
 * first invalid header, and up to and including it the bits equal the
 * reference's outcome.  Counting is by the 28 id bytes: an incoming signer
 * whose id no entry knows still counts.  The window afterwards goes to
 * signer_id_out / signer_slot_out (capacity `window` rows each; may alias the
 * inputs) and *n_out, so calls chain like tip_out.  in == NULL: the empty
 * window (genesis).  A folded row whose genesis_row[i] lies outside the
 * schedule (never what the rule gives) appends nothing: its SLOT_OK and
 * WINDOW_OK come out clear and the window stays as it was. */
int ouro_pbft_window_fold(size_t n, const uint32_t *genesis_row, const uint64_t *slot,
                          const ouro_pbft_views *views, const ouro_pbft_state *in,
                          uint8_t *signer_id_out, uint64_t *signer_slot_out, size_t *n_out,
                          uint8_t *pbft, uint64_t *signed_count);

/* The rules above for n Byron header rows (SoA host buffers: delegate_vk as
 * ouro_byron_batch has it, the slots, and status as ouro_byron_pack_cbor gives
 * it): pbft[i] = OURO_PBFT_* bits, genesis_row[i] (may be NULL) = the absolute
 * schedule row of the delegate, or OURO_LV_NO_POOL; signed_count (may be
 * NULL).  state_in == NULL: no fold -- only DELEGATE_KNOWN and BOUNDARY are
 * evaluated (a boundary row is BOUNDARY | ALL_OK either way) and the state
 * outputs are unused; otherwise the fold above runs over the results.  A
 * device error recomputes on the host path; _host is the host path alone. */
int ouro_pbft_ledger_checks(size_t n, const uint8_t *delegate_vk, const uint64_t *slot,
                            const uint8_t *status, const ouro_pbft_views *views,
                            const ouro_pbft_state *state_in, uint8_t *signer_id_out,
                            uint64_t *signer_slot_out, size_t *n_out, uint8_t *pbft,
                            uint32_t *genesis_row, uint64_t *signed_count);
int ouro_pbft_ledger_checks_host(size_t n, const uint8_t *delegate_vk, const uint64_t *slot,
                                 const uint8_t *status, const ouro_pbft_views *views,
                                 const ouro_pbft_state *state_in, uint8_t *signer_id_out,
                                 uint64_t *signer_slot_out, size_t *n_out, uint8_t *pbft,
                                 uint32_t *genesis_row, uint64_t *signed_count);
/* Device pointers on the caller's stream, not synchronised, no fold
 * (delegate_vk and genesis_row 4-byte aligned, slot 8-byte aligned;
 * genesis_row required).  The schedule is checked, packed and uploaded once by
 * ouro_pbft_views_upload (synchronous; on the calling thread's device) and
 * released by ouro_pbft_views_free. */
typedef struct ouro_pbft_views_dev ouro_pbft_views_dev;
int ouro_pbft_views_upload(const ouro_pbft_views *views, ouro_pbft_views_dev **out);
void ouro_pbft_views_free(ouro_pbft_views_dev *dv);
int ouro_pbft_ledger_checks_device(void *stream, size_t n, const uint8_t *delegate_vk,
                                   const uint64_t *slot, const uint8_t *status,
                                   const ouro_pbft_views_dev *views, uint8_t *pbft,
                                   uint32_t *genesis_row);

/* ouro_chain_validate_ledger_overlay_cbor with the Byron ledger-view checks in
 * the same call: every argument and result of that entry, unchanged, then the
 * delegation schedule, the window in and out (pbft_state_in may be NULL: no
 * fold, and the three state outputs are unused), pbft[n], genesis_row_pbft[n]
 * (may be NULL) and signed_count[n] (may be NULL).  With pbft_views NULL it is
 * the overlay entry, byte for byte, and the arguments after it are unused.  A
 * TPraos or unsliced row gets pbft = 0, row OURO_LV_NO_POOL, count 0.  The
 * slot of a Byron row is the envelope's: epoch * cfg->byron_epoch_slots + slot
 * in epoch.  How it runs: the schedule is packed and uploaded once per call
 * behind the same event as the ledger views; on a chunk's stream, after the
 * Byron slicer and the envelope slicer, k_pbft_checks_chain runs over the PBFT
 * rows already in the slot's arena, reading each row's slot from its envelope
 * record (a mixed chunk's through its index list); the chunk copies back 13
 * more bytes per PBFT row (bits, row, and the slot the host's fold needs) and
 * a mixed chunk scatters them through the existing index list; the window
 * fold runs in stream order as chunks drain, next to the counter fold.  A
 * device error recomputes the batch on the host path, this stage included,
 * the fold restarted from the window as the call found it.  _host: the host
 * path alone. */
int ouro_chain_validate_ledger_pbft_cbor(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_genesis_delegs *genesis, const ouro_ledger_globals *globals,
    const ouro_ocert_counters *counters, uint64_t *counter_out, uint8_t *present_out,
    uint8_t *ledger, uint32_t *pool_row, const ouro_pbft_views *pbft_views,
    const ouro_pbft_state *pbft_state_in, uint8_t *signer_id_out, uint64_t *signer_slot_out,
    size_t *n_out, uint8_t *pbft, uint32_t *genesis_row_pbft, uint64_t *signed_count);
int ouro_chain_validate_ledger_pbft_cbor_host(
    const uint8_t *raw, size_t raw_bytes, const uint64_t *off, const uint32_t *len, size_t n,
    uint64_t slots_per_kes_period, int64_t protocol_magic, const ouro_epoch_nonces *epochs,
    const uint8_t *eta_alpha, const uint8_t *leader_alpha, const ouro_envelope_cfg *cfg,
    const ouro_chain_tip *tip_in, uint8_t *proto, uint8_t *status, uint8_t *verdict,
    uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce, uint8_t *header_hash,
    uint8_t *envelope, ouro_chain_tip *tip_out, const ouro_ledger_views *views,
    const ouro_genesis_delegs *genesis, const ouro_ledger_globals *globals,
    const ouro_ocert_counters *counters, uint64_t *counter_out, uint8_t *present_out,
    uint8_t *ledger, uint32_t *pool_row, const ouro_pbft_views *pbft_views,
    const ouro_pbft_state *pbft_state_in, uint8_t *signer_id_out, uint64_t *signer_slot_out,
    size_t *n_out, uint8_t *pbft, uint32_t *genesis_row_pbft, uint64_t *signed_count);

/* (How ouro_byron_verify_cbor runs, since round 6: on the raw-CBOR pipeline
 * of ouro_tpraos_verify_cbor -- chunks gathered into pinned NUMA-local
 * staging, the device Byron slicer (the same cbor_byron.h parse as
 * ouro_byron_pack_cbor) and the ByronDSIGN Ed25519 kernel per chunk, 5
 * chunks in flight; a device error recomputes the batch on the host path.
 * OURO_EINVAL as for ouro_byron_pack_cbor.) */

/* Byron heavyweight delegation certificates (the "Byron delegation" use of
 * DSIGN in the north star): a certificate (epoch, issuer XPub, delegate XPub,
 * signature) -- cardano-ledger-byron's Delegation.Certificate [ext], the
 * reference's PBftDelegationCert (ouroboros-consensus-byron/src/Ouroboros/
 * Consensus/Byron/Protocol.hs:30) and the mempool's ByronDlg payload
 * (.../Byron/Ledger/Mempool.hs:90), whose signature the ledger checks under
 * the issuer's key with the SignCertificate tag.  Signed bytes, pinned on the
 * certificate inside the reference's golden Byron header
 * (tests/test_byron_cert.py):
 *   0x0a || CBOR(protocol_magic) || CBOR bytes("00" || delegate XPub || CBOR(epoch))
 * Key = issuer XPub[0:32]; ByronDSIGN acceptance (ouro_byron_ed25519_verify).
 * _message writes those bytes (at most OURO_BYRON_DLG_MSG_MAX) and returns
 * their length (0 for NULL arguments); _verify is one certificate on the
 * host path (0 / -1 / <= -2 as ouro_byron_ed25519_verify); _verify_batch
 * builds the n messages and runs ouro_byron_ed25519_verify_batch
 * (verdict[i] = 1 / 0). */
#define OURO_BYRON_DLG_MSG_MAX 96
size_t ouro_byron_dlg_cert_message(uint8_t *out, uint32_t protocol_magic,
                                   const uint8_t *delegate_xpub /* 64 */, uint64_t epoch);
int ouro_byron_dlg_cert_verify(uint32_t protocol_magic, const uint8_t *issuer_xpub /* 64 */,
                               const uint8_t *delegate_xpub /* 64 */, uint64_t epoch,
                               const uint8_t *sig /* 64 */);
int ouro_byron_dlg_cert_verify_batch(size_t n, uint32_t protocol_magic,
                                     const uint8_t *issuer_xpub /* n x 64 */,
                                     const uint8_t *delegate_xpub /* n x 64 */,
                                     const uint64_t *epoch, const uint8_t *sig /* n x 64 */,
                                     uint8_t *verdict);

/* The host-side UPDN fold (ledger-specs; the per-header step of
 * SL.updateChainDepState after the crypto): for i = 0..n-1
 *   eta_v <- eta_v (*) eta_nonce[i]
 *   eta_c <- eta_v            if slot[i] + stability_window < first_slot_next_epoch
 *            (unchanged)      otherwise
 * with a (*) b = Blake2b-256(a || b) (Nonce composition; the 32-byte values are
 * Nonce hashes).  The caller stops at the first invalid header itself (pass
 * n = that index).  eta_v / eta_c are updated in place (32 B each);
 * is_neutral[0..1] (may be NULL) say eta_v / eta_c start as NeutralNonce and
 * receive whether they still are.  Host-only, no device.  Returns OURO_OK. */
int ouro_nonce_fold(size_t n, const uint8_t *eta_nonce, const uint64_t *slot,
                    uint64_t first_slot_next_epoch, uint64_t stability_window,
                    uint8_t *eta_v, uint8_t *eta_c, int *is_neutral);

/* Latency-oriented variant for small batches (ChainSync windows of up to 300
 * pipelined headers, ouroboros-network/src/Ouroboros/Network/NodeToNode.hs:197-200):
 * the checks of a header run on eight lanes concurrently (each VRF's
 * V = [s]H - [c]Gamma split over two), then one finish pass.  Same verdicts and outputs as ouro_tpraos_verify_batch. */
int ouro_tpraos_verify_batch_lowlat(const ouro_tpraos_batch *b, uint8_t *verdict,
                                    uint8_t *beta_eta, uint8_t *beta_leader);

/* One process, several GPUs: the batch is cut into
 * contiguous shards, shard k verified on devices[k] (devices = NULL: every
 * visible device) by a persistent worker thread -- one per (device, k-th
 * listing of that device) -- with its own streams and pinned staging (the
 * pipelined path of ouro_tpraos_verify_batch), writing straight into the
 * caller's buffers (no collective is needed inside one process).  A device
 * may be listed more than once (two pipelines on one GPU).  The workers are
 * pooled per device: a call borrows one per shard and returns it when every
 * shard has finished, so concurrent callers (ChainSync windows beside
 * ChainDB's suffix re-validation) run at once on workers of their own --
 * nothing is serialised process-wide since round 6.  The first shard error
 * is returned after every shard has finished (a shard's device error is
 * recomputed on the host path like any host-buffer batch).  Same results as
 * ouro_tpraos_verify_batch. */
int ouro_device_count(void);
/* NUMA placement (each GPU's pinned staging NUMA-local).
 * ouro_device_numa_node: the node of the device's PCI function in sysfs
 * (-1 unknown; OURO_ENODEV for a bad index).  ouro_bind_thread_to_device:
 * restricts the calling thread to that node's CPUs (within the process's
 * cpuset) and prefers its memory, so the pinned staging the thread allocates
 * afterwards lands there; returns the node or -1 (left alone).  The workers of
 * ouro_tpraos_verify_batch_multi bind themselves to their device's node; all
 * pinned staging is allocated with hipHostMallocNumaUser (the allocating
 * thread's policy).  ouro_debug_multi_workers: per worker its device, node and
 * the CPUs it is bound to (0 = unbound; declared in ouro_verify_debug.h). */
int ouro_device_numa_node(int device);
int ouro_bind_thread_to_device(int device);
int ouro_tpraos_verify_batch_multi(const ouro_tpraos_batch *b, const int *devices, int ndev,
                                   uint8_t *verdict, uint8_t *beta_eta, uint8_t *beta_leader);
/* The raw-CBOR entries over several GPUs of one process -- what the bulk
 * callers of an 8-GPU node hold: ChainDB's re-validation of a stored suffix
 * (ouroboros-consensus/src/Ouroboros/Consensus/Storage/ChainDB/Impl/
 * LgrDB.hs:350-368) and ImmutableDB / VolatileDB integrity
 * (.../Storage/ImmutableDB/Impl/Validation.hs:358-365,
 * .../Storage/VolatileDB/Impl/Parser.hs:66-85).  Arguments and results as
 * ouro_tpraos_verify_cbor / ouro_integrity_verify_cbor /
 * ouro_byron_verify_cbor, plus the device list (NULL: every visible
 * device; a device may be listed more than once).  Headers are cut into
 * contiguous shards of ceil(n / ndev), shard k runs the one-device pipeline
 * (chunks, pinned NUMA-local staging, several chunks in flight) on a pooled
 * worker of devices[k] bound to that GPU's NUMA node, and writes straight into
 * the caller's buffers.  Every span is checked before any shard starts
 * (OURO_EINVAL); OURO_ENODEV for a device index outside the visible ones. */
int ouro_tpraos_verify_cbor_multi(const int *devices, int ndev, const uint8_t *raw,
                                  size_t raw_bytes, const uint64_t *off, const uint32_t *len,
                                  size_t n, uint64_t slots_per_kes_period,
                                  const uint8_t *epoch_nonce, const uint8_t *eta_alpha,
                                  const uint8_t *leader_alpha, uint8_t *status, uint8_t *verdict,
                                  uint8_t *beta_eta, uint8_t *beta_leader, uint8_t *eta_nonce);
int ouro_integrity_verify_cbor_multi(const int *devices, int ndev, const uint8_t *raw,
                                     size_t raw_bytes, const uint64_t *off, const uint32_t *len,
                                     size_t n, uint64_t slots_per_kes_period, uint8_t *status,
                                     uint8_t *verdict);
int ouro_byron_verify_cbor_multi(const int *devices, int ndev, const uint8_t *raw,
                                 size_t raw_bytes, const uint64_t *off, const uint32_t *len,
                                 size_t n, int64_t protocol_magic, uint8_t *status,
                                 uint8_t *verdict);

/* A plan for repeated fixed-capacity batches: pinned staging, device buffers
 * and the latency kernel's launch shape fixed at create; each run issues the
 * window's input copy kernel and the fused latency kernel on the plan's own
 * stream (OURO_PLAN_GRAPH=1 at create: replayed from one captured hipGraph
 * instead).  A plan is used by one thread at a time; any n <= max_headers per
 * run. */
typedef struct ouro_tpraos_plan ouro_tpraos_plan;
ouro_tpraos_plan *ouro_tpraos_plan_create(size_t max_headers, size_t max_body_bytes);
int ouro_tpraos_plan_run(ouro_tpraos_plan *plan, const ouro_tpraos_batch *b, uint8_t *verdict,
                         uint8_t *beta_eta, uint8_t *beta_leader);
void ouro_tpraos_plan_destroy(ouro_tpraos_plan *plan);

/* Asynchronous form of ouro_tpraos_plan_run for pipelined ChainSync windows
 * (SURVEY.md §8(b) "Async": a client keeps up to 300 headers in flight,
 * ouroboros-network/src/Ouroboros/Network/NodeToNode.hs:197-200, and
 * validates each window as its headers arrive,
 * ouroboros-consensus/src/Ouroboros/Consensus/MiniProtocol/ChainSync/Client.hs:792).
 * submit copies the batch into the plan's pinned staging and launches its
 * kernels, returning at once (the caller's input buffers are free again on
 * return); wait blocks until that batch's results are in the caller's buffers.
 * One batch in flight per plan: a second submit before wait, or a wait with
 * nothing submitted, returns OURO_EINVAL.  Several plans = several windows in
 * flight, each on its own stream. */
int ouro_tpraos_plan_submit(ouro_tpraos_plan *plan, const ouro_tpraos_batch *b);
int ouro_tpraos_plan_wait(ouro_tpraos_plan *plan, uint8_t *verdict, uint8_t *beta_eta,
                          uint8_t *beta_leader);

/* (A plan's latency kernel counts each header's finished checks in
 * per-header arrival counters tagged with the launch's generation -- a new
 * one per submit -- so a counter an earlier launch left mid-count, one that
 * never completed, is never counted again; tests/test_gpu_claims.py checks it
 * through a test hook reached only from the environment.) */

/* ------------------------------------------------------- host path ----- */
/* The same batches on the library's host path, explicitly: the kernels' own
 * lane routines compiled for the CPU (csrc/host_path.hip), the batch split
 * over host threads (OURO_HOST_THREADS caps them; default the CPUs the
 * process may run on, at most 64).  Same arguments, verdicts and outputs as
 * the calls without _host; no device is touched.  For nodes without a GPU,
 * for callers that keep small batches on the CPU, and the path the device
 * calls recompute on after a device error. */
int ouro_ed25519_verify_batch_host(size_t n, const uint8_t *pk, const uint8_t *sig,
                                   const uint8_t *msg, const uint64_t *msg_off,
                                   const uint32_t *msg_len, uint8_t *verdict);
int ouro_byron_ed25519_verify_batch_host(size_t n, const uint8_t *pk, const uint8_t *sig,
                                         const uint8_t *msg, const uint64_t *msg_off,
                                         const uint32_t *msg_len, uint8_t *verdict);
int ouro_vrf03_verify_batch_host(size_t n, const uint8_t *pk, const uint8_t *proof,
                                 const uint8_t *alpha, const uint64_t *alpha_off,
                                 const uint32_t *alpha_len, uint8_t *beta, uint8_t *verdict,
                                 uint32_t flags);
int ouro_sum6kes_verify_batch_host(size_t n, const uint8_t *vk, const uint32_t *t,
                                   const uint8_t *msg, const uint64_t *msg_off,
                                   const uint32_t *msg_len, const uint8_t *sig, uint8_t *verdict);
int ouro_tpraos_verify_batch_host(const ouro_tpraos_batch *b, uint8_t *verdict,
                                  uint8_t *beta_eta, uint8_t *beta_leader);
int ouro_tpraos_verify_batch_epochs_host(const ouro_tpraos_batch *b, const ouro_epoch_nonces *e,
                                         uint8_t *verdict, uint8_t *beta_eta,
                                         uint8_t *beta_leader);
int ouro_leader_check_batch_host(size_t n, const uint8_t *beta, const uint64_t *sigma_num,
                                 const uint64_t *sigma_den, int64_t act_log_hi,
                                 uint64_t act_log_lo, int f_is_one, uint8_t *verdict);

/* ---------------------------------------------- leader threshold ----- */
/* ledger-specs checkLeaderValue (shelley-spec-ledger BlockChain.hs), called by
 * meetsLeaderThreshold, ouroboros-consensus-shelley/src/Ouroboros/Consensus/
 * Shelley/Protocol.hs:473-491: is the leader VRF output beta (64 B) below
 * 1 - (1 - f)^sigma, decided with shelley-spec-non-integral's taylorExpCmp in
 * 34-digit fixed point.  sigma = sigma_num[i] / sigma_den[i] (the pool's
 * relative stake, 0 <= sigma <= 1); f is given as its ActiveSlotCoeff fields:
 * unActiveSlotLog (a signed 128-bit integer, act_log_hi:act_log_lo; the
 * reference precomputes it from f) and whether f is exactly 1.
 * verdict[i] = OURO_LEADER_YES / OURO_LEADER_NO, or OURO_LEADER_BADARG when
 * sigma or unActiveSlotLog is outside the supported domain
 * (-8 * 10^34 <= unActiveSlotLog <= 0, i.e. f <= 1 - e^-8). */
#define OURO_LEADER_NO 0u
#define OURO_LEADER_YES 1u
#define OURO_LEADER_BADARG 0xffu
int ouro_leader_check_batch(size_t n, const uint8_t *beta, const uint64_t *sigma_num,
                            const uint64_t *sigma_den, int64_t act_log_hi,
                            uint64_t act_log_lo, int f_is_one, uint8_t *verdict);

/* ----------------------------------- batch, device-resident buffers ----- */
/* Same kernels on caller-owned device memory, enqueued on `stream` (a
 * hipStream_t; NULL = HIP's default stream) and NOT synchronised: the caller
 * orders its own copies/events around them.  `msg_off`/`msg_len` etc. are
 * device pointers too.  Used by bench.py (inputs resident in HBM) and by
 * pipelined callers that overlap H2D of the next window with this one. */

int ouro_ed25519_verify_batch_device(void *stream, size_t n, const uint8_t *pk,
                                     const uint8_t *sig, const uint8_t *msg,
                                     const uint64_t *msg_off, const uint32_t *msg_len,
                                     uint8_t *verdict);
int ouro_byron_ed25519_verify_batch_device(void *stream, size_t n, const uint8_t *pk,
                                           const uint8_t *sig, const uint8_t *msg,
                                           const uint64_t *msg_off, const uint32_t *msg_len,
                                           uint8_t *verdict);
int ouro_vrf03_verify_batch_device(void *stream, size_t n, const uint8_t *pk,
                                   const uint8_t *proof, const uint8_t *alpha,
                                   const uint64_t *alpha_off, const uint32_t *alpha_len,
                                   uint8_t *beta, uint8_t *verdict);
int ouro_vrf03_verify_batch_device_flags(void *stream, size_t n, const uint8_t *pk,
                                         const uint8_t *proof, const uint8_t *alpha,
                                         const uint64_t *alpha_off, const uint32_t *alpha_len,
                                         uint8_t *beta, uint8_t *verdict, uint32_t flags);
int ouro_sum6kes_verify_batch_device(void *stream, size_t n, const uint8_t *vk,
                                     const uint32_t *t, const uint8_t *msg,
                                     const uint64_t *msg_off, const uint32_t *msg_len,
                                     const uint8_t *sig, uint8_t *verdict);
/* `b` is a host struct whose pointers are device pointers */
int ouro_tpraos_verify_batch_device(void *stream, const ouro_tpraos_batch *b,
                                    uint8_t *verdict, uint8_t *beta_eta,
                                    uint8_t *beta_leader);
int ouro_leader_check_batch_device(void *stream, size_t n, const uint8_t *beta,
                                   const uint64_t *sigma_num, const uint64_t *sigma_den,
                                   int64_t act_log_hi, uint64_t act_log_lo, int f_is_one,
                                   uint8_t *verdict);

/* ---- The forging side: PraosVRF evalCertified and checkIsLeader -------------
 *
 * The other half of the reference's `ConsensusProtocol (TPraos c)` instance:
 * checkIsLeader (ouroboros-consensus-shelley/src/Ouroboros/Consensus/Shelley/
 * Protocol.hs:366-413) evaluates the leader VRF on mkSeed seedL slot eta0 with
 * the pool's VRF signing key (VRF.evalCertified), decides meetsLeaderThreshold
 * (:473-491) or the overlay branch (lookupInOverlaySchedule, :368-399), and
 * hands back the two certified VRFs a forged header carries.  A pool operator
 * runs it once per epoch over all of the epoch's slots.  KES signing and block
 * forging are not offered.
 *
 * Every entry validates its arguments before anything runs (OURO_EINVAL: a
 * NULL array with nonzero n; a span outside alpha_bytes; nkeys not 1 or n;
 * sigma or act_log outside ouro_leader_check_batch's domain; d_num > d_den,
 * d_den == 0, or d_num > 0 with asc_inv == 0, ngen == 0 or first_slot before
 * epoch_first_slot; a slot range whose last slot passes 2^64 - 1).  n == 0
 * returns OURO_OK.  A device error recomputes on the host path as for every
 * other host-buffer batch, unless OURO_ON_DEVICE_ERROR=fail.  The *_host
 * entries run the same lane routines on the host's worker pool.
 *
 * A VRF signing key is libsodium's: sk = seed (32) || pk (32).  The scalar is
 * SHA-512(seed)[0:32], clamped; the public key bytes are used AS GIVEN, as
 * crypto_vrf_ietfdraft03_prove does (it never recomputes the key).
 *
 * KEY HYGIENE.  A key and its expansion live in call-local host memory, in a
 * launch's arguments, or in a device buffer this call owns.  Before the call
 * returns the library zeroes every buffer of its own that held them: the
 * launch's argument block, the key's staging buffer on the device, the
 * scalars and recoding carries in the per-lane scratch slots, and, on the
 * host path, the prover's locals (the expanded key, the nonce and what it was
 * hashed from, the unreduced k + c x).  Nothing of a key reaches
 * ouro_last_error.  Outside the library's reach, and not claimed: copies the
 * compiler makes (registers, spill slots, inlined temporaries such as a hash's
 * message schedule) on the host or the device, the device's registers and the
 * memory the HIP runtime manages for their spills, and the runtime's own
 * staging of a host-to-device copy.  NO
 * constant-time or side-channel claim is made: the device and host routines
 * index per-lane tables by digits of the secret scalar and branch on them.
 * These entries are for a machine that already holds the key.
 *
 * Pinned: the IETF draft-03 vectors, the oracle's prover and a prover built
 * from libsodium 1.0.18's primitives, byte for byte (tests/test_prove_rule.py).
 * Not pinned: mkSeed's composition and checkLeaderValue stay "parity unpinned"
 * as for the verifying entries; the overlay classification is pinned only to
 * the Python restatement (ledger.py). */

/* n certified VRFs.  sk: nkeys x 64, nkeys = 1 (one key for every item) or n.
 * alpha of item i: alpha[alpha_off[i] .. + alpha_len[i]).  proof: n x 80;
 * beta (may be NULL): n x 64, the outputs (proof_to_hash of each proof). */
int ouro_vrf03_prove_batch(size_t n, const uint8_t *sk, size_t nkeys, const uint8_t *alpha,
                           size_t alpha_bytes, const uint64_t *alpha_off,
                           const uint32_t *alpha_len, uint8_t *proof, uint8_t *beta);
int ouro_vrf03_prove_batch_host(size_t n, const uint8_t *sk, size_t nkeys, const uint8_t *alpha,
                                size_t alpha_bytes, const uint64_t *alpha_off,
                                const uint32_t *alpha_len, uint8_t *proof, uint8_t *beta);
/* one proof on the host path (crypto_vrf_ietfdraft03_prove's arguments) */
int ouro_vrf03_prove(uint8_t proof[80], const uint8_t sk[64], const uint8_t *m, size_t mlen);
/* pk = [clamp(SHA-512(seed)[0:32])]B and sk = seed || pk, on the host path
 * (crypto_vrf_ietfdraft03_keypair_from_seed's arguments) */
int ouro_vrf03_keypair_from_seed(uint8_t pk[32], uint8_t sk[64], const uint8_t seed[32]);

/* checkIsLeader for slots first_slot .. first_slot + n_slots - 1 of one epoch */
#define OURO_SLOT_NOT_LEADER 0u
#define OURO_SLOT_LEADER 1u           /* a Praos slot, meetsLeaderThreshold */
#define OURO_SLOT_OVERLAY_ACTIVE 2u   /* gen_index[i] = the scheduled genesis key's index */
#define OURO_SLOT_OVERLAY_INACTIVE 3u /* NonActiveSlot: nobody may forge */
typedef struct ouro_leader_params {
  const uint8_t *epoch_nonce; /* 32 B, NULL = NeutralNonce */
  uint64_t epoch_first_slot;  /* overlay positions count from here; read only when d_num > 0 */
  uint64_t sigma_num;         /* the pool's relative stake */
  uint64_t sigma_den;
  int64_t act_log_hi;         /* as ouro_leader_check_batch */
  uint64_t act_log_lo;
  int f_is_one;
  uint64_t d_num;             /* decentralisation parameter; d_num = 0: no overlay */
  uint64_t d_den;
  uint64_t asc_inv;           /* as ouro_genesis_delegs; read only when d_num > 0 */
  uint32_t ngen;              /* genesis keys of the epoch; read only when d_num > 0 */
} ouro_leader_params;
/* cls: n_slots bytes, OURO_SLOT_*.  gen_index (may be NULL): n_slots, the
 * index on an OURO_SLOT_OVERLAY_ACTIVE slot, OURO_LV_NO_POOL elsewhere --
 * whether the pool is that key's delegate is the caller's map lookup
 * (:385-399).  beta_leader (may be NULL): n_slots x 64, the leader VRF's
 * output, filled for EVERY class (on an overlay slot the reference evaluates
 * it "as normal"; no threshold applies there).  The host sits between this
 * call and ouro_tpraos_leader_vrfs on purpose: the winners are a few percent
 * of the slots. */
int ouro_tpraos_leader_schedule(const uint8_t vrf_sk[64], const ouro_leader_params *p,
                                uint64_t first_slot, size_t n_slots, uint8_t *cls,
                                uint32_t *gen_index, uint8_t *beta_leader);
int ouro_tpraos_leader_schedule_host(const uint8_t vrf_sk[64], const ouro_leader_params *p,
                                     uint64_t first_slot, size_t n_slots, uint8_t *cls,
                                     uint32_t *gen_index, uint8_t *beta_leader);
/* TPraosIsLeader's two certified VRFs for m chosen slots (rho and y of
 * Protocol.hs:409-413): the proofs of mkSeed seedEta / seedL slot[j]
 * epoch_nonce (NULL = NeutralNonce), m x 80 each, and their outputs, m x 64
 * each (either may be NULL). */
int ouro_tpraos_leader_vrfs(const uint8_t vrf_sk[64], const uint8_t *epoch_nonce, size_t m,
                            const uint64_t *slot, uint8_t *eta_proof, uint8_t *eta_output,
                            uint8_t *leader_proof, uint8_t *leader_output);
int ouro_tpraos_leader_vrfs_host(const uint8_t vrf_sk[64], const uint8_t *epoch_nonce, size_t m,
                                 const uint64_t *slot, uint8_t *eta_proof, uint8_t *eta_output,
                                 uint8_t *leader_proof, uint8_t *leader_output);

#ifdef __cplusplus
}
#endif
#endif /* OURO_VERIFY_H */
