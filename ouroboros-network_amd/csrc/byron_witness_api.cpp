// byron_witness_api.cpp -- Byron transaction witnesses from raw block CBOR
// (include/ouro_verify.h ouro_byron_block_witness_*; cbor_byron_witness.h): the
// Byron description of witness_flow.h's flow and the C entries over it.  What
// differs from witness_api.cpp's: the magic, the 64-byte key rows, the message
// (built per row, not the bare tx id) and the EBB's verdict.  Host code only:
// kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <cstring>
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor_byron_witness.h"
#include "knobs.h"
#include "launch.h"
#include "witness_flow.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

constexpr uint32_t kMsgSlot = 40;  // a signed message has at most 8 + 32 bytes

struct Byron {
  using Out = ouro_byron_block_witness_out;
  using Rows = cbor::BywRows;
  static constexpr size_t kKey = 64;
  static constexpr bool kBlockMagic = true, kEbbOk = true;
  static constexpr uint8_t kAllOk = OURO_BYW_ALL_OK;
  static constexpr auto count = launch_byron_witness_count;
  static constexpr auto scan = launch_byron_witness_scan;
  static constexpr auto emit = launch_byron_witness_emit;
  static constexpr auto verify = launch_byron_witness_verify;
  static constexpr auto finish = launch_byron_witness_finish;
  static size_t budget() { return group_budget(ouro_knobs::get().byron_witness_group_bytes); }
  static int magic_check(int64_t magic) {
    if (magic < -1 || magic > (int64_t)cbor::kWord32Max)
      return fail(OURO_EINVAL, "protocol_magic outside -1 .. 2^32 - 1");
    return OURO_OK;
  }
  static uint8_t count_one(const uint8_t* raw, uint64_t base, uint32_t len, uint32_t* ntx,
                           uint32_t* nwit) {
    return cbor::byron_witness_count_one(raw, base, len, ntx, nwit);
  }
  // ... and the magic the block's messages use: the configured one, or the
  // header's own field
  static void emit_one(const uint8_t* raw, uint64_t base, uint32_t len, const Rows& r, uint64_t tx0,
                       uint64_t wit0, uint32_t ntx, uint32_t nwit, int64_t magic, uint64_t* bmagic) {
    cbor::byron_witness_emit_one(raw, base, len, r, tx0, wit0, ntx, nwit, bmagic);
    if (magic >= 0) *bmagic = (uint64_t)magic;
  }
  // ByronDSIGN under the 32-byte key prefix over the rows' messages, built in
  // slots of kMsgSlot bytes (the blocks that fit own rows 0 .. W)
  static int verify_host(const WitnessHostRows<Out>& h) {
    std::vector<uint64_t> msg_off(h.W);
    std::vector<uint32_t> msg_len(h.W);
    std::vector<uint8_t> pk(32 * h.W), msg(kMsgSlot * h.W);
    if (int rc = host_rows(h.n, 64, [&](size_t lo, size_t hi) {
          for (size_t i = lo; i < hi; i++) {
            if (h.status[i] != OURO_PACK_OK) continue;
            for (uint64_t r = h.o.wit_begin[i]; r < h.o.wit_begin[i] + h.nwit[i]; r++) {
              msg_off[r] = kMsgSlot * r;
              msg_len[r] =
                  cbor::byron_witness_message(msg.data() + kMsgSlot * r, h.o.wit_kind[r],
                                              h.bmagic[i], h.o.tx_id + 32 * (size_t)h.o.wit_tx[r]);
              memcpy(pk.data() + 32 * r, h.vk + 64 * r, 32);
            }
          }
        }))
      return rc;
    if (int rc = h.W ? ouro_host::ed_batch(h.W, pk.data(), h.sig, msg.data(), msg_off.data(),
                                           msg_len.data(), h.o.wit_ok, 1)
                     : 0)
      return fail(rc, "Byron witness host path failed");
    return OURO_OK;
  }
};
using Flow = WitnessFlow<Byron>;

}  // namespace

extern "C" {

int ouro_byron_block_witness_count_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                        const uint32_t* len, size_t n, int64_t protocol_magic,
                                        uint8_t* status, uint32_t* ntx, uint32_t* nwit) {
  return Flow::count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, nwit, false);
}

int ouro_byron_block_witness_count_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                             const uint64_t* off, const uint32_t* len, size_t n,
                                             int64_t protocol_magic, uint8_t* status,
                                             uint32_t* ntx, uint32_t* nwit) {
  return Flow::count_call(raw, raw_bytes, off, len, n, protocol_magic, status, ntx, nwit, true);
}

int ouro_byron_block_witness_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                         const uint32_t* len, size_t n, int64_t protocol_magic,
                                         const ouro_byron_block_witness_out* out, uint8_t* status,
                                         uint8_t* verdict, uint32_t* n_bad) {
  return Flow::verify_call(raw, raw_bytes, off, len, n, protocol_magic, out, status, verdict, n_bad,
                     false);
}

int ouro_byron_block_witness_verify_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                              const uint64_t* off, const uint32_t* len, size_t n,
                                              int64_t protocol_magic,
                                              const ouro_byron_block_witness_out* out,
                                              uint8_t* status, uint8_t* verdict, uint32_t* n_bad) {
  return Flow::verify_call(raw, raw_bytes, off, len, n, protocol_magic, out, status, verdict, n_bad, true);
}

size_t ouro_byron_block_witness_work_bytes(size_t n, size_t tx_cap, size_t wit_cap) {
  return Flow::work_bytes(n, tx_cap, wit_cap);
}

int ouro_byron_block_witness_verify_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                                const uint64_t* off, const uint32_t* len, size_t n,
                                                int64_t protocol_magic,
                                                const ouro_byron_block_witness_out* out, void* work,
                                                size_t work_bytes, uint8_t* status,
                                                uint8_t* verdict, uint32_t* n_bad) {
  return Flow::device_call(stream, raw, raw_bytes, off, len, n, protocol_magic, out, work,
                           work_bytes, status, verdict, n_bad);
}

}  // extern "C"
