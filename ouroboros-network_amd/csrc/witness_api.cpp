// witness_api.cpp -- transaction key witnesses from raw block CBOR
// (include/ouro_verify.h ouro_block_witness_*; cbor_witness.h): the Shelley
// description of witness_flow.h's flow and the C entries over it.  Host code
// only: kernels are reached through launches.h.
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <vector>

#include "../../include/ouro_verify.h"
#include "cbor_witness.h"
#include "knobs.h"
#include "launch.h"
#include "witness_flow.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

struct Shelley {
  using Out = ouro_block_witness_out;
  using Rows = cbor::WitRows;
  static constexpr size_t kKey = 32;
  static constexpr bool kBlockMagic = false, kEbbOk = false;
  static constexpr uint8_t kAllOk = OURO_WIT_ALL_OK;
  static constexpr auto count = launch_witness_count;
  static constexpr auto scan = launch_witness_scan;
  static constexpr auto emit = launch_witness_emit;
  static constexpr auto verify = launch_witness_verify;
  static constexpr auto finish = launch_witness_finish;
  static size_t budget() { return group_budget(ouro_knobs::get().witness_group_bytes); }
  static int magic_check(int64_t) { return OURO_OK; }  // (no magic in this era's entries)
  static uint8_t count_one(const uint8_t* raw, uint64_t base, uint32_t len, uint32_t* ntx,
                           uint32_t* nwit) {
    return cbor::witness_count_one(raw, base, len, ntx, nwit);
  }
  static void emit_one(const uint8_t* raw, uint64_t base, uint32_t len, const Rows& r, uint64_t tx0,
                       uint64_t wit0, uint32_t ntx, uint32_t nwit, int64_t, uint64_t*) {
    cbor::witness_emit_one(raw, base, len, r, tx0, wit0, ntx, nwit);
  }
  // plain Ed25519 over the row's transaction id, in place in o.tx_id
  static int verify_host(const WitnessHostRows<Out>& h) {
    std::vector<uint64_t> msg_off(h.W);
    std::vector<uint32_t> msg_len(h.W, 32);
    for (size_t r = 0; r < h.W; r++) msg_off[r] = 32 * (uint64_t)h.o.wit_tx[r];
    if (int rc = h.W ? ouro_host::ed_batch(h.W, h.vk, h.sig, h.o.tx_id, msg_off.data(),
                                           msg_len.data(), h.o.wit_ok, 0)
                     : 0)
      return fail(rc, "witness host path failed");
    return OURO_OK;
  }
};
using Flow = WitnessFlow<Shelley>;
constexpr int64_t kNoMagic = -1;

}  // namespace

extern "C" {

int ouro_block_witness_count_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                  const uint32_t* len, size_t n, uint8_t* status, uint32_t* ntx,
                                  uint32_t* nwit) {
  return Flow::count_call(raw, raw_bytes, off, len, n, kNoMagic, status, ntx, nwit, false);
}

int ouro_block_witness_count_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                       const uint32_t* len, size_t n, uint8_t* status,
                                       uint32_t* ntx, uint32_t* nwit) {
  return Flow::count_call(raw, raw_bytes, off, len, n, kNoMagic, status, ntx, nwit, true);
}

int ouro_block_witness_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                   const uint32_t* len, size_t n,
                                   const ouro_block_witness_out* out, uint8_t* status,
                                   uint8_t* verdict, uint32_t* n_bad) {
  return Flow::verify_call(raw, raw_bytes, off, len, n, kNoMagic, out, status, verdict, n_bad,
                           false);
}

int ouro_block_witness_verify_cbor_host(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                        const uint32_t* len, size_t n,
                                        const ouro_block_witness_out* out, uint8_t* status,
                                        uint8_t* verdict, uint32_t* n_bad) {
  return Flow::verify_call(raw, raw_bytes, off, len, n, kNoMagic, out, status, verdict, n_bad,
                           true);
}

size_t ouro_block_witness_work_bytes(size_t n, size_t tx_cap, size_t wit_cap) {
  return Flow::work_bytes(n, tx_cap, wit_cap);
}

int ouro_block_witness_verify_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                          const uint64_t* off, const uint32_t* len, size_t n,
                                          const ouro_block_witness_out* out, void* work,
                                          size_t work_bytes, uint8_t* status, uint8_t* verdict,
                                          uint32_t* n_bad) {
  return Flow::device_call(stream, raw, raw_bytes, off, len, n, kNoMagic, out, work, work_bytes,
                           status, verdict, n_bad);
}

}  // extern "C"
