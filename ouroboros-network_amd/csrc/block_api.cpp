// block_api.cpp -- whole-block storage integrity and the batched Blake2b-256
// (include/ouro_verify.h): the device sequence over blocks in device memory
// (block_launch: slicer, segment hashes, Sum6KES, finish), the host path over
// the same batch (block_host), and the C entries.  Host code only: kernels
// are reached through launches.h.  The host-buffer block entry runs on the
// raw-CBOR pipeline of raw_pipe.cpp (raw_call.h RawKind kRawBlock).
// its own host copies of the out-of-line lane routines (common.h)
#define OURO_NI_LINKAGE static
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ouro_verify.h"
#include "blake2b_stream.h"
#include "cbor_block.h"
#include "host_path.h"
#include "host_util.h"
#include "knobs.h"
#include "launch.h"
#include "launches.h"
#include "raw_call.h"

using namespace ouro;
using namespace ouro_rt;

namespace {

int b2b_host(size_t n, const uint8_t* msg, const uint64_t* off, const uint32_t* len,
             uint8_t* out) {
  return host_rows(n, 256, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      uint32_t d[8];
      blake2b256_stream(d, msg + off[i], len[i]);
      digest_bytes(out + 32 * i, d);
    }
  });
}

int b2b_check(size_t n, const uint8_t* msg, size_t msg_bytes, const uint64_t* off,
              const uint32_t* len, uint8_t* out) {
  if (!off || !len || !out) return fail(OURO_EINVAL, "null argument");
  if (!msg && msg_bytes) return fail(OURO_EINVAL, "null message buffer");
  return spans_check("message", "msg_bytes", msg_bytes, off, len, n);
}

// one upload, the hash kernel and one copy-back on the calling thread's stream
int b2b_dev(size_t n, const uint8_t* msg, const uint64_t* off, const uint32_t* len, uint8_t* out) {
  hipStream_t st;
  int rc = thread_stream(&st);
  if (rc) return rc;
  Window w;
  if ((rc = window_of(n, off, len, &w))) return rc;
  Stager sg{st};
  auto dmsg = sg.up(w.span() ? msg + w.lo : msg, w.span());
  auto doff = sg.up(w.off.data(), n);
  auto dlen = sg.up(len, n);
  auto dout = sg.out<uint8_t>(32 * n);
  auto dwork = sg.out<uint8_t>(cbor::b2b_work_bytes(n));
  if (sg.rc) return sg.rc;
  if ((rc = launch_blake2b(st, n, dmsg, w.span(), doff, dlen, dout, dwork))) return rc;
  std::vector<uint8_t> tv(32 * n);
  if ((rc = download(st, tv.data(), dout, 32 * n))) return rc;
  if ((rc = finish(st))) return rc;
  memcpy(out, tv.data(), 32 * n);
  return OURO_OK;
}

}  // namespace

namespace ouro_rt {

// The device sequence of whole-block integrity over n blocks in device
// memory, on `st`: the block slicer into the arena at `a` (64-byte aligned,
// cbor::block_layout(n)), the three segment hashes per block (3n messages,
// ordered by length class), Sum6KES over the sliced header rows (the message
// is the header_body span inside the block), and the finish.
int block_launch(hipStream_t st, const uint8_t* draw, size_t raw_bytes, const uint64_t* doff,
                 const uint32_t* dlen, size_t n, uint64_t spkp, uint8_t* a, uint8_t* dstatus,
                 uint8_t* dverdict, uint8_t* dbody_hash) {
  const cbor::BlockLayout L = cbor::block_layout(n);
  const cbor::Out o = cbor::arena_out(a + L.hdr, n, nullptr, nullptr);
  const cbor::BlockOut bo = cbor::block_arena_out(a, L);
  const unsigned blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
  launch_block_pack(st, blocks, draw, raw_bytes, doff, dlen, n, spkp, o, bo, dstatus);
  int rc;
  if ((rc = launch_check())) return rc;
  if ((rc = launch_blake2b(st, 3 * n, draw, raw_bytes, bo.seg_off, bo.seg_len, a + L.digest,
                           a + L.work)))
    return rc;
  if ((rc = launch_kes(st, n, o.hot_vk, o.kes_t, draw, o.body_off, o.body_len, o.kes_sig,
                       a + L.kes)))
    return rc;
  launch_block_finish(st, blocks, n, dstatus, a + L.digest, bo.claimed, a + L.kes, dverdict,
                      dbody_hash);
  return launch_check();
}

// The host path over the same batch: the same slicer, the host build of the
// streaming Blake2b and the host Sum6KES, split over the task pool, in chunks
// (no batch-sized arena).  Every span was checked by the caller.
int block_host(const RawCall& c) {
  const size_t C = 1 << 14;
  const size_t cap = std::min(C, c.n);
  const cbor::BlockLayout L = cbor::block_layout(cap);
  std::unique_ptr<uint8_t[]> mem(new (std::nothrow) uint8_t[L.total + 64]);
  if (!mem) return fail(OURO_EDEVICE, "block host path: out of host memory");
  uint8_t* a = cbor::arena_base(mem.get());
  const cbor::Out o = cbor::arena_out(a + L.hdr, cap, nullptr, nullptr);
  const cbor::BlockOut bo = cbor::block_arena_out(a, L);
  uint8_t* kes = a + L.kes;
  uint8_t* bh = a + L.digest;  // 32 B per block here: the computed bbHash
  for (size_t lo = 0; lo < c.n; lo += C) {
    const size_t m = std::min(C, c.n - lo);
    int rc = host_rows(m, 64, [&](size_t r0, size_t r1) {
      for (size_t i = r0; i < r1; i++) {
        const uint8_t st = cbor::block_one(c.raw, c.off[lo + i], c.len[lo + i], c.spkp, o, bo, i);
        c.status[lo + i] = st;
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint8_t ok = 0;
        if (st != OURO_PACK_OK) {
          cbor::block_zero_row(o, bo, i);
        } else {
          uint32_t d[24];
          for (int s = 0; s < 3; s++)
            blake2b256_stream(d + 8 * s, c.raw + bo.seg_off[3 * i + s], bo.seg_len[3 * i + s]);
          blake2b256_96(h, d);
          uint8_t hb[32];
          digest_bytes(hb, h);
          ok = memcmp(hb, bo.claimed + 32 * i, 32) == 0 ? OURO_BLK_BODY_OK : 0;
        }
        digest_bytes(bh + 32 * i, h);
        c.verdict[lo + i] = ok;
      }
    });
    if (rc) return rc;
    if ((rc = ouro_host::kes_batch(m, o.hot_vk, o.kes_t, c.raw, o.body_off, o.body_len, o.kes_sig,
                                   kes)))
      return fail(rc, "block host path failed");
    for (size_t i = 0; i < m; i++) {
      if (c.status[lo + i] != OURO_PACK_OK) c.verdict[lo + i] = 0;
      else if (kes[i]) c.verdict[lo + i] |= OURO_BLK_KES_OK;
    }
    if (c.body_hash) memcpy(c.body_hash + 32 * lo, bh, 32 * m);
  }
  return OURO_OK;
}

}  // namespace ouro_rt

namespace {
// the device / _host pair once: the block kind on the raw-CBOR pipeline, or on
// its host path alone
int block_entry(const uint8_t* raw, size_t raw_bytes, const uint64_t* off, const uint32_t* len,
                size_t n, uint64_t spkp, uint8_t* status, uint8_t* verdict, uint8_t* body_hash,
                bool host) {
  RawCall c = RawCall::of(kRawBlock, raw, raw_bytes, off, len, n, status, verdict);
  c.spkp = spkp;
  c.body_hash = body_hash;
  return host ? raw_verify_host(c) : raw_verify(c);
}
}  // namespace

extern "C" {

// ---- batched Blake2b-256 over arbitrary spans ----
int ouro_blake2b256_batch_host(size_t n, const uint8_t* msg, size_t msg_bytes, const uint64_t* off,
                               const uint32_t* len, uint8_t* out) {
  if (n == 0) return OURO_OK;
  if (int rc = b2b_check(n, msg, msg_bytes, off, len, out)) return rc;
  return b2b_host(n, msg, off, len, out);
}

int ouro_blake2b256_batch(size_t n, const uint8_t* msg, size_t msg_bytes, const uint64_t* off,
                          const uint32_t* len, uint8_t* out) {
  if (n == 0) return OURO_OK;
  if (int rc = b2b_check(n, msg, msg_bytes, off, len, out)) return rc;
  return or_host(b2b_dev(n, msg, off, len, out), [&] { return b2b_host(n, msg, off, len, out); });
}

size_t ouro_blake2b256_work_bytes(size_t n) { return cbor::b2b_work_bytes(n) + 64; }

int ouro_blake2b256_batch_device(void* stream, size_t n, const uint8_t* msg, size_t msg_bytes,
                                 const uint64_t* off, const uint32_t* len, uint8_t* out, void* work,
                                 size_t work_bytes) {
  if (n == 0) return OURO_OK;
  if (!off || !len || !out || !work || (!msg && msg_bytes))
    return fail(OURO_EINVAL, "null argument");
  if (work_bytes < ouro_blake2b256_work_bytes(n)) return fail(OURO_EINVAL, "work area too small");
  if (misaligned(msg, 4)) return fail(OURO_EINVAL, "msg must be 4-byte aligned");
  if (misaligned(out, 16)) return fail(OURO_EINVAL, "out must be 16-byte aligned");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return launch_blake2b(st, n, msg, msg_bytes, off, len, out, cbor::arena_base(work));
}

// ---- whole-block storage integrity ----
size_t ouro_block_pack_bytes(size_t n) { return cbor::block_layout(n).total + 64; }

int ouro_block_integrity_verify_cbor(const uint8_t* raw, size_t raw_bytes, const uint64_t* off,
                                     const uint32_t* len, size_t n, uint64_t slots_per_kes_period,
                                     uint8_t* status, uint8_t* verdict, uint8_t* body_hash) {
  return block_entry(raw, raw_bytes, off, len, n, slots_per_kes_period, status, verdict, body_hash,
                     false);
}

int ouro_block_integrity_verify_cbor_host(const uint8_t* raw, size_t raw_bytes,
                                          const uint64_t* off, const uint32_t* len, size_t n,
                                          uint64_t slots_per_kes_period, uint8_t* status,
                                          uint8_t* verdict, uint8_t* body_hash) {
  return block_entry(raw, raw_bytes, off, len, n, slots_per_kes_period, status, verdict, body_hash,
                     true);
}

int ouro_block_integrity_verify_cbor_device(void* stream, const uint8_t* raw, size_t raw_bytes,
                                            const uint64_t* off, const uint32_t* len, size_t n,
                                            uint64_t slots_per_kes_period, void* arena,
                                            size_t arena_bytes, uint8_t* status, uint8_t* verdict,
                                            uint8_t* body_hash) {
  if (n == 0) return OURO_OK;
  if (!raw || !off || !len || !arena || !status || !verdict)
    return fail(OURO_EINVAL, "null argument");
  if (slots_per_kes_period == 0) return fail(OURO_EINVAL, "zero slots per KES period");
  if (arena_bytes < ouro_block_pack_bytes(n)) return fail(OURO_EINVAL, "arena too small");
  if (misaligned(raw, 4)) return fail(OURO_EINVAL, "raw must be 4-byte aligned");
  if (3 * n > 0xffffffffull) return fail(OURO_EINVAL, "too many blocks in one call");
  hipStream_t st;
  if (int rc = device_entry(stream, &st)) return rc;
  return block_launch(st, raw, raw_bytes, off, len, n, slots_per_kes_period,
                      cbor::arena_base(arena), status, verdict, body_hash);
}

}  // extern "C"
