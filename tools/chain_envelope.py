"""What the header envelope costs on one GPU (ouro_chain_validate_cbor,
ouro_chain_envelope_cbor_device), over synthetic node-configuration raw
headers in pageable host memory as tools/chain_replay.py builds them.  The two
sides of a leg are alternated on the same buffer in the same process; one JSON
object per leg.
    python tools/chain_envelope.py [n] [reps] [legs] [parent library]
legs (comma separated, default all):
  existing  ouro_chain_verify_cbor on n TPraos headers: this library against the
            parent commit's (the path given as the fourth argument; skipped
            without it) -- existing callers lose nothing
  tpraos    ouro_chain_validate_cbor against ouro_chain_verify_cbor, n TPraos
  byron     the same on n Byron headers
  eras      the same on n/2 Byron + n/2 TPraos headers
  device    ouro_chain_envelope_cbor_device alone on n TPraos headers resident
            on the device: headers/s and GB/s of raw header bytes; beside it
            ouro_blake2b256_batch_device (k_blake2b256 behind its length sort)
            over exactly the spans the header hashes cover
  device_byron  the same on n Byron headers"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import chain_replay as CR  # noqa: E402

P = CR.P
SPKP = CR.SPKP


def report(leg, n, new, old, **kw):
    r = lambda x: [round(t, 2) for t in x]  # noqa: E731
    print(json.dumps({"leg": leg, "n": n, "new_ms": r(new), "old_ms": r(old),
                      "new_median": round(statistics.median(new), 2),
                      "old_median": round(statistics.median(old), 2),
                      "old_spread": round(max(old) - min(old), 2),
                      "delta_pct": round(100 * (statistics.median(new) / statistics.median(old)
                                                - 1), 2), **kw}), flush=True)


def main():
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd.tpraos import EpochNonces

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    legs = (sys.argv[3] if len(sys.argv) > 3 else
            "existing,tpraos,byron,eras,device,device_byron").split(",")
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    dev = torch.device("cuda", 0)
    lib = _native.load()
    lib.ouro_bind_thread_to_device(0)
    one = EpochNonces(first_slot=[0], nonce=[CR.nonce_of(0)])
    cfg = _native.EnvelopeCfg(byron_epoch_slots=21600)

    def verify(s, which=lib):
        rc = which.ouro_chain_verify_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, -1,
                                          ctypes.byref(one.c_struct()), None, None, P(s.proto),
                                          P(s.st), P(s.v), P(s.be), P(s.bl), None)
        assert rc == 0, which.ouro_last_error()

    def validate(s):
        rc = lib.ouro_chain_validate_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, -1,
                                          ctypes.byref(one.c_struct()), None, None,
                                          ctypes.byref(cfg), None, P(s.proto), P(s.st), P(s.v),
                                          P(s.be), P(s.bl), None, P(s.hh), P(s.env), None)
        assert rc == 0, lib.ouro_last_error()

    def stream(buf, off, ln):
        s = CR.Stream(buf, off, ln)
        s.hh = np.zeros((s.n, 32), np.uint8)
        s.env = np.zeros(s.n, np.uint8)
        return s

    def fixed(buf, rl):
        k = buf.size // rl
        return stream(buf, np.arange(k, dtype=np.uint64) * rl, np.full(k, rl, np.uint32))

    def byron_part(k):
        with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
            wires = [bytes.fromhex(w["raw"]) for w in json.load(f)["byron_wire"]]
        braw = [wires[i % len(wires)] for i in range(k)]
        return np.frombuffer(b"".join(braw), np.uint8), np.array([len(r) for r in braw], np.uint32)

    def offsets(ln):
        off = np.zeros(ln.size, np.uint64)
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        return off

    tbuf = rl = None
    if any(x in legs for x in ("existing", "tpraos", "device")):
        tbuf, rl = CR.segment(n, 0, dev, whole=True)

    if "existing" in legs and parent:
        old = ctypes.CDLL(parent)
        for name in ("ouro_chain_verify_cbor", "ouro_last_error"):
            res, args = _native.SIGNATURES[name]
            getattr(old, name).restype, getattr(old, name).argtypes = res, args
        s = fixed(tbuf, rl)
        tn, to = CR.alternate(lambda: verify(s), lambda: verify(s, old), reps)
        report("existing", s.n, tn, to, what="ouro_chain_verify_cbor: this library / the parent's")

    def ab(leg, s, **kw):
        tn, to = CR.alternate(lambda: validate(s), lambda: verify(s), reps)
        validate(s)
        hashed = int(s.hh.any(axis=1).sum())
        report(leg, s.n, tn, to, what="ouro_chain_validate_cbor / ouro_chain_verify_cbor",
               hashed=hashed, raw_bytes=int(s.buf.size), **kw)

    if "tpraos" in legs:
        ab("tpraos", fixed(tbuf, rl))
    if "byron" in legs:
        bbuf, bln = byron_part(n)
        ab("byron", stream(bbuf, offsets(bln), bln))
    if "eras" in legs:
        half = n // 2
        bbuf, bln = byron_part(half)
        hbuf, hrl = (tbuf[:half * rl], rl) if tbuf is not None else CR.segment(half, 0, dev, True)
        ln = np.concatenate([bln, np.full(half, hrl, np.uint32)])
        ab("eras", stream(np.concatenate([bbuf, hbuf]), offsets(ln), ln), byron=half, tpraos=half)

    def hashed_span(raw):
        """(offset, length) inside a wire header of the bytes its hash covers"""
        from ouroboros_network_amd import envelope as E
        from ouroboros_network_amd import header as H
        item = E._byron_item(raw)[1] if H.era_class(raw) == H.PROTO_PBFT else None
        if item is None:
            i = 0
            mt, _, j = H._head(raw, 0)
            if mt == 4:
                i = H.skip(raw, j)
            _, _, j = H._head(raw, i)
            _, ln_, k_ = H._head(raw, j)
            return k_, ln_
        return raw.index(item), len(item)

    def device_leg(name, buf, off, ln, hoff, hlen):
        """the device form alone, and k_blake2b256 (ouro_blake2b256_batch_device)
        over exactly the spans the header hashes cover, both timed with stream
        events around the launches"""
        k = int(off.size)
        pad = (-buf.size) % 4
        d_raw = torch.tensor(np.concatenate([buf, np.zeros(pad, np.uint8)]), device=dev)
        d_off = torch.tensor(off.astype(np.int64), device=dev)
        d_len = torch.tensor(ln.astype(np.int32), device=dev)
        d_hoff = torch.tensor(hoff.astype(np.int64), device=dev)
        d_hlen = torch.tensor(hlen.astype(np.int32), device=dev)
        wb = lib.ouro_chain_envelope_work_bytes(k)
        work = torch.zeros(wb, dtype=torch.uint8, device=dev)
        bwb = lib.ouro_blake2b256_work_bytes(k)
        bwork = torch.zeros(bwb, dtype=torch.uint8, device=dev)
        st = torch.zeros(k, dtype=torch.uint8, device=dev)
        hh = torch.zeros((k, 32), dtype=torch.uint8, device=dev)
        hh2 = torch.zeros((k, 32), dtype=torch.uint8, device=dev)
        bits = torch.zeros(k, dtype=torch.uint8, device=dev)
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def envelope():
            rc = lib.ouro_chain_envelope_cbor_device(
                sp, d_raw.data_ptr(), buf.size, d_off.data_ptr(), d_len.data_ptr(), k,
                ctypes.byref(cfg), None, work.data_ptr(), wb, st.data_ptr(), hh.data_ptr(),
                bits.data_ptr(), None)
            assert rc == 0, lib.ouro_last_error()

        def blake():
            rc = lib.ouro_blake2b256_batch_device(sp, k, d_raw.data_ptr(), buf.size,
                                                  d_hoff.data_ptr(), d_hlen.data_ptr(),
                                                  hh2.data_ptr(), bwork.data_ptr(), bwb)
            assert rc == 0, lib.ouro_last_error()

        def events(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            return ms

        me, mb = events(envelope), events(blake)
        med, medb = statistics.median(me), statistics.median(mb)
        hbytes = int(hlen.astype(np.int64).sum())
        print(json.dumps({
            "leg": name, "n": k, "envelope_ms": [round(x, 3) for x in me],
            "envelope_median_ms": round(med, 3), "headers_per_s": round(k / med * 1e3),
            "raw_gb_per_s": round(buf.size / med / 1e6, 2),
            "blake2b_ms": [round(x, 3) for x in mb], "blake2b_median_ms": round(medb, 3),
            "blake2b_hashes_per_s": round(k / medb * 1e3),
            "blake2b_gb_per_s": round(hbytes / medb / 1e6, 2), "hashed_bytes": hbytes,
            "sliced": int(((st == 0) | (st == 6)).sum().item()),
            # a TPraos hash has no prefix: there the two digests are the same bytes
            "same_digests": bool((hh == hh2).all().item())}), flush=True)

    if "device" in legs:
        k = tbuf.size // rl
        o0, l0 = hashed_span(bytes(tbuf[:rl]))
        off = np.arange(k, dtype=np.uint64) * rl
        device_leg("device", tbuf, off, np.full(k, rl, np.uint32), off + np.uint64(o0),
                   np.full(k, l0, np.uint32))
    if "device_byron" in legs:
        bbuf, bln = byron_part(n)
        boff = offsets(bln)
        with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
            wires = [bytes.fromhex(w["raw"]) for w in json.load(f)["byron_wire"]]
        sp_ = [hashed_span(w) for w in wires]
        ho = np.array([sp_[i % len(wires)][0] for i in range(n)], np.uint64)
        hl = np.array([sp_[i % len(wires)][1] for i in range(n)], np.uint32)
        device_leg("device_byron", bbuf, boff, bln, boff + ho, hl)


if __name__ == "__main__":
    main()
