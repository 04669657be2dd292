"""A stored chain replayed through the combined raw entry on one GPU
(ouro_chain_verify_cbor) against the single-era, single-nonce entries it
replaces, over synthetic node-configuration raw headers in pageable host
memory (bench.synth_raw_node_headers, one segment per epoch nonce,
concatenated).  Prints one JSON object per leg; the two sides of a leg are
alternated on the same buffer in the same process.
    python tools/chain_replay.py [n] [reps] [legs]
legs (comma separated, default all):
  pure    n TPraos headers of one epoch, a one-entry schedule: the combined
          entry against ouro_tpraos_verify_cbor
  epochs  n headers over 8 epochs in one call under a 512-entry schedule,
          against the same headers as 8 single-nonce calls
  eras    n/2 Byron + n/2 TPraos headers in one call, against
          ouro_byron_verify_cbor + ouro_tpraos_verify_cbor back to back"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPKP = 129600
EPOCHS = 8       # the synthetic slots are t * SPKP + i % 1000 with t = i % 64:
PERIODS = 64     # epoch e = the KES periods [8 e, 8 e + 8)
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def nonce_of(e):
    return bytes((101 + 7 * e + k) & 0xFF for k in range(32))


def segment(n, e, dev, whole=False):
    """n synthetic headers proved under epoch e's nonce, and of those (unless
    `whole`) the ones whose slots lie in epoch e: (uint8 array of whole
    headers, header length)"""
    import torch

    import bench
    raw, rl = bench.synth_raw_node_headers(n, 1024, dev, nonce_of(e), SPKP)
    if not whole:
        t = torch.arange(n, device=dev) % PERIODS
        keep = (t // (PERIODS // EPOCHS)) == e
        raw = raw.view(n, rl)[keep].reshape(-1)
    buf = raw.cpu().numpy()
    del raw
    torch.cuda.empty_cache()
    return buf, rl


class Stream:
    def __init__(self, buf, off, ln):
        self.buf, self.off, self.ln, self.n = buf, off, ln, int(off.size)
        n = self.n
        self.proto = np.zeros(n, np.uint8)
        self.st = np.zeros(n, np.uint8)
        self.v = np.zeros(n, np.uint8)
        self.be = np.zeros((n, 64), np.uint8)
        self.bl = np.zeros((n, 64), np.uint8)

    @classmethod
    def fixed(cls, buf, rl):
        n = buf.size // rl
        return cls(buf, np.arange(n, dtype=np.uint64) * rl, np.full(n, rl, np.uint32))

    def rows(self, lo, hi):
        return Stream(self.buf, self.off[lo:hi].copy(), self.ln[lo:hi].copy())


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(a, b, reps):
    """a and b alternated reps times after one untimed call of each"""
    a(), b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a))
        tb.append(timed(b))
    return ta, tb


def report(leg, n, combined, split, **kw):
    r = lambda x: [round(t, 2) for t in x]  # noqa: E731
    print(json.dumps({"leg": leg, "n": n, "combined_ms": r(combined), "split_ms": r(split),
                      "combined_median": round(statistics.median(combined), 2),
                      "split_median": round(statistics.median(split), 2),
                      "split_spread": round(max(split) - min(split), 2), **kw}), flush=True)


def main():
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd.tpraos import EpochNonces

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    legs = (sys.argv[3] if len(sys.argv) > 3 else "pure,epochs,eras").split(",")
    dev = torch.device("cuda", 0)
    lib = _native.load()
    lib.ouro_bind_thread_to_device(0)

    def chain(s, epochs):
        e = None if epochs is None else ctypes.byref(epochs.c_struct())
        rc = lib.ouro_chain_verify_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, -1, e,
                                        None, None, P(s.proto), P(s.st), P(s.v), P(s.be), P(s.bl),
                                        None)
        assert rc == 0, lib.ouro_last_error()

    def tpraos(s, eta0):
        e0 = np.frombuffer(eta0, np.uint8)
        rc = lib.ouro_tpraos_verify_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, P(e0),
                                         None, None, P(s.st), P(s.v), P(s.be), P(s.bl), None)
        assert rc == 0, lib.ouro_last_error()

    def byron(s):
        rc = lib.ouro_byron_verify_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, -1, P(s.st),
                                        P(s.v))
        assert rc == 0, lib.ouro_last_error()

    if "pure" in legs:
        s = Stream.fixed(*segment(n, 0, dev, whole=True))
        one = EpochNonces(first_slot=[0], nonce=[nonce_of(0)])
        tc, ts = alternate(lambda: chain(s, one), lambda: tpraos(s, nonce_of(0)), reps)
        chain(s, one)
        ok = bool((s.proto == 1).all() and (s.st == 0).all() and ((s.v & 0x3F) == 0x3F).all())
        report("pure", s.n, tc, ts, all_valid=ok)
        del s

    if "epochs" in legs:
        parts = [segment(n, e, dev) for e in range(EPOCHS)]
        rl = parts[0][1]
        s = Stream.fixed(np.concatenate([p[0] for p in parts]), rl)
        cuts = np.cumsum([0] + [p[0].size // rl for p in parts])
        del parts
        # 512 entries: every epoch's slots cut into 64 runs that carry its nonce
        k = 512
        per = PERIODS * SPKP // k
        sched = EpochNonces(first_slot=np.arange(k, dtype=np.uint64) * per,
                            nonce=[nonce_of(j // (k // EPOCHS)) for j in range(k)])
        segs = [s.rows(int(cuts[e]), int(cuts[e + 1])) for e in range(EPOCHS)]

        def split():
            for e, g in enumerate(segs):
                tpraos(g, nonce_of(e))

        tc, ts = alternate(lambda: chain(s, sched), split, reps)
        split()
        ok_split = all(bool(((g.v & 0x3F) == 0x3F).all()) for g in segs)
        chain(s, sched)
        ok = bool((s.st == 0).all() and ((s.v & 0x3F) == 0x3F).all())
        report("epochs", s.n, tc, ts, epochs=EPOCHS, schedule=k, all_valid=ok and ok_split)
        del s, segs

    if "eras" in legs:
        with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
            wires = [bytes.fromhex(w["raw"]) for w in json.load(f)["byron_wire"]]
        half = n // 2
        braw = [wires[i % len(wires)] for i in range(half)]
        bln = np.array([len(r) for r in braw], np.uint32)
        bbuf = np.frombuffer(b"".join(braw), np.uint8)
        tbuf, rl = segment(half, 0, dev, whole=True)
        ln = np.concatenate([bln, np.full(half, rl, np.uint32)])
        off = np.zeros(ln.size, np.uint64)
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        s = Stream(np.concatenate([bbuf, tbuf]), off, ln)
        sb, st_ = s.rows(0, half), s.rows(half, 2 * half)
        one = EpochNonces(first_slot=[0], nonce=[nonce_of(0)])

        def split():
            byron(sb)
            tpraos(st_, nonce_of(0))

        tc, ts = alternate(lambda: chain(s, one), split, reps)
        chain(s, one)
        ok = bool((s.proto[:half] == 0).all() and (s.proto[half:] == 1).all() and
                  (s.v[:half] == 1).all() and ((s.v[half:] & 0x3F) == 0x3F).all())
        report("eras", s.n, tc, ts, byron=half, tpraos=half, all_valid=ok)


if __name__ == "__main__":
    main()
