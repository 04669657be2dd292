#!/usr/bin/env python3
"""Byron transaction witnesses from raw blocks: blocks/s, witness rows/s and
GB/s of the ouro_byron_block_witness_verify_cbor entries (DESIGN.md §1j, §5;
profiles/byron_witnesses/).

Workload: N synthetic regular Byron blocks (default 65,536) in one buffer,
every witness valid, two mixes chosen like tools/byron_blocks.py's:
  light  0 to 10 transactions of about 250 B per block, one or two witnesses
         each (7.5 witness rows per block on average);
  heavy  300 transactions of about 250 B per block, one witness each (300
         witness rows per block).
Witness kinds alternate (VKWitness, RedeemWitness).  The blocks are drawn from a
pool of distinct signed blocks laid out back to back, so the bytes walked and
hashed and the signatures verified are N blocks' worth.

Legs, per mix (each warmed up; every repetition printed):
  device    the device-resident entry with exact capacities: count, scan, emit,
            tx ids, verify (the message built in the lane), tail, finish;
  pageable  the host-buffer entry as one call from pageable memory (upload, the
            same sequence per group, copy back);
  host16    the _host entry on 16 threads (the CPU baseline);
  edbatch   for orientation: ouro_byron_ed25519_verify_batch from pageable
            memory on as many signatures over the same messages, gathered.
Times are host clocks around calls that end synchronised.  Every run's verdicts
are checked (all blocks OURO_BYW_ALL_OK, all signatures valid) before its time
is reported.  One JSON line per measurement on stdout; --summary writes the
medians.

The workloads come from the test suite's builders (tests/byron_witness_cases.py,
with the oracle signing them), reached through sys.path.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def build_mix(mix, n, pool, seed=1):
    """n blocks back to back: dict(buf, raw_bytes, off, len, totals, magic) and
    the rows' keys, signatures and messages for the edbatch leg"""
    import byron_block_cases as C
    import byron_witness_cases as WC
    from ouroboros_network_amd import byron_witness as BW

    rng = np.random.default_rng(seed)
    magic = WC.GOLDEN_MAGIC

    def block(b):
        ntx = 300 if mix == "heavy" else int(rng.integers(0, 11))
        pairs = []
        for t in range(ntx):
            tx = C.sized_array(int(rng.integers(200, 300)), rng)
            c = 1 if mix == "heavy" else 1 + int(rng.integers(0, 2))
            kinds = [WC.VK if (t + q) % 2 == 0 else WC.REDEEM for q in range(c)]
            pairs.append((tx, WC.signed_vector(tx, kinds, magic, first_key=(7 * b + t) % 50)))
        raw = C.make_block(pairs, form=0, indefinite=bool(rng.integers(0, 2)), magic=magic)
        p = BW.parse_byron_witnesses(raw)
        ids = p.tx_ids(raw)
        k = len(p.witnesses)
        msg, mlen = np.zeros((k, 40), np.uint8), np.zeros(k, np.uint32)
        for r, w in enumerate(p.witnesses):
            m = BW.byron_witness_message(magic, w.kind, ids[w.tx])
            msg[r, :len(m)], mlen[r] = np.frombuffer(m, np.uint8), len(m)
        pk = np.frombuffer(b"".join(w.key[:32] for w in p.witnesses), np.uint8).reshape(k, 32)
        sig = np.frombuffer(b"".join(w.sig for w in p.witnesses), np.uint8).reshape(k, 64)
        return raw, len(p.tx_spans), k, pk, sig, msg, mlen

    blocks = [block(b) for b in range(pool)]
    pick = rng.integers(0, pool, size=n)
    ln = np.array([len(blocks[k][0]) for k in pick], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    nbytes = int(ln.sum(dtype=np.uint64))
    # (one copy of the heavy mix's gigabytes: the padding joins with the blocks)
    raw = b"".join([blocks[k][0] for k in pick] + [bytes(-nbytes % 4)])
    totals = [int(sum(blocks[k][q] for k in pick)) for q in (1, 2)]
    cat = lambda q: np.concatenate([blocks[k][q] for k in pick])  # noqa: E731
    return dict(buf=np.frombuffer(raw, np.uint8), raw_bytes=nbytes, off=off, len=ln, totals=totals,
                magic=magic, pk=cat(3), sig=cat(4), msg=cat(5), mlen=cat(6))


def rate(n, rows, nbytes, sec):
    return dict(seconds=round(sec, 6), blocks_per_s=round(n / sec, 1),
                rows_per_s=round(rows / sec, 1), gb_per_s=round(nbytes / sec / 1e9, 3))


def run(args):
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd import byron_witness as BW

    lib = _native.load()
    dev = torch.device("cuda", 0)
    legs = args.legs.split(",")
    summary = {}
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for mix in args.mixes.split(","):
        t0 = time.time()
        w = build_mix(mix, args.n, args.pool_heavy if mix == "heavy" else args.pool)
        n, nbytes, (T, W), magic = args.n, w["raw_bytes"], w["totals"], w["magic"]
        emit(run="workload", mix=mix, n=n, raw_bytes=nbytes, transactions=T, witness_rows=W,
             rows_per_block=round(W / n, 2), build_seconds=round(time.time() - t0, 1))
        triple = (w["buf"][:nbytes], w["off"], w["len"])
        times = {}

        def timed(name, f, reps):
            for _ in range(args.warmup if name != "host16" else 0):
                f()
            times[name] = []
            for rep in range(reps):
                dt = f()
                times[name].append(dt)
                emit(run=name, mix=mix, rep=rep, **rate(n, W, nbytes, dt))

        if "device" in legs:
            up = lambda a, dt: torch.tensor(a.astype(dt), device=dev)  # noqa: E731
            with warnings.catch_warnings():   # (a read-only view, only read from)
                warnings.simplefilter("ignore")
                d_raw = torch.from_numpy(w["buf"]).to(dev)
            d_off, d_len = up(w["off"], np.int64), up(w["len"], np.int32)
            z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
            z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
            o = dict(tx_begin=z(n + 1, torch.int64), wit_begin=z(n + 1, torch.int64),
                     tx_id=z8(max(T, 1), 32), wit_tx=z(max(W, 1), torch.int32),
                     wit_kind=z8(max(W, 1)), wit_ok=z8(max(W, 1)), wit_vk=z8(max(W, 1), 64))
            out = BW.ByronWitnessOutC(T, W, *(o[f].data_ptr() for f in (
                "tx_begin", "wit_begin", "tx_id", "wit_tx", "wit_kind", "wit_ok", "wit_vk")))
            status, verdict, n_bad = z8(n), z8(n), z(n, torch.int32)
            wb = int(lib.ouro_byron_block_witness_work_bytes(n, T, W))
            work = z8(wb)
            emit(run="work_area", mix=mix, bytes=wb)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def device():
                verdict.zero_()
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = lib.ouro_byron_block_witness_verify_cbor_device(
                    st, d_raw.data_ptr(), nbytes, d_off.data_ptr(), d_len.data_ptr(), n, magic,
                    ctypes.byref(out), work.data_ptr(), wb, status.data_ptr(), verdict.data_ptr(),
                    n_bad.data_ptr())
                _native.check(rc, "ouro_byron_block_witness_verify_cbor_device")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                assert bool((verdict == BW.BYW_ALL_OK).all().item())
                assert int(o["wit_begin"][n].item()) == W and bool((o["wit_ok"][:W] == 1).all().item())
                return dt

            timed("device", device, args.reps)
            del d_raw, work, o

        def host_buffer(host):
            def f():
                t = time.perf_counter()
                r = BW.verify_byron_block_witnesses(triple, magic, tx_cap=T, wit_cap=W, host=host)
                dt = time.perf_counter() - t
                assert (r.verdict == BW.BYW_ALL_OK).all() and int(r.wit_begin[-1]) == W
                return dt
            return f

        if "pageable" in legs:
            timed("pageable", host_buffer(False), args.reps)
        if "host16" in legs:
            with _native.knob_env(OURO_HOST_THREADS="16"):
                timed("host16", host_buffer(True), args.host_reps)
        if "edbatch" in legs and W:
            moff = np.arange(W, dtype=np.uint64) * 40
            ok = np.zeros(W, np.uint8)

            def edbatch():
                ok[:] = 0
                t = time.perf_counter()
                rc = lib.ouro_byron_ed25519_verify_batch(W, P(w["pk"]), P(w["sig"]), P(w["msg"]),
                                                         P(moff), P(w["mlen"]), P(ok))
                dt = time.perf_counter() - t
                _native.check(rc, "ouro_byron_ed25519_verify_batch")
                assert (ok == 1).all()
                return dt

            timed("edbatch", edbatch, args.reps)
        summary[mix] = dict(n=n, raw_bytes=nbytes, transactions=T, witness_rows=W,
                            rows_per_block=round(W / n, 2), reps=args.reps)
        for name, v in times.items():
            summary[mix][name] = rate(n, W, nbytes, statistics.median(v))
            summary[mix][name + "_seconds_min_max"] = [round(min(v), 6), round(max(v), 6)]
    if args.summary:
        os.makedirs(os.path.dirname(os.path.abspath(args.summary)), exist_ok=True)
        with open(args.summary, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=64, help="distinct signed blocks, light mix")
    ap.add_argument("--pool-heavy", type=int, default=8, help="distinct signed blocks, heavy mix")
    ap.add_argument("--mixes", default="light,heavy")
    ap.add_argument("--legs", default="device,pageable,host16,edbatch")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--summary", default="", help="write the medians to this JSON file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("byron_witnesses: no GPU (a measurement needs one; no fallback)")
    run(args)


if __name__ == "__main__":
    main()
