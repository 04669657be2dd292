#!/usr/bin/env python3
"""Byron whole-block integrity from raw blocks: blocks/s and GB/s of the
ouro_byron_block_integrity_verify_cbor entries (DESIGN.md §1i, §5;
profiles/byron_block_integrity/).

Workload: N synthetic regular Byron blocks (default 65,536) in one buffer,
every block valid, two mixes:
  light  0 to 10 transactions of about 250 B per block;
  heavy  300 transactions of about 250 B per block.
Every transaction carries the golden block's witness vector (140 B).  The
blocks are drawn from a pool of distinct signed blocks laid out back to back,
so the bytes walked and hashed are N blocks' worth.

Legs, per mix (each warmed up; every repetition printed):
  device    the device-resident entry with exact capacities: count, scan, emit,
            leaf hashes, Merkle roots, plain hashes, ByronDSIGN, finish;
  pageable  the host-buffer entry from pageable memory (upload, the same
            sequence per group, copy back);
  host16    the _host entry on 16 threads (the CPU baseline).
Times are host clocks around calls that end synchronised.  Every run's verdicts
are checked (all blocks OURO_BYB_ALL_OK) before its time is reported.  One JSON
line per measurement on stdout; --summary writes the medians.

The workloads come from the test suite's builders (tests/byron_block_cases.py,
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
    """n blocks back to back: dict(buf, raw_bytes, off, len, totals, magic)"""
    import byron_block_cases as C
    from ouroboros_network_amd import byron_block as BB

    rng = np.random.default_rng(seed)
    wit = C.parts()["wit"]
    magic = C.parts()["magic_value"]

    def block():
        ntx = 300 if mix == "heavy" else int(rng.integers(0, 11))
        pairs = [(C.sized_array(int(rng.integers(200, 300)), rng), wit) for _ in range(ntx)]
        raw = C.make_block(pairs, form=0, indefinite=bool(rng.integers(0, 2)))
        return raw, BB.byron_block_counts(raw, magic)

    blocks = [block() for _ in range(pool)]
    pick = rng.integers(0, pool, size=n)
    ln = np.array([len(blocks[k][0]) for k in pick], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    nbytes = int(ln.sum(dtype=np.uint64))
    # (one copy of the heavy mix's gigabytes: the padding joins with the blocks)
    raw = b"".join([blocks[k][0] for k in pick] + [bytes(-nbytes % 4)])
    totals = [int(sum(blocks[k][1][q] for k in pick)) for q in (1, 2, 3)]
    return dict(buf=np.frombuffer(raw, np.uint8), raw_bytes=nbytes, off=off, len=ln, totals=totals,
                magic=magic)


def rate(n, txs, nbytes, sec):
    return dict(seconds=round(sec, 6), blocks_per_s=round(n / sec, 1),
                txs_per_s=round(txs / sec, 1), gb_per_s=round(nbytes / sec / 1e9, 3))


def run(args):
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd import byron_block as BB

    lib = _native.load()
    dev = torch.device("cuda", 0)
    legs = args.legs.split(",")
    summary = {}
    for mix in args.mixes.split(","):
        t0 = time.time()
        w = build_mix(mix, args.n, args.pool_heavy if mix == "heavy" else args.pool)
        n, nbytes, (T, G, M), magic = args.n, w["raw_bytes"], w["totals"], w["magic"]
        emit(run="workload", mix=mix, n=n, raw_bytes=nbytes, transactions=T, gather_bytes=G,
             msg_bytes=M, build_seconds=round(time.time() - t0, 1))
        triple = (w["buf"][:nbytes], w["off"], w["len"])
        times = {}

        def timed(name, f, reps):
            for _ in range(args.warmup if name != "host16" else 0):
                f()
            times[name] = []
            for rep in range(reps):
                dt = f()
                times[name].append(dt)
                emit(run=name, mix=mix, rep=rep, **rate(n, T, nbytes, dt))

        if "device" in legs:
            up = lambda a, dt: torch.tensor(a.astype(dt), device=dev)  # noqa: E731
            with warnings.catch_warnings():   # (a read-only view, only read from)
                warnings.simplefilter("ignore")
                d_raw = torch.from_numpy(w["buf"]).to(dev)
            d_off, d_len = up(w["off"], np.int64), up(w["len"], np.int32)
            z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
            status, verdict, root = z8(n), z8(n), z8(n, 32)
            wb = int(lib.ouro_byron_block_work_bytes(n, T, G, M))
            work = z8(wb)
            emit(run="work_area", mix=mix, bytes=wb)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def device():
                verdict.zero_()
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = lib.ouro_byron_block_integrity_verify_cbor_device(
                    st, d_raw.data_ptr(), nbytes, d_off.data_ptr(), d_len.data_ptr(), n, magic, T,
                    G, M, work.data_ptr(), wb, status.data_ptr(), verdict.data_ptr(),
                    root.data_ptr())
                _native.check(rc, "ouro_byron_block_integrity_verify_cbor_device")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                assert bool((verdict == BB.BYB_ALL_OK).all().item())
                return dt

            timed("device", device, args.reps)
            del d_raw, work

        def host_buffer(host):
            def f():
                t = time.perf_counter()
                v, _, _ = BB.verify_byron_block_integrity(triple, magic, host=host)
                dt = time.perf_counter() - t
                assert (v == BB.BYB_ALL_OK).all()
                return dt
            return f

        if "pageable" in legs:
            timed("pageable", host_buffer(False), args.reps)
        if "host16" in legs:
            with _native.knob_env(OURO_HOST_THREADS="16"):
                timed("host16", host_buffer(True), args.host_reps)
        summary[mix] = dict(n=n, raw_bytes=nbytes, transactions=T, gather_bytes=G, msg_bytes=M,
                            reps=args.reps)
        for name, v in times.items():
            summary[mix][name] = rate(n, T, nbytes, statistics.median(v))
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
    ap.add_argument("--legs", default="device,pageable,host16")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--summary", default="", help="write the medians to this JSON file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("byron_blocks: no GPU (a measurement needs one; no fallback)")
    run(args)


if __name__ == "__main__":
    main()
