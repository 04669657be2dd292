#!/usr/bin/env python3
"""Whole-block storage integrity: blocks/s and GB/s of
ouro_block_integrity_verify_cbor (profiles/block_integrity/).

Workload: N synthetic valid blocks (default 65,536) in one buffer, two
body-size mixes:
  a  uniform, bodies of about 2 KB;
  b  half at most 200 B, a quarter about 4 KB, a quarter about 64 KB.
The blocks are drawn from a pool of distinct signed blocks per size class
(each needs its own Sum6KES signature: the body hash is in the signed header
body) laid out back to back, so the bytes moved and hashed are N blocks' worth.

Runs (each warmed up, then repeated; every repetition is printed):
  device   ouro_block_integrity_verify_cbor_device on device-resident blocks,
           OURO_BLOCK_SORT 1 against 0 alternated within the process;
  onecall  ouro_block_integrity_verify_cbor from pageable host memory, the
           same alternation;
  host     ouro_block_integrity_verify_cbor_host on 16 threads (the CPU baseline);
  integrity  (--mode integrity) ouro_integrity_verify_cbor over raw headers,
           for the parent-against-this-commit comparison: run once per
           library (OURO_VERIFY_LIB), alternated by the caller.
Times are host clocks around calls that end in a device synchronise.  Every
run's verdicts are checked (all blocks valid) before its time is reported.
One JSON line per measurement on stdout.

The workloads come from the test suite's builders (tests/block_cases.py for
blocks, tests/hdr_cases.py for headers, with the oracle signing them), reached
through sys.path: this tool depends on those two test modules.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SPKP = 129600


def emit(**kw):
    print(json.dumps(kw), flush=True)


def build_mix(mix, n, pool, seed=1):
    """(buf, off, len, body bytes) of n valid blocks"""
    import block_cases as BC

    rng = np.random.default_rng(seed)

    def block(body):
        # three segments: bodies ~ 60 %, witnesses ~ 35 %, metadata the rest
        a, b = max(1, body * 6 // 10), max(1, body * 35 // 100)
        c = max(1, body - a - b)
        segs = [BC.segment(x, rng, as_map=False) for x in (a, b, c)]
        return BC.make_block(segs, form=2, tag=2 + int(rng.integers(0, 3)))

    if mix == "a":
        classes = [(1.0, lambda: int(rng.integers(1800, 2300)))]
    else:
        classes = [(0.5, lambda: int(rng.integers(3, 200))),
                   (0.25, lambda: int(rng.integers(3800, 4400))),
                   (0.25, lambda: int(rng.integers(60000, 68000)))]
    pools = [[block(size()) for _ in range(pool)] for _, size in classes]
    pick = rng.choice(len(classes), size=n, p=[w for w, _ in classes])
    raws = [pools[c][int(rng.integers(0, pool))] for c in pick]
    ln = np.array([len(r) for r in raws], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(raws), np.uint8)
    return buf, off, ln


def rate(n, nbytes, sec):
    return dict(seconds=round(sec, 6), blocks_per_s=round(n / sec, 1),
                gb_per_s=round(nbytes / sec / 1e9, 3))


def run_blocks(args):
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd import block as B

    lib = _native.load()
    for mix in args.mixes.split(","):
        t0 = time.time()
        buf, off, ln = build_mix(mix, args.n, args.pool)
        n, nbytes = int(off.size), int(buf.size)
        emit(run="workload", mix=mix, n=n, raw_bytes=nbytes, build_seconds=round(time.time() - t0, 1))
        if "device" in args.runs:
            dev = torch.device("cuda", 0)
            d_raw = torch.tensor(buf, device=dev)
            d_off = torch.tensor(off.astype(np.int64), device=dev)
            d_len = torch.tensor(ln.astype(np.int32), device=dev)
            nb = int(lib.ouro_block_pack_bytes(n))
            arena = torch.zeros(nb, dtype=torch.uint8, device=dev)
            status = torch.zeros(n, dtype=torch.uint8, device=dev)
            verdict = torch.zeros(n, dtype=torch.uint8, device=dev)
            bh = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream()

            def once():
                verdict.zero_()
                torch.cuda.synchronize()
                t = time.perf_counter()
                rc = lib.ouro_block_integrity_verify_cbor_device(
                    ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), nbytes, d_off.data_ptr(),
                    d_len.data_ptr(), n, SPKP, arena.data_ptr(), nb, status.data_ptr(),
                    verdict.data_ptr(), bh.data_ptr())
                _native.check(rc, "ouro_block_integrity_verify_cbor_device")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                assert bool((verdict == 3).all().item()), "a block did not verify"
                return dt

            for sort in (1, 0):
                with _native.knob_env(OURO_BLOCK_SORT=str(sort)):
                    for _ in range(args.warmup):
                        once()
            for rep in range(args.reps):
                for sort in (1, 0):
                    with _native.knob_env(OURO_BLOCK_SORT=str(sort)):
                        emit(run="device", mix=mix, sort=sort, rep=rep, **rate(n, nbytes, once()))
            del d_raw, arena
        if "onecall" in args.runs:
            def call():
                t = time.perf_counter()
                v, s, _ = B.verify_block_integrity_cbor((buf, off, ln), SPKP)
                dt = time.perf_counter() - t
                assert (v == 3).all()
                return dt

            for sort in (1, 0):
                with _native.knob_env(OURO_BLOCK_SORT=str(sort)):
                    for _ in range(max(1, args.warmup - 1)):
                        call()
            for rep in range(args.reps):
                for sort in (1, 0):
                    with _native.knob_env(OURO_BLOCK_SORT=str(sort)):
                        emit(run="onecall", mix=mix, sort=sort, rep=rep, **rate(n, nbytes, call()))
        if "host" in args.runs:
            with _native.knob_env(OURO_HOST_THREADS="16"):
                for rep in range(max(1, args.reps // 2)):
                    t = time.perf_counter()
                    v, s, _ = B.verify_block_integrity_cbor((buf, off, ln), SPKP, host=True)
                    dt = time.perf_counter() - t
                    assert (v == 3).all()
                    emit(run="host16", mix=mix, rep=rep, **rate(n, nbytes, dt))


def run_integrity(args):
    """ouro_integrity_verify_cbor (the existing header entry) on this process's
    library: raw headers from a signed pool, as hdr_cases.seeded_raw builds them"""
    import json as _json

    import torch  # noqa: F401  (its HIP runtime first, as the package does)

    import hdr_cases as HC
    from ouroboros_network_amd import _native
    from ouroboros_network_amd import header as H

    with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
        kats = _json.load(f)
    pool, _ = HC.seeded_raw(kats, None, args.pool, spkp=SPKP)
    rng = np.random.default_rng(2)
    raws = [pool[int(i)] for i in rng.integers(0, len(pool), args.n)]
    trip = H.raw_triplet(raws)
    nbytes = int(trip[0].size)
    for _ in range(args.warmup):
        ok, st = H.verify_integrity_cbor(trip, SPKP)
    assert ok.all()
    for rep in range(args.reps):
        t = time.perf_counter()
        ok, st = H.verify_integrity_cbor(trip, SPKP)
        dt = time.perf_counter() - t
        assert ok.all()
        r = rate(args.n, nbytes, dt)
        emit(run="integrity_cbor", lib=args.label or _native.LIB_PATH, rep=rep, seconds=r["seconds"],
             headers_per_s=r["blocks_per_s"], gb_per_s=r["gb_per_s"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("blocks", "integrity"), default="blocks")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=64, help="distinct signed blocks per size class")
    ap.add_argument("--mixes", default="a,b")
    ap.add_argument("--runs", default="device,onecall,host")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--root", default="", help="integrity mode: the source tree (with its built "
                    "library) to import the package from, e.g. a checkout of the parent commit")
    args = ap.parse_args()
    if args.root:
        root = os.path.abspath(args.root)
        sys.path[:0] = [root, os.path.join(root, "tests")]
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_block_integrity: no GPU (a measurement needs one; no fallback)")
    (run_blocks if args.mode == "blocks" else run_integrity)(args)


if __name__ == "__main__":
    main()
