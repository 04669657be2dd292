#!/usr/bin/env python3
"""Transaction witnesses from raw blocks: blocks/s and witnesses/s of
ouro_block_witness_verify_cbor_device (profiles/block_witnesses/).

Workload: N synthetic blocks (default 65,536) in one buffer, every witness
valid, two mixes:
  small  1 to 4 transactions per block, bodies of 150 to 400 B, 1 to 3 key
         witnesses each;
  big    half such blocks, a quarter with one body of about 4 KB, a quarter
         with one body of about 64 KB (two witnesses on it) beside two small
         transactions.
The blocks are drawn from a pool of distinct signed blocks per class laid out
back to back, so the bytes walked and hashed are N blocks' worth.

Runs, alternated within one process (each warmed up; every repetition printed):
  witness   the device-resident entry with exact capacities: slice, scan,
            emit, tx ids, Ed25519, finish;
  ed_alone  ouro_ed25519_verify_batch_device on the same witnesses gathered
            beforehand (keys, signatures and tx ids already in rows): what
            `witness` would cost were slicing, scanning and hashing free;
  host16    ouro_block_witness_verify_cbor_host on 16 threads (the CPU baseline).
Times are host clocks around calls that end in a device synchronise.  Every
run's verdicts are checked (all witnesses valid) before its time is reported.
One JSON line per measurement on stdout; --summary writes the medians and the
share of `witness` that `ed_alone` leaves to the new kernels.

The workloads come from the test suite's builders (tests/witness_cases.py,
with the oracle signing them), reached through sys.path.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def build_mix(mix, n, pool, seed=1):
    """n blocks back to back and their witnesses gathered: dict(buf, off, len,
    ntx, nwit, pk, sig, txid, wit_tx)"""
    import witness_cases as WC
    from ouroboros_network_amd import witness as W

    rng = np.random.default_rng(seed)
    key = [0]

    def block(big_body):
        sizes = [int(rng.integers(150, 400)) for _ in range(int(rng.integers(1, 5)))]
        counts = [int(rng.integers(1, 4)) for _ in sizes]
        if big_body:
            sizes, counts = [big_body] + sizes[:2], [2] + counts[:2]
        bodies = [WC.tx_body(s, rng) for s in sizes]
        sets = []
        for b, c in zip(bodies, counts):
            wits = []
            for _ in range(c):
                key[0] += 1
                wits.append(WC.vkey_wit(key[0] % 4096, WC.b2b(b)))
            sets.append(WC.cmap([(WC.uint(0), WC.arr(wits))]))
        raw = WC.make_block(bodies, sets, form=2, tag=2 + int(rng.integers(0, 3)))
        p = W.parse_witnesses(raw)
        ids = p.tx_ids(raw)
        return dict(raw=raw, ntx=len(ids), txid=np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32),
                    pk=np.frombuffer(b"".join(w.vk for w in p.witnesses), np.uint8).reshape(-1, 32),
                    sig=np.frombuffer(b"".join(w.sig for w in p.witnesses), np.uint8).reshape(-1, 64),
                    tx=np.array([w.tx for w in p.witnesses], np.int64))

    if mix == "small":
        classes = [(1.0, lambda: 0)]
    else:
        classes = [(0.5, lambda: 0), (0.25, lambda: int(rng.integers(3800, 4400))),
                   (0.25, lambda: int(rng.integers(60000, 68000)))]
    pools = [[block(size()) for _ in range(pool)] for _, size in classes]
    pick = rng.choice(len(classes), size=n, p=[w for w, _ in classes])
    blocks = [pools[c][int(rng.integers(0, pool))] for c in pick]
    ln = np.array([len(b["raw"]) for b in blocks], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    ntx = np.array([b["ntx"] for b in blocks], np.int64)
    tx_begin = np.concatenate([[0], np.cumsum(ntx)])
    raw = b"".join(b["raw"] for b in blocks)
    return dict(buf=np.frombuffer(raw + bytes(-len(raw) % 4), np.uint8), raw_bytes=len(raw), off=off,
                len=ln, T=int(tx_begin[-1]),
                pk=np.concatenate([b["pk"] for b in blocks]),
                sig=np.concatenate([b["sig"] for b in blocks]),
                txid=np.concatenate([b["txid"] for b in blocks]),
                wit_tx=np.concatenate([b["tx"] + t0 for b, t0 in zip(blocks, tx_begin[:-1])]))


def rate(n, wits, nbytes, sec):
    return dict(seconds=round(sec, 6), blocks_per_s=round(n / sec, 1),
                witnesses_per_s=round(wits / sec, 1), gb_per_s=round(nbytes / sec / 1e9, 3))


def run(args):
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd import witness as W

    lib = _native.load()
    dev = torch.device("cuda", 0)
    summary = {}
    for mix in args.mixes.split(","):
        t0 = time.time()
        w = build_mix(mix, args.n, args.pool)
        n, nbytes, T, Wn = args.n, w["raw_bytes"], w["T"], int(w["pk"].shape[0])
        emit(run="workload", mix=mix, n=n, raw_bytes=nbytes, transactions=T, witnesses=Wn,
             build_seconds=round(time.time() - t0, 1))
        up = lambda a, dt=None: torch.tensor(a if dt is None else a.astype(dt), device=dev)  # noqa: E731
        d_raw, d_off, d_len = up(w["buf"]), up(w["off"], np.int64), up(w["len"], np.int32)
        z8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
        tx_begin = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        wit_begin = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        tx_id, wit_tx = z8(T, 32), torch.zeros(Wn, dtype=torch.int32, device=dev)
        wit_kind, wit_ok, wit_vk = z8(Wn), z8(Wn), z8(Wn, 32)
        status, verdict = z8(n), z8(n)
        n_bad = torch.zeros(n, dtype=torch.int32, device=dev)
        out = W.WitnessOutC(T, Wn, tx_begin.data_ptr(), wit_begin.data_ptr(), tx_id.data_ptr(),
                            wit_tx.data_ptr(), wit_kind.data_ptr(), wit_ok.data_ptr(),
                            wit_vk.data_ptr())
        wb = int(lib.ouro_block_witness_work_bytes(n, T, Wn))
        work = z8(wb)
        # the same witnesses gathered beforehand, for the Ed25519 kernel alone
        g_pk, g_sig, g_msg = up(w["pk"]), up(w["sig"]), up(w["txid"])
        g_off, g_len = up(32 * w["wit_tx"], np.int64), up(np.full(Wn, 32), np.int32)
        g_ver = z8(Wn)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def witness():
            verdict.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = lib.ouro_block_witness_verify_cbor_device(
                st, d_raw.data_ptr(), nbytes, d_off.data_ptr(), d_len.data_ptr(), n,
                ctypes.byref(out), work.data_ptr(), wb, status.data_ptr(), verdict.data_ptr(),
                n_bad.data_ptr())
            _native.check(rc, "ouro_block_witness_verify_cbor_device")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert bool((verdict == 1).all().item()) and int(wit_begin[n].item()) == Wn
            return dt

        def ed_alone():
            g_ver.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = lib.ouro_ed25519_verify_batch_device(
                st, Wn, g_pk.data_ptr(), g_sig.data_ptr(), g_msg.data_ptr(), g_off.data_ptr(),
                g_len.data_ptr(), g_ver.data_ptr())
            _native.check(rc, "ouro_ed25519_verify_batch_device")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert bool((g_ver == 1).all().item())
            return dt

        runs = dict(witness=witness, ed_alone=ed_alone)
        for _ in range(args.warmup):
            for f in runs.values():
                f()
        # the tx ids and rows of the last witness run are the gathered ones
        assert torch.equal(tx_id, g_msg) and torch.equal(wit_vk, g_pk)
        times = {k: [] for k in runs}
        for rep in range(args.reps):
            for name, f in runs.items():
                dt = f()
                times[name].append(dt)
                emit(run=name, mix=mix, rep=rep, **rate(n, Wn, nbytes, dt))
        host = []
        with _native.knob_env(OURO_HOST_THREADS="16"):
            for rep in range(args.host_reps):
                t = time.perf_counter()
                r = W.verify_block_witnesses((w["buf"][:nbytes], w["off"], w["len"]), tx_cap=T,
                                             wit_cap=Wn, host=True)
                dt = time.perf_counter() - t
                assert (r.verdict == 1).all()
                host.append(dt)
                emit(run="host16", mix=mix, rep=rep, **rate(n, Wn, nbytes, dt))
        med = {k: statistics.median(v) for k, v in times.items()}
        summary[mix] = dict(
            n=n, raw_bytes=nbytes, transactions=T, witnesses=Wn, reps=args.reps,
            witness=rate(n, Wn, nbytes, med["witness"]), ed_alone=rate(n, Wn, nbytes, med["ed_alone"]),
            witness_seconds_min_max=[round(min(times["witness"]), 6), round(max(times["witness"]), 6)],
            ed_alone_seconds_min_max=[round(min(times["ed_alone"]), 6),
                                      round(max(times["ed_alone"]), 6)],
            new_kernels_share=round(1 - med["ed_alone"] / med["witness"], 4),
            host16=rate(n, Wn, nbytes, statistics.median(host)) if host else None)
        del d_raw, work
    if args.summary:
        os.makedirs(os.path.dirname(os.path.abspath(args.summary)), exist_ok=True)
        with open(args.summary, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=64, help="distinct signed blocks per class")
    ap.add_argument("--mixes", default="small,big")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--summary", default="", help="write the medians to this JSON file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_block_witnesses: no GPU (a measurement needs one; no fallback)")
    run(args)


if __name__ == "__main__":
    main()
