#!/usr/bin/env python3
"""The cost of the shared OCERT checks where there is nothing to share:
bench.py's batch (1,048,576 headers, 1,024 pools) with every ocert_sigma row
made distinct (the row index added into its first four bytes), launched and
timed as bench.py's plain run does (device-resident inputs,
ouro_tpraos_verify_batch_device on the current stream, wall time over --steps
launches).  Every header then carries its own -- forged -- certificate: the
group pass finds n records, above kOcertShareMax(n), and the header kernel
runs the OCERT core inline (verdict 14 everywhere).

Run it once per library (OURO_VERIFY_LIB selects one, as for bench.py): the
parent's, the product, and a -DOURO_OCERT_BYPASS=0 build that shares whatever
the count.  --pools-distinct 0 times the untouched batch instead.  Prints one
JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headers", type=int, default=1 << 20)
    ap.add_argument("--pools", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pools-distinct", type=int, default=1,
                    help="1: every sigma row distinct (default); 0: the batch as synthesised")
    args = ap.parse_args()

    import torch

    import bench
    from ouroboros_network_amd import _native

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = args.headers
    t, _ = bench.synth_headers(n, args.pools, dev)
    if args.pools_distinct:
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        sig = t["ocert_sigma"].view(n, 64)
        for k in range(4):
            sig[:, k] += ((idx >> (8 * k)) & 0xFF).to(torch.uint8)
    hdr = bench.DeviceHeaders(t, n, dev)
    stream = torch.cuda.current_stream()
    for _ in range(args.warmup):
        hdr.launch(stream)
    torch.cuda.synchronize()
    lib = _native.load()
    groups = None
    if hasattr(lib, "ouro_debug_last_ocert_groups"):
        groups = int(lib.ouro_debug_last_ocert_groups(ctypes.c_void_p(stream.cuda_stream)))
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        hdr.launch(stream)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    v = hdr.verdict.cpu().numpy()
    print(json.dumps({
        "tool": "ocert_distinct", "lib": os.environ.get("OURO_VERIFY_LIB", "product"),
        "headers": n, "pools": args.pools, "distinct_sigma": bool(args.pools_distinct),
        "groups": groups, "steps": args.steps,
        "ms_per_step_median": float(np.median(ms)), "ms_per_step_min": float(min(ms)),
        "ms_per_step_max": float(max(ms)),
        "verdict_counts": {str(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))},
    }))


if __name__ == "__main__":
    main()
