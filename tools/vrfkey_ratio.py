#!/usr/bin/env python3
"""Where the per-key VRF tables (OURO_VRFKEY_SHARE) stop paying: bench.py's
batch of 1,048,576 headers at several pool counts, launched and timed as
bench.py's plain run does (device-resident inputs,
ouro_tpraos_verify_batch_device on the current stream, wall time over --steps
launches).  A pool count of 0 stands for "every key distinct": the 1,024-pool
batch with the row index added into the first four bytes of every vrf_vk, so
every header carries its own -- forged -- key (verdict 3 everywhere; the
kernels do the same work whatever the verdict).

Run it once per library (OURO_VERIFY_LIB selects one, as for bench.py): the
parent's and the product, alternated by the caller.  --tab-mb sets
OURO_VRFKEY_TAB_MB for the run, so that pool counts above the default
budget's 5,900 keys still build tables and the crossover in headers per key
(csrc/vrfkey_ws.h OURO_VRFKEY_MIN_PER_KEY, compiled in) shows.  Prints one
JSON line per pool count.
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
    ap.add_argument("--pools", default="1024,4096,32768,0",
                    help="comma-separated pool counts; 0 = every vrf_vk distinct")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tab-mb", type=int, default=None)
    args = ap.parse_args()
    if args.tab_mb is not None:
        os.environ["OURO_VRFKEY_TAB_MB"] = str(args.tab_mb)

    import torch

    import bench
    from ouroboros_network_amd import _native

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = args.headers
    lib = _native.load()
    for pools in (int(p) for p in args.pools.split(",")):
        t, _ = bench.synth_headers(n, pools or 1024, dev)
        if not pools:
            idx = torch.arange(n, dtype=torch.int64, device=dev)
            vk = t["vrf_vk"].view(n, 32)
            for k in range(4):
                vk[:, k] += ((idx >> (8 * k)) & 0xFF).to(torch.uint8)
        hdr = bench.DeviceHeaders(t, n, dev)
        stream = torch.cuda.current_stream()
        for _ in range(args.warmup):
            hdr.launch(stream)
        torch.cuda.synchronize()
        shared = ctypes.c_int(0)
        keys = int(lib.ouro_debug_last_vrfkey_groups(ctypes.c_void_p(stream.cuda_stream),
                                                     ctypes.byref(shared)))
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            hdr.launch(stream)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        v = hdr.verdict.cpu().numpy()
        print(json.dumps({
            "tool": "vrfkey_ratio", "lib": os.environ.get("OURO_VERIFY_LIB", "product"),
            "headers": n, "pools": pools or n, "distinct_keys": not pools,
            "tab_mb": args.tab_mb, "keys_found": keys, "shared": bool(shared.value),
            "headers_per_key": n / (pools or n), "steps": args.steps,
            "ms_per_step_median": float(np.median(ms)), "ms_per_step_min": float(min(ms)),
            "ms_per_step_max": float(max(ms)),
            "verdict_counts": {str(k): int(c) for k, c in zip(*np.unique(v, return_counts=True))},
        }), flush=True)
        del hdr, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
