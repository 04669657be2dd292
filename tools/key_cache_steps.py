#!/usr/bin/env python3
"""What the key directories (csrc/key_cache.h, OURO_KEY_CACHE) cost where they
cannot help, and what they save where they can: bench.py's batch of 1,048,576
headers launched as bench.py's plain run does (device-resident inputs,
ouro_tpraos_verify_batch_device, wall time per launch), in four parts:

  fresh        the first three launches on a stream the library has not seen
               (the first one also allocates the workspaces);
  cold         the knobs reloaded, which empties the directories without
               freeing anything, then three launches: one cold step and two
               warm ones;
  adversarial  --adv-pools pools, then as many other keys, alternately: the two
               sets together exceed the table budget, so every launch empties
               the directory and builds every table again;
  knob         OURO_KEY_CACHE=0 and 1 in this one process, --rounds interleaved
               rounds of --steps launches each (median per round).

Run it once per library (OURO_VERIFY_LIB selects one, as for bench.py); a
library without the directories runs every launch cold, and its "knob" rows
are two equal sides.  Prints one JSON line per part.
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
    ap.add_argument("--adv-pools", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    import bench
    from ouroboros_network_amd import _native

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = args.headers
    lib = _native.load()

    def stats(stream):
        out = (ctypes.c_uint64 * 8)()
        lib.ouro_debug_key_cache(ctypes.c_void_p(stream.cuda_stream), out)
        return list(out)

    def timed(hdr, stream, count):
        ms = []
        for _ in range(count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hdr.launch(stream)
            stream.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms

    t, _ = bench.synth_headers(n, args.pools, dev)
    hdr = bench.DeviceHeaders(t, n, dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        fresh = timed(hdr, stream, 3)
        print(json.dumps({"part": "fresh", "headers": n, "pools": args.pools, "ms": fresh,
                          "key_cache": stats(stream)}), flush=True)
        _native.reload_knobs()
        cold = timed(hdr, stream, 3)
        print(json.dumps({"part": "cold", "headers": n, "pools": args.pools, "ms": cold,
                          "cold_minus_warm_ms": round(cold[0] - min(cold[1:]), 3),
                          "key_cache": stats(stream)}), flush=True)

        for r in range(args.rounds):
            row = {"part": "knob", "round": r + 1, "headers": n, "pools": args.pools}
            for side in ("0", "1"):
                with _native.knob_env(OURO_KEY_CACHE=side):
                    timed(hdr, stream, 2)
                    row["ms_cache_" + side] = float(np.median(timed(hdr, stream, args.steps)))
            print(json.dumps(row), flush=True)

        # two disjoint key sets that do not fit the budget together
        ta, _ = bench.synth_headers(n, args.adv_pools, dev)
        tb = {k: v.clone() for k, v in ta.items()}
        tb["vrf_vk"].view(n, 32)[:, 5] += 1   # other keys (forged: the same work whatever the verdict)
        torch.cuda.synchronize()
        ha, hb = bench.DeviceHeaders(ta, n, dev), bench.DeviceHeaders(tb, n, dev)
        _native.reload_knobs()
        timed(ha, stream, 1)
        timed(hb, stream, 1)
        before = stats(stream)
        ms = []
        for _ in range(args.steps // 2):
            ms += timed(ha, stream, 1) + timed(hb, stream, 1)
        after = stats(stream)
        same = timed(hb, stream, 3)  # the last set again: warm
        print(json.dumps({"part": "adversarial", "headers": n, "pools_each": args.adv_pools,
                          "ms": ms, "median_ms": float(np.median(ms)),
                          "emptied": after[2] - before[2], "launches": len(ms),
                          "warm_same_set_ms": same}), flush=True)


if __name__ == "__main__":
    main()
