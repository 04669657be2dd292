#!/usr/bin/env python3
"""What the Byron ledger-view checks cost on one GPU: k_pbft_checks and
k_byron_key_hash alone (the device-pointer entries on rows resident on the
device, timed with stream events), the host-buffer entry, and the host's
window fold, over n seeded regular rows of 7 delegates under mainnet's window
(2,160 signers, threshold 475).  One JSON object per leg.
    python tools/pbft_checks.py [n] [reps]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ouroboros_network_amd import _native  # noqa: E402
from ouroboros_network_amd import pbft as P  # noqa: E402


def report(leg, n, ms, **kw):
    med = statistics.median(ms)
    print(json.dumps({"leg": leg, "n": n, "ms": [round(t, 3) for t in ms], "median_ms": round(med, 3),
                      "ns_per_row": round(1e6 * med / n, 2), **kw}), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    import torch

    torch.cuda.init()
    lib = _native.load()
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 256, (7, 64), dtype=np.uint8)
    ids = P.byron_key_hash(keys, host=True)
    v = P.PBftViews([(0, [(ids[i].tobytes(), bytes([i + 1]) * 28) for i in range(7)])], 2160, 475)
    vk = np.ascontiguousarray(keys[np.arange(n) % 7])
    slot = np.arange(n, dtype=np.uint64) * 20
    status = np.zeros(n, np.uint8)
    dev = torch.device("cuda", 0)
    d_vk, d_slot = torch.tensor(vk, device=dev), torch.tensor(slot.view(np.int64), device=dev)
    d_status = torch.tensor(status, device=dev)
    bits = torch.zeros(n, dtype=torch.uint8, device=dev)
    rows = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
    cv, h = v.c_struct(), ctypes.c_void_p()
    _native.check(lib.ouro_pbft_views_upload(ctypes.byref(cv), ctypes.byref(h)), "upload")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ms = []
        for r in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms.append(a.elapsed_time(b))
        return ms

    report("k_pbft_checks", n, timed(lambda: _native.check(lib.ouro_pbft_ledger_checks_device(
        st, n, d_vk.data_ptr(), d_slot.data_ptr(), d_status.data_ptr(), h, bits.data_ptr(),
        rows.data_ptr()), "device")))
    report("k_byron_key_hash", n, timed(lambda: _native.check(lib.ouro_byron_key_hash_batch_device(
        st, n, d_vk.data_ptr(), out.data_ptr()), "device")))
    assert int((bits == 1).sum()) == n
    lib.ouro_pbft_views_free(h)

    def wall(fn):
        ms = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            fn()
            if r >= 1:
                ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    report("ouro_pbft_ledger_checks (host buffers, no fold)", n,
           wall(lambda: P.pbft_checks(vk, slot, status, v)))
    nb, nr, _ = P.pbft_checks(vk, slot, status, v)
    res = {}

    def fold():
        res["out"] = P.pbft_window_fold(nb, nr, slot, v, P.PBftState())

    report("ouro_pbft_window_fold (host)", n, wall(fold))
    assert int((res["out"][0] == P.PBFT_ALL_OK).sum()) == n
    report("ouro_pbft_ledger_checks_host (no fold)", n,
           wall(lambda: P.pbft_checks(vk, slot, status, v, host=True)))


if __name__ == "__main__":
    main()
