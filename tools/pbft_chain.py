#!/usr/bin/env python3
"""What the Byron ledger-view checks cost inside the raw-CBOR pipeline, on one
GPU: ouro_chain_validate_ledger_pbft_cbor of this library against
ouro_chain_validate_cbor of the parent commit's (the path given as the third
argument; this library's own entry without it) on the same n raw Byron headers
in pageable host memory, the two alternated in one process.  The headers are
the 768 signed headers of tests/pbft_cases.chain3 repeated (valid signatures,
three delegates, an EBB every 256), under mainnet's window (2,160, threshold
475).  One JSON object.
    python tools/pbft_chain.py [n] [reps] [parent library]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pbft_cases as PC  # noqa: E402
from ouroboros_network_amd import _native  # noqa: E402
from ouroboros_network_amd import header as H  # noqa: E402
from ouroboros_network_amd import pbft as P  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    import torch

    torch.cuda.init()
    lib = _native.load()
    old = lib
    if len(sys.argv) > 3:
        old = ctypes.CDLL(os.path.abspath(sys.argv[3]))
        f = old.ouro_chain_validate_cbor
        f.restype, f.argtypes = _native.SIGNATURES["ouro_chain_validate_cbor"]
    base = list(PC.chain3())
    raws = (base * (n // len(base) + 1))[:n]
    buf, off, ln = H.raw_triplet(raws)
    lv, g, spkp = PC.trivial_ledger()
    pv = PC.chain_views(2160, 475)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    u8 = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    proto, status, verdict, be, bl, hh, env = u8(n), u8(n), u8(n), u8(n, 64), u8(n, 64), u8(n, 32), u8(n)
    ledger, rows = u8(n), np.zeros(n, np.uint32)
    pb, prow, cnt = u8(n), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    c_cfg, t_in, t_out = H._c_cfg(PC.chain_cfg()), H._c_tip(None), _native.ChainTip()
    cv, cg, cp = lv.c_struct(), g.c_struct(), pv.c_struct()
    cs, id_out, slot_out, n_out, _keep = P._state_args(P.PBftState(), pv.window)
    head = (ptr(buf), buf.size, ptr(off), ptr(ln), n, spkp, -1, None, None, None,
            ctypes.byref(c_cfg), ctypes.byref(t_in), ptr(proto), ptr(status), ptr(verdict), ptr(be),
            ptr(bl), None, ptr(hh), ptr(env), ctypes.byref(t_out))

    def run_old():
        assert old.ouro_chain_validate_cbor(*head) == 0

    def run_new():
        assert lib.ouro_chain_validate_ledger_pbft_cbor(
            *head, ctypes.byref(cv), None, ctypes.byref(cg), None, None, None, ptr(ledger),
            ptr(rows), ctypes.byref(cp), ctypes.byref(cs), ptr(id_out), ptr(slot_out),
            ctypes.addressof(n_out), ptr(pb), ptr(prow), ptr(cnt)) == 0

    t = {"old": [], "new": []}
    for r in range(reps + 2):
        for name, fn in (("old", run_old), ("new", run_new)):
            t0 = time.perf_counter()
            fn()
            if r >= 2:
                t[name].append(1e3 * (time.perf_counter() - t0))
    assert (verdict == 1).all() and int((pb & P.PBFT_DELEGATE_KNOWN != 0).sum()) > 0.99 * n
    med = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({
        "n": n, "old": "parent ouro_chain_validate_cbor" if old is not lib else
        "this library's ouro_chain_validate_cbor", "new": "ouro_chain_validate_ledger_pbft_cbor",
        "old_ms": [round(x, 2) for x in t["old"]], "new_ms": [round(x, 2) for x in t["new"]],
        "old_median": round(med["old"], 2), "new_median": round(med["new"], 2),
        "old_spread": round(max(t["old"]) - min(t["old"]), 2),
        "delta_pct": round(100 * (med["new"] / med["old"] - 1), 2),
        "known_rows": int((pb & P.PBFT_DELEGATE_KNOWN != 0).sum()), "window_after": n_out.value}))


if __name__ == "__main__":
    main()
