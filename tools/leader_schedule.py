#!/usr/bin/env python3
"""One epoch's leader schedule: slots/s of ouro_tpraos_leader_schedule on the
GPU and of ouro_tpraos_leader_schedule_host on --host-threads host threads
(default 16; DESIGN.md §5, profiles/leader_schedule/).

Workload: 432,000 consecutive slots (one mainnet epoch) under one seeded VRF
key, sigma = 1/100, f = 1/20, a fixed epoch nonce, no overlay; class, genesis
index and the 64-byte output of every slot are returned.  For orientation
`ed_alone` times ouro_ed25519_verify_batch on as many seeded signatures: a
schedule lane does one Elligator2, one 253-bit variable-base chain, one
inversion and two SHA-512, about one verification's work.

Runs, alternated within one process (each warmed up; every repetition printed):
  device   the host-buffer entry: launch, copy back, synchronise;
  host     the *_host entry on the worker pool, the whole epoch by default
           (--host-slots fewer: scaled to the epoch, and the summary says so).
           The pool's width is set here, through OURO_HOST_THREADS before the
           library loads (it reads its switches once), and recorded with the
           CPUs the process may run on;
  ed_alone ouro_ed25519_verify_batch, host buffers, on --slots signatures.
Times are host clocks around calls that return after a device synchronise.
The device's classes and outputs are checked against the host's on the slots
the host ran before any time is reported.  One JSON line per measurement on
stdout; --summary writes the medians.
"""
import argparse
import json
import os
import statistics
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

L_ONE_TWENTIETH = -512932943875505334261961442546873     # floor(10^34 ln(1 - 1/20))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=432_000)
    ap.add_argument("--host-slots", type=int, default=432_000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summary", default=None)
    a = ap.parse_args()

    os.environ["OURO_HOST_THREADS"] = str(a.host_threads)
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torch.cuda.init()
    import oracle_ffi as O
    from ouroboros_network_amd import Ed25519DSIGN, PraosVRF
    from ouroboros_network_amd.leader import ActiveSlotCoeff, leader_schedule

    _, sk = PraosVRF.keypair_from_seed(bytes(range(32)))
    eta0 = bytes(reversed(range(32)))
    f = ActiveSlotCoeff(L_ONE_TWENTIETH)
    sigma = Fraction(1, 100)
    first = 4_924_800

    def device():
        return leader_schedule(sk, eta0, first, a.slots, sigma, f)

    def host():
        return leader_schedule(sk, eta0, first, a.host_slots, sigma, f, host=True)

    d, h = device(), host()
    m = min(a.slots, a.host_slots)
    for x, y in zip(d, h):
        assert (x[:m] == y[:m]).all(), "device and host schedules differ"
    winners = int((d[0] == 1).sum())
    emit(check="device == host", slots=m, winners_in_epoch=winners)

    pk, sig, msg = O.synth_ed25519(a.slots, first=1, threads=16)

    def ed():
        assert Ed25519DSIGN.verify_batch(pk, msg, sig).all()

    runs = {"device": (device, a.slots), "host": (host, a.host_slots), "ed_alone": (ed, a.slots)}
    times = {k: [] for k in runs}
    for rep in range(a.warmup + a.reps):
        for name, (fn, n) in runs.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= a.warmup:
                times[name].append(dt)
                emit(run=name, rep=rep - a.warmup, items=n, seconds=dt, items_per_s=n / dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    summary = {
        "slots": a.slots, "host_slots": a.host_slots, "reps": a.reps,
        "host_threads": a.host_threads, "host_cpus_in_affinity": len(os.sched_getaffinity(0)),
        "host_scaled": a.host_slots != a.slots,
        "device_epoch_s": med["device"],
        "device_spread_s": [min(times["device"]), max(times["device"])],
        "host_epoch_s": med["host"] * a.slots / a.host_slots,
        "host_spread_s": [min(times["host"]) * a.slots / a.host_slots,
                          max(times["host"]) * a.slots / a.host_slots],
        "ed_alone_s": med["ed_alone"],
        "device_slots_per_s": a.slots / med["device"],
        "host_slots_per_s": a.host_slots / med["host"],
        "device_over_host": (med["host"] * a.slots / a.host_slots) / med["device"],
        "device_ns_per_slot": 1e9 * med["device"] / a.slots,
        "ed_alone_ns_per_item": 1e9 * med["ed_alone"] / a.slots,
        "winners_in_epoch": winners,
    }
    emit(summary=summary)
    if a.summary:
        os.makedirs(os.path.dirname(os.path.abspath(a.summary)), exist_ok=True)
        with open(a.summary, "w") as fh:
            json.dump(summary, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
