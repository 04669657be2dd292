"""What the ledger-view checks cost on one GPU (ouro_chain_validate_ledger_cbor,
ouro_tpraos_ledger_checks_device), over synthetic node-configuration raw
headers in pageable host memory as tools/chain_replay.py builds them.  The two
sides of a leg are alternated on the same buffer in the same process; one JSON
object per leg.
    python tools/ledger_view.py [n] [reps] [legs] [parent library]
legs (comma separated, default all):
  existing  ouro_chain_validate_cbor on n TPraos headers: this library against
            the parent commit's (the path given as the fourth argument; skipped
            without it) -- existing callers lose nothing
  ledger    ouro_chain_validate_ledger_cbor against ouro_chain_validate_cbor on
            n TPraos headers, under 50 view entries of 3,000 pools each (the
            stream's pools among them) and a counters table
  device    k_ledger_checks alone (ouro_tpraos_ledger_checks_device) on the n
            sliced rows resident on the device, timed with stream events
  existing_ledger  ouro_chain_validate_ledger_cbor (no genesis-delegation
            schedule): this library against the parent commit's, twice: this
            library first in every pair, then the parent's first
  overlay   ouro_chain_validate_ledger_overlay_cbor with a schedule (7 genesis
            keys per entry, the stream's first pools as delegates, asc_inv = 20)
            against ouro_chain_validate_ledger_cbor, both under d = 1/2
  device_overlay  k_ledger_checks_overlay against k_ledger_checks on the
            resident rows under d = 1/2"""
import ctypes
import json
import os
import statistics
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import chain_replay as CR  # noqa: E402

P = CR.P
SPKP = CR.SPKP
ENTRIES, POOLS = 50, 3000


def report(leg, n, new, old, **kw):
    r = lambda x: [round(t, 2) for t in x]  # noqa: E731
    print(json.dumps({"leg": leg, "n": n, "new_ms": r(new), "old_ms": r(old),
                      "new_median": round(statistics.median(new), 2),
                      "old_median": round(statistics.median(old), 2),
                      "old_spread": round(max(old) - min(old), 2),
                      "delta_pct": round(100 * (statistics.median(new) / statistics.median(old)
                                                - 1), 2), **kw}), flush=True)


def main():
    import torch

    from ouroboros_network_amd import _native
    from ouroboros_network_amd import ledger as L
    from ouroboros_network_amd.tpraos import EpochNonces

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    legs = (sys.argv[3] if len(sys.argv) > 3 else
            "existing,ledger,device,existing_ledger,overlay,device_overlay").split(",")
    parent = sys.argv[4] if len(sys.argv) > 4 else None
    dev = torch.device("cuda", 0)
    lib = _native.load()
    lib.ouro_bind_thread_to_device(0)
    one = EpochNonces(first_slot=[0], nonce=[CR.nonce_of(0)])
    cfg = _native.EnvelopeCfg(byron_epoch_slots=21600)
    tbuf, rl = CR.segment(n, 0, dev, whole=True)
    s = CR.Stream.fixed(tbuf, rl)
    s.hh = np.zeros((s.n, 32), np.uint8)
    s.env = np.zeros(s.n, np.uint8)
    s.ledger = np.zeros(s.n, np.uint8)
    s.prow = np.zeros(s.n, np.uint32)

    def validate(which=lib):
        rc = which.ouro_chain_validate_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, -1,
                                            ctypes.byref(one.c_struct()), None, None,
                                            ctypes.byref(cfg), None, P(s.proto), P(s.st), P(s.v),
                                            P(s.be), P(s.bl), None, P(s.hh), P(s.env), None)
        assert rc == 0, which.ouro_last_error()

    if "existing" in legs and parent:
        old = ctypes.CDLL(parent)
        for name in ("ouro_chain_validate_cbor", "ouro_last_error"):
            res, args = _native.SIGNATURES[name]
            getattr(old, name).restype, getattr(old, name).argtypes = res, args
        tn, to = CR.alternate(validate, lambda: validate(old), reps)
        report("existing", s.n, tn, to, what="ouro_chain_validate_cbor: this library / the parent's")

    # the stream's rows (host slicer): its pools go into every entry
    arena = np.zeros(lib.ouro_tpraos_pack_bytes(s.n), np.uint8)
    b = _native.TPraosBatch()
    slot = np.zeros(s.n, np.uint64)
    pst = np.zeros(s.n, np.uint8)
    rc = lib.ouro_tpraos_pack_cbor(P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, P(arena),
                                   arena.size, ctypes.byref(b), P(slot), None, P(pst), 0)
    assert rc == 0 and not pst.any()

    def col(addr, dt, w):
        a = np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint8)),
                                  shape=(s.n * w * np.dtype(dt).itemsize,))
        return a.view(dt).reshape(s.n, w) if w > 1 else a.view(dt)

    issuer = col(b.issuer_vk, np.uint8, 32)
    vrf = col(b.vrf_vk, np.uint8, 32)
    lead = col(b.leader_output, np.uint8, 64)
    c0 = col(b.ocert_kes_period, np.uint64, 1)
    pairs = {bytes(r[:32]): bytes(r[32:]) for r in np.unique(np.concatenate([issuer, vrf], 1),
                                                             axis=0)}
    rng = np.random.default_rng(1)
    pools = [L.Pool(L.pool_id(c), L.vrf_key_hash(v), (1, POOLS)) for c, v in pairs.items()]
    assert len(pools) <= POOLS
    fill = [L.Pool(rng.bytes(28), rng.bytes(32), (1, POOLS)) for _ in range(POOLS - len(pools))]
    top = int(slot.max()) + 1
    views = L.LedgerViews([L.Entry(j * top // ENTRIES, (0, 1), tuple(pools + fill))
                           for j in range(ENTRIES)])
    g = L.Globals(SPKP, 2**32, L._oracle_leader().active_slot_log(Fraction(1, 20)))
    table = L.Counters(views.all_pool_ids())
    cv, cg, cc = views.c_struct(), g.c_struct(), table.c_struct()
    co, po = np.zeros_like(table.counter), np.zeros_like(table.present)

    def ledger(which=lib, cv=cv, gen=None):
        name, extra = "ouro_chain_validate_ledger_cbor", ()
        if gen is not None:
            name, extra = "ouro_chain_validate_ledger_overlay_cbor", (ctypes.byref(gen),)
        rc = getattr(which, name)(
            P(s.buf), s.buf.size, P(s.off), P(s.ln), s.n, SPKP, -1, ctypes.byref(one.c_struct()),
            None, None, ctypes.byref(cfg), None, P(s.proto), P(s.st), P(s.v), P(s.be), P(s.bl),
            None, P(s.hh), P(s.env), None, ctypes.byref(cv), *extra, ctypes.byref(cg),
            ctypes.byref(cc), P(co), P(po), P(s.ledger), P(s.prow))
        assert rc == 0, which.ouro_last_error()

    def hist():
        return {hex(int(k)): int(v) for k, v in zip(*np.unique(s.ledger, return_counts=True))}

    if "existing_ledger" in legs and parent:
        old = ctypes.CDLL(parent)
        for name in ("ouro_chain_validate_ledger_cbor", "ouro_last_error"):
            res, args = _native.SIGNATURES[name]
            getattr(old, name).restype, getattr(old, name).argtypes = res, args
        tn, to = CR.alternate(ledger, lambda: ledger(old), reps)
        report("existing_ledger", s.n, tn, to,
               what="ouro_chain_validate_ledger_cbor: this library / the parent's")
        # the same with the parent's call first in every pair
        to, tn = CR.alternate(lambda: ledger(old), ledger, reps)
        report("existing_ledger", s.n, tn, to,
               what="ouro_chain_validate_ledger_cbor: this library / the parent's, parent first")

    # the overlay legs: the same pools under d = 1/2, 7 genesis keys per entry
    # whose delegates are the stream's first pools (their ids are in the table)
    views_h = L.LedgerViews([L.Entry(e.first_slot, (1, 2), e.pools) for e in views.entries])
    cvh = views_h.c_struct()
    dl = (pools + fill)[:7]
    gen_h = L.GenesisDelegs([tuple(L.GenDeleg(bytes([i]) * 28, p.pool_id, p.vrf_hash)
                                   for i, p in enumerate(dl))] * ENTRIES, 20)
    cgen = gen_h.c_struct()
    if "overlay" in legs:
        tn, to = CR.alternate(lambda: ledger(cv=cvh, gen=cgen), lambda: ledger(cv=cvh), reps)
        ledger(cv=cvh, gen=cgen)
        report("overlay", s.n, tn, to,
               what="ouro_chain_validate_ledger_overlay_cbor / ouro_chain_validate_ledger_cbor, "
                    "d = 1/2", genesis_keys=7, asc_inv=20, bits=hist())

    if "ledger" in legs:
        tn, to = CR.alternate(ledger, validate, reps)
        ledger()
        report("ledger", s.n, tn, to,
               what="ouro_chain_validate_ledger_cbor / ouro_chain_validate_cbor",
               entries=ENTRIES, pools_per_entry=POOLS, stream_pools=len(pools), bits=hist(),
               all_valid=bool(((s.v & 0x3F) == 0x3F).all()),
               view_bytes=int(28 + 32 + 16) * views.rows)

    if "device" in legs or "device_overlay" in legs:
        d = [torch.tensor(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64
                          else np.ascontiguousarray(a), device=dev)
             for a in (issuer, vrf, slot, lead, c0)]
        out = torch.zeros(s.n, dtype=torch.uint8, device=dev)
        rows = torch.zeros(s.n, dtype=torch.int32, device=dev)
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def kernel_leg(leg, cv, gen, **kw):
            h = ctypes.c_void_p()
            assert lib.ouro_ledger_views_upload_overlay(ctypes.byref(cv), gen, ctypes.byref(h)) == 0

            def kern():
                rc = lib.ouro_tpraos_ledger_checks_device(sp, s.n, *[t.data_ptr() for t in d], h,
                                                          ctypes.byref(cg), out.data_ptr(),
                                                          rows.data_ptr())
                assert rc == 0, lib.ouro_last_error()

            kern()
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                kern()
                e.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(e))
            lib.ouro_ledger_views_free(h)
            med = statistics.median(ms)
            print(json.dumps({"leg": leg, "n": s.n, "kernel_ms": [round(x, 3) for x in ms],
                              "kernel_median_ms": round(med, 3),
                              "headers_per_s": round(s.n / med * 1e3),
                              "known": int((out & 1).sum().item()),
                              "leader_ok": int(((out & 4) != 0).sum().item()),
                              "overlay": int(((out & 0x40) != 0).sum().item()),
                              "overlay_active": int(((out & 0x20) != 0).sum().item()), **kw}),
                  flush=True)

        if "device" in legs:
            kernel_leg("device", cv, None)
        if "device_overlay" in legs:
            kernel_leg("device_overlay", cvh, None, kernel="k_ledger_checks, d = 1/2")
            kernel_leg("device_overlay", cvh, ctypes.byref(cgen),
                       kernel="k_ledger_checks_overlay, d = 1/2, 7 keys, asc_inv = 20")


if __name__ == "__main__":
    main()
