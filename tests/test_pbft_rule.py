"""The Byron ledger-view checks on the host: the library's host path
(csrc/sha3.h, csrc/pbft_view.h, ouro_pbft_window_fold) against hashlib and the
plain-Python restatement pbft.pbft_rule, and both against the reference's
golden files (tests/golden/reference_pbft.json: the golden header is signed by
a delegate of the golden ledger state, which pins the hash and the direction
of the lookup end to end).  No GPU."""
import collections
import ctypes
import hashlib
import os

import numpy as np
import pytest

import pbft_cases as PC
from ouroboros_network_amd import _native
from ouroboros_network_amd import pbft as P
from ouroboros_network_amd._native import LV_NO_POOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ouroboros-network_amd", "lib", "libouro_devhost_test.so")


@pytest.fixture(scope="module")
def dh():
    lib = ctypes.CDLL(SO)
    lib.dh_sha3_256_short.restype = ctypes.c_int
    lib.dh_sha3_256_short.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
    lib.dh_byron_key_hash.restype = None
    lib.dh_byron_key_hash.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.dh_pbft_check.restype = ctypes.c_int
    lib.dh_pbft_check.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64,
                                  ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    return lib


# ---- the hashes -----------------------------------------------------------------

def test_sha3_256_short_every_length(dh):
    rng = np.random.default_rng(3)
    for n in range(136):
        for msg in (bytes(rng.integers(0, 256, n, dtype=np.uint8)), b"\xff" * n, bytes(n)):
            out = ctypes.create_string_buffer(32)
            assert dh.dh_sha3_256_short(out, msg, n) == 0
            assert out.raw == hashlib.sha3_256(msg).digest(), n
    assert dh.dh_sha3_256_short(ctypes.create_string_buffer(32), bytes(136), 136) == -1


def test_key_hash_pinned_by_the_golden_files(dh):
    g = PC.golden()
    assert g["header"]["genesis_id"].startswith("1a1ff703")
    assert g["header"]["genesis_id"].endswith("e54c67")
    assert g["header"]["delegate_id"].startswith("b30c3e09")
    assert g["header"]["delegate_id"].endswith("12f8f2")
    ks = [g["header"]["genesis_vk"], g["header"]["delegate_vk"], g["gen_tx"]["key"]]
    want = [g["header"]["genesis_id"], g["header"]["delegate_id"], g["gen_tx"]["id"]]
    x = np.frombuffer(bytes.fromhex("".join(ks)), np.uint8).reshape(3, 64)
    got = P.byron_key_hash(x, host=True)
    assert [r.tobytes().hex() for r in got] == want
    assert [P.key_hash(bytes.fromhex(k)).hex() for k in ks] == want
    for k, w in zip(ks, want):
        out = ctypes.create_string_buffer(28)
        dh.dh_byron_key_hash(out, bytes.fromhex(k))
        assert out.raw.hex() == w
    # the golden header's pair is one entry of the golden ledger state's map,
    # genesis id first; the golden window's signer is the GenTx key
    assert [want[0], want[1]] in g["delegation_map"]
    assert want[2] in g["chain_dep_state"]


def test_key_hash_seeded_keys():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, (1000, 64), dtype=np.uint8)
    x[0], x[1] = 0, 255
    got = P.byron_key_hash(x, host=True)
    for i in range(1000):
        assert got[i].tobytes() == P.key_hash(x[i].tobytes()), i
    assert P.byron_key_hash(np.zeros((0, 64), np.uint8), host=True).shape == (0, 28)


# ---- the golden header against the golden ledger state --------------------------

def test_golden_header_is_signed_by_a_delegate_of_the_golden_ledger_state(dh):
    g = PC.golden()
    v = PC.golden_views()
    vk = np.frombuffer(bytes.fromhex(g["header"]["delegate_vk"]), np.uint8).reshape(1, 64)
    bits, row, _ = P.pbft_checks(vk, [5], [PC.OK], v, host=True)
    assert bits[0] == P.PBFT_DELEGATE_KNOWN
    assert v.genesis_of_row(int(row[0])).hex() == g["header"]["genesis_id"]
    assert v.delegate_id[int(row[0])].tobytes().hex() == g["header"]["delegate_id"]
    cv, r = v.c_struct(), ctypes.c_uint32(0)
    assert dh.dh_pbft_check(ctypes.addressof(cv), vk.tobytes(), 5, PC.OK,
                            ctypes.byref(r)) == P.PBFT_DELEGATE_KNOWN
    assert r.value == row[0]
    # the genesis key itself is no delegate: the lookup runs delegate -> genesis
    gk = np.frombuffer(bytes.fromhex(g["header"]["genesis_vk"]), np.uint8).reshape(1, 64)
    bits, row, _ = P.pbft_checks(gk, [5], [PC.OK], v, host=True)
    assert bits[0] == 0 and row[0] == LV_NO_POOL
    for byte in (0, 31, 32, 63):
        bad = vk.copy()
        bad[0, byte] ^= 1
        bits, row, _ = P.pbft_checks(bad, [5], [PC.OK], v, host=True)
        assert bits[0] == 0 and row[0] == LV_NO_POOL
        assert dh.dh_pbft_check(ctypes.addressof(cv), bad.tobytes(), 5, PC.OK,
                                ctypes.byref(r)) == 0 and r.value == LV_NO_POOL


def test_golden_chain_dep_state_round_trips():
    g = PC.golden()
    raw = bytes.fromhex(g["chain_dep_state"])
    assert len(raw) == 39
    st = P.PBftState.from_cbor(raw)
    assert st.signers == [(s, bytes.fromhex(g["gen_tx"]["id"])) for s in (1, 2, 3, 4)]
    assert g["gen_tx"]["id"].startswith("b4c0e081")
    assert st.to_cbor() == raw
    # two keys, interleaved: decoding sorts by slot, encoding puts each key's
    # slots newest first under ascending keys
    a, b = b"\x01" * 28, b"\x02" * 28
    st2 = P.PBftState([(3, b), (5, a), (5, b), (300, a), (70000, b)])
    assert P.PBftState.from_cbor(st2.to_cbor()).signers == [(3, b), (5, a), (5, b), (300, a),
                                                           (70000, b)]
    assert P.PBftState.from_cbor(P.PBftState().to_cbor()).signers == []
    with pytest.raises(ValueError):
        P.PBftState.from_cbor(b"\x82\x00\xa0")


# ---- the host entries against the restatement -----------------------------------

# (ngen, k, window, threshold): the threshold sits near each set's mean count so
# that rows land on both sides of it
CONFIGS = [(1, 1, 10, 7), (1, 3, 10, 7), (3, 1, 10, 3), (3, 3, 10, 3), (7, 1, 10, 1), (7, 3, 10, 1)]


def test_host_entries_equal_the_rule_on_seeded_rows():
    seen = collections.Counter()
    total = 0
    for c, (ngen, k, window, threshold) in enumerate(CONFIGS):
        v = PC.schedule(ngen, k, window, threshold)
        vk, slot, status = PC.rows(340, ngen, k, 100 + c)
        total += len(slot)
        keys = [r.tobytes() for r in vk]
        wb, wr, wc, wst = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), P.PBftState())
        gb, gr, gc, gst = P.pbft_checks(vk, slot, status, v, state=P.PBftState(), host=True)
        assert (gb == wb).all() and (gr == wr).all() and (gc == wc).all() and gst == wst
        # without a state: the lookup alone
        nb, nr, nc = P.pbft_checks(vk, slot, status, v, host=True)
        lb, lr, _, _ = P.pbft_rule(v, keys, slot.tolist(), status.tolist())
        assert (nb == lb).all() and (nr == lr).all() and not nc.any()
        # the fold entry over the lookup's results is the same fold
        fb, fc, fst = P.pbft_window_fold(nb, nr, slot, v, P.PBftState())
        assert (fb == wb).all() and (fc == wc).all() and fst == wst
        seen.update(PC.outcome(b, s) for b, s in zip(wb, status))
        if k == 3:  # key 0: a delegate in entries 0 and 2, nobody's in entry 1
            rows0 = {int(r) for r, x in zip(wr, keys) if x == keys_of(0) and r != LV_NO_POOL}
            assert len(rows0) == 2
    assert total >= 2000
    for name in ("all_ok", "over_threshold", "slot_back", "unknown_delegate", "boundary",
                 "tpraos", "unsliced"):
        assert seen[name] >= 50, (name, dict(seen))


def keys_of(i):
    return PC.keys(16)[0][i].tobytes()


# ---- the window's edges ----------------------------------------------------------

def _edge_views(window=5, threshold=2):
    _, ids = PC.keys(16)
    return P.PBftViews([(0, [(ids[i], PC.gen_id(i)) for i in range(3)])], window, threshold)


def _edge_rows():
    """40 regular rows of delegates 0, 1, 2 (genesis A, B, C)"""
    kk, _ = PC.keys(16)
    who = [0, 0, 0, 1, 2, 0, 1, 1, 1, 2] + [int(x) for x in
                                            np.random.default_rng(5).integers(0, 3, 30)]
    slot = [10, 10, 11, 12, 13, 14, 15, 15, 14, 14] + list(range(16, 46))
    slot[20], slot[21] = 30, 29   # one more step back, later on
    vk = np.stack([kk[w] for w in who])
    return vk, np.array(slot, np.uint64), np.zeros(40, np.uint8), who


def test_window_edges_by_hand():
    v = _edge_views()
    vk, slot, status, _ = _edge_rows()
    A = P.PBFT_DELEGATE_KNOWN | P.PBFT_SLOT_OK | P.PBFT_WINDOW_OK
    bits, rows, cnt, st = P.pbft_checks(vk[:10], slot[:10], status[:10], v, state=P.PBftState(),
                                        host=True)
    # A A A B C | A B B B C with window 5, threshold 2:
    #   A's count 1, 2 (= threshold: ok), 3 (threshold + 1: over); B 1; C 1: the
    #   window is full (5) and nothing was dropped so far; the 6th row drops the
    #   oldest A: A's count stays 3 (4 if the trim began one row late)
    assert cnt.tolist() == [1, 2, 3, 1, 1, 3, 2, 3, 3, 1]
    over = A & ~P.PBFT_WINDOW_OK
    back = A & ~P.PBFT_SLOT_OK
    #   slots 10 10 11 12 13 14 15 15 14 14: equal slots pass, 15 -> 14 fails, and
    #   14 -> 14 passes again (the last signed slot is the one appended as given)
    assert bits.tolist() == [A, A, over, A, A, over, A, over, over & back, A]
    assert len(st.signers) == 5 and [s for s, _ in st.signers] == [14, 15, 15, 14, 14]
    for m, n_out in ((4, 4), (5, 5), (6, 5)):  # the trim begins exactly when the window is full
        _, _, _, s = P.pbft_checks(vk[:m], slot[:m], status[:m], v, state=P.PBftState(), host=True)
        assert len(s.signers) == n_out


def test_window_incoming_states_and_chaining():
    v = _edge_views()
    vk, slot, status, _ = _edge_rows()
    keys = [r.tobytes() for r in vk]
    X = b"\x77" * 28  # an id no entry knows: it still counts, and it is dropped in its turn
    for st0 in (P.PBftState(), P.PBftState([(1, PC.gen_id(0))] * 4),
                P.PBftState([(1, PC.gen_id(0)), (2, PC.gen_id(1))] * 2 + [(3, PC.gen_id(2))]),
                P.PBftState([(1, X)] * 5)):
        want = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), st0)
        got = P.pbft_checks(vk, slot, status, v, state=st0, host=True)
        assert all((g == w).all() for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
        # two chained calls equal one call
        for cut in (1, 5, 17, 39):
            a = P.pbft_checks(vk[:cut], slot[:cut], status[:cut], v, state=st0, host=True)
            b = P.pbft_checks(vk[cut:], slot[cut:], status[cut:], v, state=a[3], host=True)
            for q in range(3):
                assert (np.concatenate([a[q], b[q]]) == want[q]).all()
            assert b[3] == want[3]
    got = P.pbft_checks(vk[:1], slot[:1], status[:1], v, state=P.PBftState([(1, X)] * 5), host=True)
    assert got[3].signers == [(1, X)] * 4 + [(10, PC.gen_id(0))] and got[2][0] == 1


def test_window_of_one():
    vk, slot, status, _ = _edge_rows()
    keys = [r.tobytes() for r in vk]
    for threshold, ok in ((0, False), (1, True)):
        v = _edge_views(1, threshold)
        got = P.pbft_checks(vk, slot, status, v, state=P.PBftState(), host=True)
        want = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), P.PBftState())
        assert all((g == w).all() for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
        assert (got[2] == 1).all() and len(got[3].signers) == 1
        assert all(bool(b & P.PBFT_WINDOW_OK) == ok for b in got[0])


def test_outputs_may_alias_the_inputs():
    v = _edge_views()
    vk, slot, status, _ = _edge_rows()
    st0 = P.PBftState([(1, PC.gen_id(0)), (2, PC.gen_id(1)), (3, PC.gen_id(2))])
    want = P.pbft_checks(vk, slot, status, v, state=st0, host=True)
    ids = np.zeros((5, 28), np.uint8)
    slots = np.zeros(5, np.uint64)
    for i, (s, g) in enumerate(st0.signers):
        ids[i], slots[i] = np.frombuffer(g, np.uint8), s
    n = ctypes.c_size_t(0)
    cs = _native.PBftStateC(3, ids.ctypes.data, slots.ctypes.data)
    cv = v.c_struct()
    bits, rows, cnt = np.zeros(40, np.uint8), np.zeros(40, np.uint32), np.zeros(40, np.uint64)
    lib = _native.load()
    a = np.ascontiguousarray(vk)
    rc = lib.ouro_pbft_ledger_checks_host(40, a.ctypes.data, slot.ctypes.data, status.ctypes.data,
                                          ctypes.byref(cv), ctypes.byref(cs), ids.ctypes.data,
                                          slots.ctypes.data, ctypes.addressof(n), bits.ctypes.data,
                                          rows.ctypes.data, cnt.ctypes.data)
    assert rc == 0 and (bits == want[0]).all() and (cnt == want[2]).all()
    assert [(int(slots[i]), ids[i].tobytes()) for i in range(n.value)] == want[3].signers
    # the fold entry likewise, from the lookup's bits
    ids2 = np.zeros((5, 28), np.uint8)
    slots2 = np.zeros(5, np.uint64)
    for i, (s, g) in enumerate(st0.signers):
        ids2[i], slots2[i] = np.frombuffer(g, np.uint8), s
    cs2 = _native.PBftStateC(3, ids2.ctypes.data, slots2.ctypes.data)
    b2 = (bits & P.PBFT_DELEGATE_KNOWN).astype(np.uint8)
    rc = lib.ouro_pbft_window_fold(40, rows.ctypes.data, slot.ctypes.data, ctypes.byref(cv),
                                   ctypes.byref(cs2), ids2.ctypes.data, slots2.ctypes.data,
                                   ctypes.addressof(n), b2.ctypes.data, None)
    assert rc == 0 and (b2 == want[0]).all()
    assert [(int(slots2[i]), ids2[i].tobytes()) for i in range(n.value)] == want[3].signers


def test_boundary_rows_leave_the_state_alone():
    v = _edge_views()
    vk, slot, _, _ = _edge_rows()
    status = np.full(40, PC.EBB, np.uint8)
    st0 = P.PBftState([(50, PC.gen_id(1))])
    bits, rows, cnt, st = P.pbft_checks(vk, slot, status, v, state=st0, host=True)
    assert (bits == (P.PBFT_BOUNDARY | P.PBFT_ALL_OK)).all() and (rows == LV_NO_POOL).all()
    assert not cnt.any() and st == st0
    bits, _, _ = P.pbft_checks(vk, slot, status, v, host=True)
    assert (bits == (P.PBFT_BOUNDARY | P.PBFT_ALL_OK)).all()
    for other in (PC.ECBOR, 2, 3, PC.ESHELLEY, 4, 5, 8):
        bits, rows, _, st = P.pbft_checks(vk, slot, np.full(40, other, np.uint8), v, state=st0,
                                          host=True)
        assert not bits.any() and (rows == LV_NO_POOL).all() and st == st0


# ---- OURO_EINVAL, before anything runs -------------------------------------------

def _call(v, state=None, n=1):
    vk = np.zeros((max(n, 1), 64), np.uint8)
    return P.pbft_checks(vk[:n], np.zeros(n, np.uint64), np.zeros(n, np.uint8), v, state=state,
                         host=True)


def test_einval():
    _, ids = PC.keys(16)
    a, b = sorted(ids[:2])
    ok = [(0, [(a, PC.gen_id(0)), (b, PC.gen_id(1))]), (10, [(a, PC.gen_id(0))])]
    _call(P.PBftViews(ok, 5, 2))                                    # the baseline passes
    bad = []
    bad.append(P.PBftViews([], 5, 2))                               # k = 0
    bad.append(P.PBftViews([(j, []) for j in range(4097)], 5, 2))   # k > OURO_EPOCHS_MAX
    bad.append(P.PBftViews([(1, ok[0][1])], 5, 2))                  # first_slot[0] != 0
    bad.append(P.PBftViews([ok[0], (0, ok[1][1])], 5, 2))           # not strictly increasing
    bad.append(P.PBftViews([ok[0], (10, ok[1][1]), (10, [])], 5, 2))
    bad.append(P.PBftViews(ok, 0, 2))                               # window = 0
    bad.append(P.PBftViews([(0, [(b, PC.gen_id(0)), (a, PC.gen_id(1))])], 5, 2, sort=False))
    bad.append(P.PBftViews([(0, [(a, PC.gen_id(0)), (a, PC.gen_id(1))])], 5, 2, sort=False))
    bad.append(P.PBftViews([(0, [(a, PC.gen_id(0)), (b, PC.gen_id(0))])], 5, 2))  # genesis id twice
    v = P.PBftViews(ok, 5, 2)
    v.dlg_begin[0] = 1                                              # dlg_begin[0] != 0
    bad.append(v)
    v = P.PBftViews(ok, 5, 2)
    v.dlg_begin[1], v.dlg_begin[2] = 2, 1                           # decreasing
    bad.append(v)
    v = P.PBftViews(ok, 5, 2)
    v.dlg_begin[2] = (1 << 16) + 1                                  # > OURO_LV_GEN_ROWS_MAX
    bad.append(v)
    for i, v in enumerate(bad):
        with pytest.raises(ValueError):
            _call(v)
        with pytest.raises(ValueError):
            _call(v, n=0)                                           # before anything runs
        with pytest.raises(ValueError):
            P.pbft_window_fold([], [], [], v, P.PBftState())
    # NULL arrays
    lib = _native.load()
    good = P.PBftViews(ok, 5, 2)
    for field in ("first_slot", "dlg_begin", "delegate_id", "genesis_id"):
        cv = good.c_struct()
        setattr(cv, field, None)
        assert lib.ouro_pbft_ledger_checks_host(0, None, None, None, ctypes.byref(cv), None, None,
                                                None, None, None, None, None) == _native.OURO_EINVAL
    assert lib.ouro_pbft_ledger_checks_host(0, None, None, None, None, None, None, None, None,
                                            None, None, None) == _native.OURO_EINVAL
    cv = good.c_struct()
    z = np.zeros(64, np.uint8)
    assert lib.ouro_pbft_ledger_checks_host(1, None, z.ctypes.data, z.ctypes.data, ctypes.byref(cv),
                                            None, None, None, None, z.ctypes.data, None,
                                            None) == _native.OURO_EINVAL
    # the state: more signers than the window holds, NULL arrays, NULL outputs
    with pytest.raises(ValueError):
        _call(good, state=P.PBftState([(1, a)] * 6))
    _call(good, state=P.PBftState([(1, a)] * 5))
    cs = _native.PBftStateC(2, None, None)
    ids5, slots5, n = np.zeros((5, 28), np.uint8), np.zeros(5, np.uint64), ctypes.c_size_t(0)
    assert lib.ouro_pbft_ledger_checks_host(0, None, None, None, ctypes.byref(cv), ctypes.byref(cs),
                                            ids5.ctypes.data, slots5.ctypes.data,
                                            ctypes.addressof(n), None, None,
                                            None) == _native.OURO_EINVAL
    cs = _native.PBftStateC(0, None, None)
    for hole in range(3):
        outs = [ids5.ctypes.data, slots5.ctypes.data, ctypes.addressof(n)]
        outs[hole] = None
        assert lib.ouro_pbft_ledger_checks_host(0, None, None, None, ctypes.byref(cv),
                                                ctypes.byref(cs), *outs, None, None,
                                                None) == _native.OURO_EINVAL
        assert lib.ouro_pbft_window_fold(0, None, None, ctypes.byref(cv), ctypes.byref(cs), *outs,
                                         None, None) == _native.OURO_EINVAL
    assert lib.ouro_byron_key_hash_batch_host(1, None, None) == _native.OURO_EINVAL
    assert lib.ouro_pbft_views_upload(ctypes.byref(cv), None) == _native.OURO_EINVAL


# ---- the chain entry, host path ---------------------------------------------------

def _chain(raws, pv, state, host=True, **kw):
    lv, g, spkp = PC.trivial_ledger()
    return P.validate_chain_pbft_cbor(raws, spkp, -1, lv, g, pv, state=state, cfg=PC.chain_cfg(),
                                      host=host, **kw)


def _same_base(a, b):
    """crypto, hashes, envelope, tip, first invalid, OURO_LV_* bits and rows"""
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3] and a[4] == b[4]
    assert a[5].tobytes() == b[5].tobytes() and a[6].tobytes() == b[6].tobytes()


def _short_chain(stranger_at=None):
    spec = [("e", 0)] + [("r", 0, 1 + i, 3 if i == stranger_at else i % 3) for i in range(20)]
    spec += [("e", 1)] + [("r", 1, 2 + i, (i + 2) % 3) for i in range(9)]
    return PC.byron_chain(spec)


def test_chain_entry_null_schedule_is_the_overlay_entry():
    import ledger_cases as LC
    import overlay_cases as OC
    import envelope_cases as EC
    from ouroboros_network_amd import header as H
    from ouroboros_network_amd import ledger as L

    s = OC.chain_stream()
    kw = dict(genesis=s["genesis"], cfg=EC.VAL_CFG, epochs=s["epochs"], nonce=True, host=True)
    ref = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       counters=L.Counters(s["table_ids"], s["known"]), **kw)
    got = H.validate_chain_ledger_cbor(s["raws"], LC.SPKP, -1, s["views"], LC.G_CHAIN,
                                       counters=L.Counters(s["table_ids"], s["known"]),
                                       pbft=False, **kw)
    _same_base(ref, got)
    assert ref[7].as_dict() == got[7].as_dict() and len(got) == len(ref)


def test_chain_entry_signed_byron_chain_and_an_undelegated_signer():
    pv = PC.chain_views(8, 3)
    raws = _short_chain()
    st0 = P.PBftState([(0, PC.gen_id(2))])
    got = _chain(raws, pv, st0)
    want = PC.expect_pbft(raws, pv, PC.chain_cfg(), st0)
    n = len(raws)
    assert (got[0][0] == 0).all() and (got[0][2] == 1).all()      # PBFT rows, every verdict 1
    for q in range(3):
        np.testing.assert_array_equal(got[8 + q], want[q])
    assert got[11] == want[3]
    assert ((got[8] & P.PBFT_ALL_OK) == P.PBFT_ALL_OK).all()       # full ALL_OK, EBBs included
    assert (got[8][[0, 21]] == (P.PBFT_BOUNDARY | P.PBFT_ALL_OK)).all()
    assert (got[5] == 0).all()                                     # no TPraos row: no OURO_LV_* bit
    # without a state: the lookup alone; without the genesis_row / count buffers too
    nb = _chain(raws, pv, None)
    np.testing.assert_array_equal(nb[8], PC.expect_pbft(raws, pv, PC.chain_cfg(), None)[0])
    assert nb[11] is None and not nb[10].any()
    # the other outputs are the overlay entry's
    lv, g, spkp = PC.trivial_ledger()
    from ouroboros_network_amd import header as H
    ref = H.validate_chain_ledger_cbor(raws, spkp, -1, lv, g, cfg=PC.chain_cfg(), host=True)
    _same_base(ref, got)
    # the header the library accepted so far: header 7 re-signed by a key that
    # is nobody's delegate -- its signature verifies, the lookup says no
    bad = _short_chain(stranger_at=6)
    assert bad[7] != raws[7] and n == len(bad)
    got = _chain(bad, pv, st0)
    want = PC.expect_pbft(bad, pv, PC.chain_cfg(), st0)
    assert (got[0][2] == 1).all()
    assert got[8][7] == 0 and got[9][7] == LV_NO_POOL and want[0][7] == 0
    for q in range(3):
        np.testing.assert_array_equal(got[8 + q], want[q])
    assert got[11] == want[3] and len(got[11].signers) == 8
    # two chained calls equal one call (the tip and the window carried over)
    a = _chain(bad[:11], pv, st0)
    b = _chain(bad[11:], pv, a[11], tip=a[3])
    for q in range(3):
        np.testing.assert_array_equal(np.concatenate([a[8 + q], b[8 + q]]), want[q])
    assert b[11] == want[3]
    # n = 0: the window passes through; a bad schedule is refused first
    assert _chain([], pv, st0)[11] == st0
    with pytest.raises(ValueError):
        _chain(raws, P.PBftViews([(0, [])], 0, 1), st0)
    with pytest.raises(ValueError):
        _chain(raws, pv, P.PBftState([(0, PC.gen_id(0))] * 9))
