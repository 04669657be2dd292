"""The header envelope rule (CPU-only): ouroboros_network_amd.envelope pinned
to the reference's golden fixtures, and the library's host path
(ouro_chain_envelope_cbor_host: csrc/envelope.h envelope_link, both slicers'
envelope records, the host build of the prefixed Blake2b-256) against
envelope.py on every branch of the rule.  Expected bits are written out by
hand where a case is about one branch, so envelope.py is checked too."""
import ctypes

import numpy as np
import pytest

import envelope_cases as EC
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as B
from ouroboros_network_amd import envelope as E
from ouroboros_network_amd import header as H

BN, SL, PH, EX, ALL = E.ENV_BLOCKNO_OK, E.ENV_SLOT_OK, E.ENV_PREVHASH_OK, E.ENV_EXTRA_OK, \
    E.ENV_ALL_OK
CFG = E.Cfg(EC.EPOCH_SLOTS)
P = bytes(range(32))  # some previous hash


def host(raws, tip=E.ORIGIN, cfg=CFG):
    return H.chain_envelope_cbor(raws, cfg, tip, host=True)


def assert_matches_python(raws, tip=E.ORIGIN, cfg=CFG):
    """the host path = envelope.py on this stream; returns the bits"""
    st, hh, bits, tip_out = host(raws, tip, cfg)
    usable, hashes, want, want_tip = EC.expect(raws, tip, cfg)
    for i, r in enumerate(raws):
        if H.era_class(r) == H.PROTO_PBFT:
            assert st[i] == B.byron_status(r)[0], i
        else:
            assert (st[i] == H.PACK_OK) == usable[i], i
    assert [bytes(h) for h in hh] == hashes
    assert list(bits) == want
    assert tip_out == want_tip
    return list(bits)


# ---- pinned by the reference's fixtures ---------------------------------------
def test_byron_hashes_and_the_ebb_link_are_the_golden_ones():
    fx = EC.fixtures()
    reg, ebb = bytes.fromhex(fx["byron_regular_header"]), bytes.fromhex(fx["byron_ebb_header"])
    golden = H.bytes_at(bytes.fromhex(fx["header_hash_byron"]), 0)
    tip = H.array_items(bytes.fromhex(fx["ann_tip_byron"]), 0)
    tip_hash = H.bytes_at(bytes.fromhex(fx["ann_tip_byron"]),
                          H.array_items(bytes.fromhex(fx["ann_tip_byron"]), tip[1][0])[1][0])
    assert tip_hash == golden
    for form in (1, 2, 3):
        r, e = EC.byron_wire(1, reg, form), EC.byron_wire(0, ebb, form)
        assert E.header_hash(r) == golden
        rr, er = E.header_record(r, CFG), E.header_record(e, CFG)
        # the golden regular block's prevHash field is the golden EBB's hash
        assert rr.prev == er.hash == EC.b2b(b"\x82\x00" + ebb)
        assert (er.is_ebb, er.slot, er.block_no, er.prev) == (True, 0, 0, E.GENESIS)
        assert (rr.is_ebb, rr.slot, rr.block_no) == (False, 1, 1)
        # EBB at Origin, then the regular header: expectedNextBlockNo = succ 0,
        # minimumNextSlotNo = the EBB's own slot, the hashes link
        assert E.validate_envelope([e, r], E.ORIGIN, CFG)[2] == [ALL, ALL]
        assert assert_matches_python([e, r]) == [ALL, ALL]


def test_ann_tips_decode_as_tips():
    """the golden annotated tips: [era, [slot, hash, block_no(, isEBB)]]"""
    fx = EC.fixtures()
    for era, name in enumerate(("byron", "shelley", "allegra", "mary")):
        buf = bytes.fromhex(fx["ann_tip_" + name])
        top = H.array_items(buf, 0)
        assert H.uint_at(buf, top[0][0]) == era
        f = H.array_items(buf, top[1][0])
        assert len(f) == (4 if era == 0 else 3) and len(H.bytes_at(buf, f[1][0])) == 32
        tip = E.Tip(H.PROTO_PBFT if era == 0 else H.PROTO_TPRAOS, False, H.uint_at(buf, f[0][0]),
                    H.uint_at(buf, f[2][0]), H.bytes_at(buf, f[1][0]))
        # a TPraos header built on that tip links to it, in C as in Python
        raw, _ = EC.tpraos(tip.hash, tip.slot + 1, tip.block_no + 1)
        assert assert_matches_python([raw], tip) == [ALL]


# ---- every branch of the link rule ---------------------------------------------
def test_origin():
    ebb0, _ = EC.byron_ebb(bytes(32), 0, 0)
    assert assert_matches_python([ebb0]) == [ALL]
    t, _ = EC.tpraos(EC.GENESIS, 0, 0)
    assert assert_matches_python([t]) == [ALL]           # null = GenesisHash
    t, _ = EC.tpraos(EC.GENESIS, 7, 1)
    assert assert_matches_python([t]) == [SL | PH | EX]  # expectedFirstBlockNo = 0
    t, _ = EC.tpraos(P, 0, 0)
    assert assert_matches_python([t]) == [BN | SL | EX]  # a block hash at Origin
    r, _ = EC.byron_regular(P, 0, 0, 0)
    assert assert_matches_python([r]) == [BN | SL | EX]  # a regular Byron header never has GenesisHash
    e1, _ = EC.byron_ebb(P, 1, 0)
    assert assert_matches_python([e1]) == [BN | SL | EX]  # only the epoch-0 EBB has it


@pytest.mark.parametrize("form", [1, 2, 3])
def test_byron_ebb_and_regular_pairs(form):
    S = EC.EPOCH_SLOTS
    r0, h0 = EC.byron_regular(P, 0, 5, 9, form=form)
    tip = E.Tip(H.PROTO_PBFT, False, 4, 8, P)
    # non-EBB -> non-EBB: succ, succ
    assert assert_matches_python([r0], tip) == [ALL]
    r1, _ = EC.byron_regular(h0, 0, 5, 10, form=form)
    assert assert_matches_python([r0, r1], tip)[1] == BN | PH | EX      # the same slot
    # non-EBB -> EBB: the same block number, a later slot
    e, he = EC.byron_ebb(h0, 1, 9, form=form)
    assert assert_matches_python([r0, e], tip)[1] == ALL
    e_succ, _ = EC.byron_ebb(h0, 1, 10, form=form)
    assert assert_matches_python([r0, e_succ], tip)[1] == SL | PH | EX  # succ is wrong here
    # EBB -> non-EBB: succ, the same slot allowed
    r2, h2 = EC.byron_regular(he, 1, 0, 10, form=form)
    assert assert_matches_python([r0, e, r2], tip)[2] == ALL
    r2b, _ = EC.byron_regular(he, 0, S - 1, 10, form=form)
    assert assert_matches_python([r0, e, r2b], tip)[2] == BN | PH | EX   # a smaller slot
    r2c, _ = EC.byron_regular(he, 1, 0, 9, form=form)
    assert assert_matches_python([r0, e, r2c], tip)[2] == SL | PH | EX   # the EBB's own number
    # EBB -> EBB: succ, succ
    e2, _ = EC.byron_ebb(he, 2, 10, form=form)
    assert assert_matches_python([r0, e, e2], tip)[2] == ALL
    e2b, _ = EC.byron_ebb(he, 1, 9, form=form)
    assert assert_matches_python([r0, e, e2b], tip)[2] == PH | EX


def test_byron_to_shelley_is_succ_on_both():
    r0, h0 = EC.byron_regular(P, 3, 7, 9)
    e, he = EC.byron_ebb(h0, 4, 9)
    s0 = 4 * EC.EPOCH_SLOTS
    t, _ = EC.tpraos(he, s0 + 1, 10, era=1)
    assert assert_matches_python([r0, e, t])[2] == ALL
    t, _ = EC.tpraos(he, s0, 10, era=1)           # the EBB's slot: only Byron shares it
    assert assert_matches_python([r0, e, t])[2] == BN | PH | EX
    t, _ = EC.tpraos(h0, 3 * EC.EPOCH_SLOTS + 8, 9)  # a non-EBB's number: only an EBB shares it
    assert assert_matches_python([r0, t])[1] == SL | PH | EX


def test_slots_block_numbers_and_previous_hashes():
    t0, h0 = EC.tpraos(P, 100, 50)
    tip = E.Tip(H.PROTO_TPRAOS, False, 99, 49, P)
    cases = [
        (EC.tpraos(h0, 101, 51), ALL),
        (EC.tpraos(h0, 2**40, 51), ALL),
        (EC.tpraos(h0, 100, 51), BN | PH | EX),            # an equal slot
        (EC.tpraos(h0, 99, 51), BN | PH | EX),             # a smaller slot
        (EC.tpraos(h0, 101, 52), SL | PH | EX),            # block number off by one, up
        (EC.tpraos(h0, 101, 50), SL | PH | EX),            # and down
        (EC.tpraos(bytes(32), 101, 51), BN | SL | EX),     # a wrong previous hash
        (EC.tpraos(h0[:31] + bytes([h0[31] ^ 1]), 101, 51), BN | SL | EX),
        (EC.tpraos(EC.GENESIS, 101, 51), BN | SL | EX),    # GenesisHash past Origin
        (EC.tpraos(EC.C.cbor_bytes(h0[:31]), 101, 51), BN | SL | EX),     # bytes(31): malformed
        (EC.tpraos(b"\x00", 101, 51), BN | SL | EX),              # a uint: malformed
        (EC.tpraos(b"\xf7", 101, 51), BN | SL | EX),              # undefined, not null
    ]
    for (raw, _), want in cases:
        assert assert_matches_python([t0, raw], tip) == [ALL, want]
    # the largest Word64 has no successor
    tmax, hmax = EC.tpraos(P, 2**64 - 1, 2**64 - 1)
    nxt, _ = EC.tpraos(hmax, 2**64 - 1, 0)
    assert assert_matches_python([tmax, nxt], E.Tip(H.PROTO_TPRAOS, False, 5, 2**64 - 2, P)) == \
        [ALL, PH | EX]


def test_ebb_off_the_epoch_boundary():
    S = EC.EPOCH_SLOTS
    r0, h0 = EC.byron_regular(P, 0, 5, 9)
    e, _ = EC.byron_ebb(h0, 1, 9)
    tip = E.Tip(H.PROTO_PBFT, False, 4, 8, P)
    assert assert_matches_python([r0, e], tip) == [ALL, ALL]
    # slot = epoch * S is a multiple of S until the Word64 product wraps: the
    # first epoch whose product does lands on a slot that is none
    epoch = -(-2**64 // S)
    assert 0 < (epoch * S) % 2**64 < S
    e, _ = EC.byron_ebb(h0, epoch, 9)
    slot = epoch * S - 2**64
    assert E.header_record(e, CFG).slot == slot and slot > 5  # (r0 is in slot 5)
    assert assert_matches_python([r0, e], tip) == [ALL, BN | SL | PH]


def test_chain_checks_limits_at_one_under_and_one_over():
    t0, h0 = EC.tpraos(P, 100, 50)
    tip = E.Tip(H.PROTO_TPRAOS, False, 99, 49, P)
    raw, _ = EC.tpraos(h0, 101, 51, body_size=3000, prot_major=2)
    size = E.header_record(raw).header_size
    assert size > 800
    for dh in (-1, 0, 1):
        for db in (-1, 0, 1):
            for dv in (-1, 0, 1):
                cfg = E.Cfg(EC.EPOCH_SLOTS, (size + dh, 3000 + db, 2 + dv))
                want = ALL if min(dh, db, dv) >= 0 else BN | SL | PH
                assert assert_matches_python([t0, raw], tip, cfg)[1] == want, (dh, db, dv)
    # no limits: the bit is set; a field 7 that is no uint fails only under limits
    odd, _ = EC.tpraos(h0, 101, 51, body_size=b"\x40", prot_major=2)
    assert assert_matches_python([t0, odd], tip)[1] == ALL
    assert assert_matches_python([t0, odd], tip, E.Cfg(EC.EPOCH_SLOTS, (2**32, 2**32, 2**32)))[1] \
        == BN | SL | PH
    # limits do not touch Byron headers
    r0, _ = EC.byron_regular(P, 0, 5, 9)
    assert assert_matches_python([r0], E.Tip(H.PROTO_PBFT, False, 4, 8, P),
                                 E.Cfg(EC.EPOCH_SLOTS, (0, 0, 0))) == [ALL]


def test_unusable_headers_in_the_middle_and_at_position_zero():
    raws = EC.good_chain(6, 6)
    assert assert_matches_python(raws) == [ALL] * 12
    for pos in (0, 3, 8):
        cut = list(raws)
        cut[pos] = cut[pos][:-3]                       # truncated: the slicer rejects it
        bits = assert_matches_python(cut)
        assert bits[pos] == 0 and bits[pos + 1] == EX  # the successor: EXTRA alone
        assert bits[pos + 2:] == [ALL] * (10 - pos)
    # an EBB whose fields have another shape: accepted by the slicer, unusable here
    h1 = E.header_record(raws[1], CFG).hash
    for cons in (EC.arr(EC.C.cbor_uint(1)), EC.arr(EC.C.cbor_bytes(b"x"), EC.arr(EC.C.cbor_uint(1))),
                 EC.arr(EC.C.cbor_uint(1), EC.arr(EC.C.cbor_uint(1), EC.C.cbor_uint(2)))):
        bad, _ = EC.byron_ebb(h1, 1, 1, consensus=cons)
        st, hh, bits, _ = host(raws[:2] + [bad, raws[2]])
        assert st[2] == B.PACK_EBB and bits[2] == 0 and not hh[2].any() and bits[3] == EX
        assert_matches_python(raws[:2] + [bad, raws[2]])
    # a regular header whose slotId / difficulty have another shape
    for kw in (dict(slot_id=EC.C.cbor_uint(5)), dict(difficulty=EC.C.cbor_uint(5)),
               dict(difficulty=EC.arr())):
        bad, _ = EC.byron_regular(h1, 0, 1, 2, **kw)
        st, hh, bits, _ = host(raws[:2] + [bad])
        assert st[2] == B.PACK_OK and bits[2] == 0 and not hh[2].any()
        assert_matches_python(raws[:2] + [bad])


def test_one_stream_cut_at_every_position_chains_through_the_tip():
    raws = EC.good_chain(14, 26)
    assert len(raws) == 40
    raws[9] = raws[9][:-1]                              # unusable
    raws[20], _ = EC.tpraos(P, 5, 5)                    # links to nothing
    whole = assert_matches_python(raws)
    assert whole.count(ALL) == 36
    for cut in range(41):
        st1, hh1, b1, tip = host(raws[:cut])
        st2, hh2, b2, tip2 = host(raws[cut:], tip)
        assert list(b1) + list(b2) == whole, cut
        assert tip2 == EC.expect(raws)[3]
    assert E.first_invalid(whole) == 9


# ---- argument checks and struct layouts ------------------------------------------
def test_argument_checks():
    lib = _native.load()
    raws = EC.good_chain(3, 2)
    buf, off, ln = H.raw_triplet(raws)
    n = len(raws)
    st, hh, bits = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    cfg = _native.EnvelopeCfg(byron_epoch_slots=EC.EPOCH_SLOTS)
    tip = _native.ChainTip(origin=1)

    def call(cfg_=cfg, tip_=tip, st_=st, hh_=hh, bits_=bits, entry="ouro_chain_envelope_cbor_host",
             raw_bytes=buf.size):
        return getattr(lib, entry)(ptr(buf), raw_bytes, ptr(off), ptr(ln), n,
                                   ctypes.byref(cfg_) if cfg_ is not None else None,
                                   ctypes.byref(tip_) if tip_ is not None else None,
                                   ptr(st_) if st_ is not None else None,
                                   ptr(hh_) if hh_ is not None else None,
                                   ptr(bits_) if bits_ is not None else None, None)

    for entry in ("ouro_chain_envelope_cbor_host", "ouro_chain_envelope_cbor"):
        # (every one is refused before a device is looked for)
        assert call(hh_=None, entry=entry) == _native.OURO_EINVAL
        assert call(bits_=None, entry=entry) == _native.OURO_EINVAL
        assert call(st_=None, entry=entry) == _native.OURO_EINVAL
        assert call(cfg_=None, entry=entry) == _native.OURO_EINVAL
        assert call(cfg_=_native.EnvelopeCfg(), entry=entry) == _native.OURO_EINVAL  # PBFT, 0 slots
        assert call(tip_=_native.ChainTip(origin=1, slot=1), entry=entry) == _native.OURO_EINVAL
        assert call(tip_=_native.ChainTip(origin=1, proto=1), entry=entry) == _native.OURO_EINVAL
        assert call(tip_=_native.ChainTip(proto=2), entry=entry) == _native.OURO_EINVAL
        assert call(tip_=_native.ChainTip(proto=1, is_ebb=1), entry=entry) == _native.OURO_EINVAL
        assert call(raw_bytes=buf.size - 1, entry=entry) == _native.OURO_EINVAL
    assert call() == _native.OURO_OK and call(tip_=None) == _native.OURO_OK
    # an empty batch: cfg and tip are checked all the same, and the tip passes through
    good = _native.ChainTip(proto=1, slot=9, block_no=4)
    for entry in ("ouro_chain_envelope_cbor_host", "ouro_chain_envelope_cbor"):
        fn = getattr(lib, entry)
        out = _native.ChainTip()
        empty = lambda t, c=cfg: fn(ptr(buf), buf.size, ptr(off), ptr(ln), 0,  # noqa: E731
                                    ctypes.byref(c) if c is not None else None, ctypes.byref(t),
                                    ptr(st), ptr(hh), ptr(bits), ctypes.byref(out))
        assert empty(_native.ChainTip(origin=1, slot=1)) == _native.OURO_EINVAL
        assert empty(_native.ChainTip(proto=2)) == _native.OURO_EINVAL
        assert empty(good, None) == _native.OURO_EINVAL
        assert empty(good) == _native.OURO_OK
        assert bytes(out) == bytes(good)
    # no PBFT header in the batch: a zero epoch length is fine
    t, _ = EC.tpraos(EC.GENESIS, 0, 0)
    assert list(host([t], cfg=E.Cfg(0))[2]) == [ALL]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "env.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ouro_verify.h"',
             'int main(void){',
             'printf("%zu %zu\\n", sizeof(ouro_chain_tip), sizeof(ouro_envelope_cfg));']
    for cls, c in ((_native.ChainTip, "ouro_chain_tip"), (_native.EnvelopeCfg, "ouro_envelope_cfg")):
        for name, _ in cls._fields_:
            lines.append(f'printf("%zu\\n", offsetof({c}, {name}));')
    src.write_text("\n".join(lines + ["return 0;}", ""]))
    exe = tmp_path / "env"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [ctypes.sizeof(_native.ChainTip),
                                          ctypes.sizeof(_native.EnvelopeCfg)] == [56, 40]
    want = [getattr(cls, name).offset for cls in (_native.ChainTip, _native.EnvelopeCfg)
            for name, _ in cls._fields_]
    assert [int(x) for x in out[2:]] == want
    assert want == [0, 1, 2, 3, 8, 16, 24, 0, 8, 16, 24, 32]
    assert (_native.ENV_BLOCKNO_OK, _native.ENV_SLOT_OK, _native.ENV_PREVHASH_OK,
            _native.ENV_EXTRA_OK, _native.ENV_ALL_OK) == (BN, SL, PH, EX, ALL) == (1, 2, 4, 8, 15)
