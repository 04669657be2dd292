"""The header envelope on the device (ouro_chain_envelope_cbor and _device:
k_envelope_slice, k_header_hash, k_envelope_link) against envelope.py and
hashlib: the reference's fixtures, header lengths through every residue of the
hashed length mod 128 at every start alignment, linked chains with broken
links across eras, chaining through the tip, the device-pointer form and the
recompute after a device error."""
import ctypes
import hashlib

import numpy as np
import pytest

import envelope_cases as EC
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as B
from ouroboros_network_amd import envelope as E
from ouroboros_network_amd import header as H

pytestmark = pytest.mark.gpu
ALL = E.ENV_ALL_OK
CFG = E.Cfg(EC.EPOCH_SLOTS)


def check(raws, triple=None, tip=E.ORIGIN, cfg=CFG, want=None):
    """the device entry on `raws` (or on their (buf, off, len) triple) =
    envelope.py; returns the bits"""
    st, hh, bits, tip_out = H.chain_envelope_cbor(triple if triple is not None else raws, cfg, tip)
    usable, hashes, wbits, wtip = want or EC.expect(raws, tip, cfg)
    assert [bytes(h) for h in hh] == hashes
    assert list(bits) == wbits
    assert tip_out == wtip
    # the slicer's status: exactly the Python slicers' (a Byron header's code,
    # a TPraos header's acceptance), and for a rejected TPraos header the code
    # the pinned host slicer gives (tests/test_pack.py pins it to header.py)
    EC.assert_status(st, raws)
    tp = [i for i, r in enumerate(raws) if H.era_class(r) == H.PROTO_TPRAOS]
    if tp:
        z = np.zeros((len(tp), 32), np.uint8)
        host = H.pack_cbor([raws[i] for i in tp], slots_per_kes_period=100, eta_alpha=z,
                           leader_alpha=z).status
        assert st[tp].tolist() == host.tolist()
    return list(bits)


@pytest.fixture(scope="module")
def residues():
    """1,024 headers per era, each a valid link to the one before: the hashed
    length (header item + prefix) steps through every residue mod 128, and
    the cycling gaps put every length at every start alignment"""
    raws, h = [], None
    e0, h = EC.byron_ebb(bytes(32), 0, 0)
    raws.append(e0)
    for i in range(1, 1024):
        raw, h = EC.byron_regular(h, 0, i, i, extra_len=i % 331, form=1 + i % 3)
        raws.append(raw)
    for i in range(1024):
        raw, h = EC.tpraos(h, 30000 + i, 1024 + i, era=(None if i % 3 else 3),
                           body_hash_len=i % 200)
        raws.append(raw)
    want = EC.expect(raws)
    assert want[2] == [ALL] * 2048
    for era, part in ((0, raws[:1024]), (1, raws[1024:])):
        npre = 2 if era == 0 else 0
        lens = {(len(E._byron_item(r)[1]) if era == 0 else E.header_record(r).header_size) + npre
                for r in part}
        assert {x % 128 for x in lens} == set(range(128))
    return raws, want


def test_fixtures_hash_to_the_golden_values(gpu_lib):
    fx = EC.fixtures()
    reg, ebb = bytes.fromhex(fx["byron_regular_header"]), bytes.fromhex(fx["byron_ebb_header"])
    golden = H.bytes_at(bytes.fromhex(fx["header_hash_byron"]), 0)
    raws = []
    for form in (1, 2, 3):
        raws += [EC.byron_wire(0, ebb, form), EC.byron_wire(1, reg, form)]
    raws += [bytes.fromhex(h["raw"]) for h in EC.kats()["headers"]]
    st, hh, bits, _ = H.chain_envelope_cbor(raws, CFG)
    for k in (1, 3, 5):
        assert bytes(hh[k]) == golden
        assert bytes(hh[k - 1]) == hashlib.blake2b(b"\x82\x00" + ebb, digest_size=32).digest()
    assert list(bits[:2]) == [ALL, ALL]
    check(raws)


def test_every_length_residue_at_every_alignment(gpu_lib, residues):
    raws, want = residues
    recs = [E.header_record(r, CFG) for r in raws]
    hashed = [(len(E._byron_item(r)[1]) + 2) if x.proto == H.PROTO_PBFT else x.header_size
              for r, x in zip(raws, recs)]
    pairs = {0: set(), 1: set()}
    for shift in range(4):
        buf, off, ln = EC.spaced(raws, shift=shift)
        # the upload is the window from the first header, allocation-aligned:
        # a header's address on the device mod 4 is its distance from it mod 4
        for x, h, o in zip(recs, hashed, off):
            pairs[x.proto].add((h % 128, int(o - off[0]) % 4))
        check(raws, (buf, off, ln), want=want)
    # every (hashed length mod 128, start address mod 4) pair occurred, per era
    full = {(r, a) for r in range(128) for a in range(4)}
    assert pairs[0] == full and pairs[1] == full
    check(raws, want=want)


def tag24_payload(raw):
    """the bytes inside a TPraos wire header's #6.24 byte string"""
    i = 0
    mt, _, j = H._head(raw, 0)
    if mt == 4:  # [era, wrapped]
        i = H.skip(raw, j)
    _, _, j = H._head(raw, i)
    _, ln, k = H._head(raw, j)
    return raw[k:k + ln]


def run_device(gpu_lib, buf, off, ln, raw_bytes=None, shift=0, work_less=0):
    """ouro_chain_envelope_cbor_device over (buf, off, len) copied to the
    device: (rc, status, hashes, bits, tip_out)"""
    import torch

    n = int(off.size)
    dev = torch.device("cuda", 0)
    pad = (-buf.size) % 4
    d_raw = torch.tensor(np.concatenate([buf, np.zeros(pad + 4, np.uint8)]), device=dev)
    d_off = torch.tensor(off.astype(np.int64), device=dev)
    d_len = torch.tensor(ln.astype(np.int32), device=dev)
    wb = gpu_lib.ouro_chain_envelope_work_bytes(n)
    assert wb >= 128 * n
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    hh = torch.full((n, 32), 5, dtype=torch.uint8, device=dev)
    bits = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    tip = torch.full((56,), 3, dtype=torch.uint8, device=dev)
    cfg, t_in = H._c_cfg(CFG), H._c_tip(E.ORIGIN)
    stream = torch.cuda.current_stream()
    rc = gpu_lib.ouro_chain_envelope_cbor_device(
        ctypes.c_void_p(stream.cuda_stream), d_raw.data_ptr() + shift,
        buf.size if raw_bytes is None else raw_bytes, d_off.data_ptr(), d_len.data_ptr(), n,
        ctypes.byref(cfg), ctypes.byref(t_in), work.data_ptr(), wb - work_less, status.data_ptr(),
        hh.data_ptr(), bits.data_ptr(), tip.data_ptr())
    torch.cuda.synchronize()
    t = _native.ChainTip.from_buffer_copy(tip.cpu().numpy().tobytes())
    return (rc, status.cpu().numpy(), [bytes(h) for h in hh.cpu().numpy()],
            list(bits.cpu().numpy()), t)


def test_device_resident_form_on_the_fixtures(gpu_lib):
    """the golden Byron regular and EBB headers in their three wire forms and
    the golden Shelley-family headers through the device-pointer entry"""
    fx = EC.fixtures()
    reg, ebb = bytes.fromhex(fx["byron_regular_header"]), bytes.fromhex(fx["byron_ebb_header"])
    golden = H.bytes_at(bytes.fromhex(fx["header_hash_byron"]), 0)
    ebb_hash = hashlib.blake2b(b"\x82\x00" + ebb, digest_size=32).digest()
    raws = []
    for form in (1, 2, 3):
        raws += [EC.byron_wire(0, ebb, form), EC.byron_wire(1, reg, form)]
    shelley = [bytes.fromhex(h["raw"]) for h in EC.kats()["headers"]]
    raws += shelley
    want = EC.expect(raws)
    for shift in range(4):
        buf, off, ln = EC.spaced(raws, shift=shift)
        rc, st, hh, bits, tip = run_device(gpu_lib, buf, off, ln)
        _native.check(rc, "ouro_chain_envelope_cbor_device")
        assert hh[0::2][:3] == [ebb_hash] * 3 and hh[1::2][:3] == [golden] * 3
        assert hh[6:] == [hashlib.blake2b(tag24_payload(r), digest_size=32).digest()
                          for r in shelley]
        assert hh == want[1] and bits == want[2] and H._py_tip(tip) == want[3]
        assert bits[:2] == [ALL, ALL]
        assert st.tolist() == [B.PACK_EBB, B.PACK_OK] * 3 + [H.PACK_OK] * len(shelley)


def test_device_resident_form(gpu_lib, residues, broken):
    raws, _ = residues
    raws = raws[700:1400]
    want = EC.expect(raws)
    buf, off, ln = EC.spaced(raws)
    rc, st, hh, bits, tip = run_device(gpu_lib, buf, off, ln)
    _native.check(rc, "ouro_chain_envelope_cbor_device")
    assert hh == want[1] and bits == want[2] and H._py_tip(tip) == want[3]
    EC.assert_status(st, raws)
    # rejected headers of both eras, and spans that leave the buffer: the
    # device form reports those per header, as OURO_PACK_ESPAN
    braws, bwant = broken
    buf, off, ln = EC.spaced(braws)
    cut = int(off[990])  # raw_bytes ends before header 990: it and its successors are outside
    rc, st, hh, bits, tip = run_device(gpu_lib, buf, off, ln, raw_bytes=cut)
    _native.check(rc, "ouro_chain_envelope_cbor_device")
    EC.assert_status(st[:990], braws[:990])
    assert hh[:990] == bwant[1][:990] and bits[:990] == bwant[2][:990]
    assert st[990:].tolist() == [5] * 10 and bits[990:] == [0] * 10      # OURO_PACK_ESPAN
    assert hh[990:] == [bytes(32)] * 10 and not H._py_tip(tip).usable
    # refused before anything is enqueued
    buf, off, ln = EC.spaced(raws[:8])
    assert run_device(gpu_lib, buf, off, ln, shift=1)[0] == _native.OURO_EINVAL
    assert run_device(gpu_lib, buf, off, ln, work_less=1)[0] == _native.OURO_EINVAL


@pytest.fixture(scope="module")
def broken():
    """1,000 headers: Byron with EBBs, the era switch, TPraos; and in it a wrong
    previous hash, an equal slot, a block number off by one, GenesisHash in the
    middle, a malformed previous hash, truncated headers of both eras, and an
    EBB of another shape"""
    raws = EC.good_chain(400, 600, ebb_every=13, extra_step=7)
    bad = {}

    def redo(i, **kw):
        r = E.header_record(raws[i], CFG)
        p = E.header_record(raws[i - 1], CFG)
        a = dict(prev=p.hash, slot=r.slot, block_no=r.block_no)
        a.update(kw)
        if r.proto == H.PROTO_PBFT:
            raws[i], _ = EC.byron_regular(a["prev"], a["slot"] // EC.EPOCH_SLOTS,
                                          a["slot"] % EC.EPOCH_SLOTS, a["block_no"])
        else:
            raws[i], _ = EC.tpraos(a["prev"], a["slot"], a["block_no"])
        bad[i] = True

    redo(100, prev=bytes(32))
    redo(255, block_no=7)
    redo(256, prev=b"\x11" * 32)
    redo(600, slot=E.header_record(raws[599], CFG).slot)
    redo(601, block_no=E.header_record(raws[601], CFG).block_no + 1)
    redo(511, prev=b"\x33" * 32)
    redo(512, slot=E.header_record(raws[511], CFG).slot - 1)
    redo(700, prev=EC.GENESIS)
    redo(701, prev=b"\x41\x00")
    raws[50] = raws[50][:-2]
    raws[800] = raws[800][:-2]
    raws[999] = raws[999][:40]
    raws[300], _ = EC.byron_ebb(b"\x22" * 32, 3, 3, consensus=EC.arr(EC.C.cbor_uint(3)))
    want = EC.expect(raws)
    n_bad = sum(1 for b in want[2] if b != ALL)
    assert 15 <= n_bad <= 34
    return raws, want


def test_broken_links_across_eras(gpu_lib, broken):
    raws, want = broken
    bits = check(raws, want=want)
    assert bits[100] == ALL & ~E.ENV_PREVHASH_OK and bits[50] == 0 and bits[51] == E.ENV_EXTRA_OK
    assert bits[600] == ALL & ~E.ENV_SLOT_OK and bits[700] == ALL & ~E.ENV_PREVHASH_OK
    assert E.first_invalid(bits) == 50


def test_a_strict_alternation_of_eras(gpu_lib):
    """Byron and TPraos headers one by one: the neighbour of a header is its
    neighbour in the stream, whatever its era"""
    raws, h, slot = [], bytes(32), 0
    for i in range(300):
        slot += 1 + i % 3
        if i % 2:
            raw, h2 = EC.tpraos(h if i % 7 else b"\x55" * 32, slot, i)
        else:
            raw, h2 = EC.byron_regular(h, slot // EC.EPOCH_SLOTS, slot % EC.EPOCH_SLOTS,
                                       i if i % 11 else i + 1, form=1 + i % 3)
        raws.append(raw)
        h = h2
    bits = check(raws)
    assert bits.count(ALL) > 200 and bits.count(ALL) < 290


def test_chaining_through_the_tip(gpu_lib, broken):
    raws, want = broken
    for cut in (0, 1, 50, 51, 300, 301, 400, 999, 1000):
        _, hh1, b1, tip = H.chain_envelope_cbor(raws[:cut], CFG)
        _, hh2, b2, tip2 = H.chain_envelope_cbor(raws[cut:], CFG, tip)
        assert list(b1) + list(b2) == want[2], cut
        assert tip2 == want[3]


def test_the_limits_on_the_device(gpu_lib, residues):
    raws, _ = residues
    part = raws[1000:1100]
    sizes = sorted(E.header_record(r).header_size for r in part[24:])
    cfg = E.Cfg(EC.EPOCH_SLOTS, (sizes[len(sizes) // 2], 2**32, 2**32))
    bits = check(part, cfg=cfg)
    assert 20 < sum(1 for b in bits if not b & E.ENV_EXTRA_OK) < 60


@pytest.mark.device_error
def test_device_error_recomputes_on_the_host_path(gpu_lib, broken):
    """OURO_TEST_DEVICE_ERROR (the test build's hook): the launches report an
    error and the entry answers from the host path"""
    raws, want = broken
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1"):
        check(raws, want=want)
        msg = gpu_lib.ouro_last_error().decode()
        assert "recomputed on the host path" in msg, msg


# ---- the combined entry: ouro_chain_validate_cbor ---------------------------------
def sched_for(raws):
    """a three-entry epoch schedule whose boundaries fall inside the stream's
    TPraos part"""
    from ouroboros_network_amd.tpraos import EpochNonces

    slots = [r.slot for r in (E.header_record(x, CFG) for x in raws)
             if r is not None and r.proto == H.PROTO_TPRAOS]
    cut = sorted(slots)
    first = [0, cut[len(cut) // 3], cut[2 * len(cut) // 3]]
    return EpochNonces(first_slot=first, nonce=[b"\x07" * 32, bytes(32), b"\x09" * 32],
                       neutral=[0, 1, 0])


def assert_same_crypto(raws, got, sched):
    """the combined entry's crypto outputs = the existing entry's, byte for byte"""
    ref = H.verify_chain_cbor(raws, 100, -1, epochs=sched, nonce=True)
    for x, y in zip(ref, got):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("slots", [1, 3, 6])
def test_validate_in_small_chunks(gpu_lib, small_chunks, broken, slots):
    """chunks of 256 headers: the broken links at 255 | 256 and 511 | 512 sit on
    a chunk's last and first header, chunk [256, 512) is mixed (the era switch
    at 400, an unusable EBB at 300), and every chunk's first header is linked
    on the host to the chunk before it"""
    raws, want = broken
    sched = sched_for(raws)
    ref = H.verify_chain_cbor(raws, 100, -1, epochs=sched, nonce=True)  # (default chunks)
    small_chunks(CHUNK=256, SLOTS=slots)
    crypto, hh, bits, tip, accepted = H.validate_chain_cbor(raws, 100, -1, cfg=CFG, epochs=sched,
                                                            nonce=True)
    assert [bytes(h) for h in hh] == want[1]
    assert list(bits) == want[2]
    assert tip == want[3]
    for x, y in zip(ref, crypto):
        assert x.tobytes() == y.tobytes()
    assert_same_crypto(raws, crypto, sched)
    for i in (255, 256, 511, 512, 300, 301):
        assert bits[i] != ALL
    assert bits[258] == ALL and bits[514] == ALL and bits[400] == ALL


def test_validate_a_strict_alternation_in_mixed_chunks(gpu_lib, small_chunks):
    raws, h, slot = [], bytes(32), 0
    for i in range(600):
        slot += 1 + i % 3
        if i % 2:
            raw, h = EC.tpraos(h if i % 7 else b"\x55" * 32, slot, i)
        else:
            raw, h = EC.byron_regular(h, slot // EC.EPOCH_SLOTS, slot % EC.EPOCH_SLOTS,
                                      i if i % 11 else i + 1, form=1 + i % 3, extra_len=i % 97)
        raws.append(raw)
    want = EC.expect(raws)
    small_chunks(CHUNK=256, SLOTS=3)
    crypto, hh, bits, tip, _ = H.validate_chain_cbor(raws, 100, -1, cfg=CFG, nonce=True)
    assert [bytes(x) for x in hh] == want[1]
    assert list(bits) == want[2] and tip == want[3]
    assert_same_crypto(raws, crypto, None)
    assert 350 < list(bits).count(ALL) < 590


def test_validate_against_the_oracle_on_a_signed_linked_chain(gpu_lib, small_chunks):
    import chain_cases as CC
    from test_chain_validate import assert_validate

    raws, ea, la, want_crypto, want_env = EC.validate_stream()
    got = H.validate_chain_cbor(raws, CC.SPKP, -1, cfg=EC.VAL_CFG, epochs=CC.sched3(), nonce=True)
    assert_validate(got, raws, want_crypto, want_env)
    tip = E.validate_envelope(raws[:30], E.ORIGIN, EC.VAL_CFG)[3]
    got = H.validate_chain_cbor(raws[30:], CC.SPKP, -1, cfg=EC.VAL_CFG, tip=tip,
                                epochs=CC.sched3(), nonce=True)
    assert got[4] == 5 and list(got[2]) == want_env[2][30:]


@pytest.mark.device_error
def test_validate_device_error_recomputes_on_the_host_path(gpu_lib, small_chunks, broken):
    raws, want = broken
    sched = sched_for(raws)
    ref = H.verify_chain_cbor(raws, 100, -1, epochs=sched, nonce=True, host=True)
    with _native.knob_env(OURO_TEST_DEVICE_ERROR="1", OURO_CBOR_CHUNK="256"):
        crypto, hh, bits, tip, _ = H.validate_chain_cbor(raws, 100, -1, cfg=CFG, epochs=sched,
                                                         nonce=True)
        msg = gpu_lib.ouro_last_error().decode()
        assert "recomputed on the host path" in msg, msg
    assert [bytes(h) for h in hh] == want[1] and list(bits) == want[2] and tip == want[3]
    for x, y in zip(ref, crypto):
        assert x.tobytes() == y.tobytes()
