"""The era classifier and the combined raw entry on the host path (CPU-only):
header.era_class / csrc/cbor.h era_class, and ouro_chain_verify_cbor_host --
Byron and Shelley-family raw headers, over several epochs, in one call.

Expected values (chain_cases.py): TPraos rows from the pinned host slicer +
the oracle with explicit per-row alphas, PBFT rows from byron.byron_status +
the oracle's donna-style verify.  tests/test_gpu_chain_cbor.py runs the same
streams through the device pipeline.
"""
import ctypes
import functools

import numpy as np
import pytest

import chain_cases as K
from ouroboros_network_amd import _native
from ouroboros_network_amd import byron as B
from ouroboros_network_amd import header as H

MAGIC = -1  # each Byron header's own protocol magic (byron.HEADER_MAGIC)


@functools.lru_cache(maxsize=None)
def classifier_inputs():
    """the 16 reference fixtures, each with bit flips 0x01 / 0x04 / 0x20 / 0x80
    at every byte and truncated to 0, 1, 2, 3, 5, 9, 50 and len - 1 bytes"""
    kats = K.load_kats()
    fixtures = [bytes.fromhex(h["raw"]) for h in kats["headers"]] + \
        [bytes.fromhex(w["raw"]) for w in kats["byron_wire"]] + [bytes.fromhex(kats["byron"]["raw"])]
    assert len(fixtures) == 16
    out = []
    for g in fixtures:
        out.append(g)
        for pos in range(len(g)):
            for bit in (0x01, 0x04, 0x20, 0x80):
                m = bytearray(g)
                m[pos] ^= bit
                out.append(bytes(m))
        out += [g[:k] for k in (0, 1, 2, 3, 5, 9, 50, len(g) - 1)]
    return out, np.array([H.era_class(r) for r in out], np.uint8)


def test_era_class_never_turns_a_header_away_from_its_slicer():
    """no input classed PBFT parses as a Shelley header; no input classed
    TPraos has Byron status OK or EBB"""
    raws, cls = classifier_inputs()
    assert len(raws) > 44000
    def parses(r):  # (the Python slicer rejects with CBORError or an IndexError)
        try:
            H.parse_header(r)
            return True
        except Exception:
            return False

    shelley = byron = 0
    for r, c in zip(raws, cls):
        is_byron = B.byron_status(r)[0] in (B.PACK_OK, B.PACK_EBB)
        is_shelley = parses(r)
        assert not (c == H.PROTO_PBFT and is_shelley)
        assert not (c == H.PROTO_TPRAOS and is_byron)
        byron += is_byron
        shelley += is_shelley
    assert shelley > 20000 and byron > 10000  # both slicers accept plenty of them


def test_c_classifier_equals_the_python_one():
    """csrc/cbor.h era_class, read through `proto` of the host entry"""
    raws, cls = classifier_inputs()
    z = np.zeros((len(raws), 32), np.uint8)
    proto, status, verdict, *_ = H.verify_chain_cbor(raws, K.SPKP, MAGIC, eta_alpha=z,
                                                     leader_alpha=z, host=True)
    np.testing.assert_array_equal(proto, cls)
    # a header goes to exactly one slicer: the other era's statuses never appear
    assert not np.isin(status, (H.PACK_EBYRON, B.PACK_ESHELLEY)).any()
    assert (status[proto == H.PROTO_PBFT] != H.PACK_OK).any()
    assert (verdict[status == B.PACK_EBB] == 1).all()


def _order(n, interleaved):
    if not interleaved:
        return np.arange(n)
    # one by one: Byron, Shelley, Byron, ... (8 + 7 fixtures)
    out = []
    for i in range(8):
        out.append(i)
        if i < 7:
            out.append(8 + i)
    return np.array(out)


@pytest.mark.parametrize("interleaved", [False, True], ids=["byron_then_shelley", "one_by_one"])
def test_reference_fixtures_in_one_call(interleaved):
    raws, ea, la, kinds, want = K.fixtures15()
    o = _order(len(raws), interleaved)
    got = H.verify_chain_cbor([raws[i] for i in o], K.SPKP, MAGIC, eta_alpha=ea[o],
                              leader_alpha=la[o], nonce=True, host=True)
    K.assert_chain_equal(got, tuple(w[o] for w in want))
    proto, status, verdict, be, bl, en = got
    assert list(proto) == [([0] * 8 + [1] * 7)[i] for i in o]
    for row, i in enumerate(o):
        if i >= 8:
            assert verdict[row] == K.STRICT and status[row] == H.PACK_OK
            assert be[row].any() and bl[row].any() and en[row].any()
        else:
            assert verdict[row] == 1
            assert status[row] == (B.PACK_EBB if kinds[i] == "boundary" else B.PACK_OK)
            assert not be[row].any() and not bl[row].any() and not en[row].any()
    assert sum(k == "regular" for k in kinds) == 5 and sum(k == "boundary" for k in kinds) == 3


def test_every_single_byte_corruption_mixed():
    """a regular Byron fixture and a Shelley fixture, each with every
    single-byte ^0x04 corruption, interleaved into one call"""
    raws, ea, la, want = K.corruptions()
    assert 1500 < len(raws) < 1700
    got = H.verify_chain_cbor(raws, K.SPKP, MAGIC, eta_alpha=ea, leader_alpha=la, nonce=True,
                              host=True)
    K.assert_chain_equal(got, want)
    proto, _status, verdict = got[:3]
    for cls in (H.PROTO_PBFT, H.PROTO_TPRAOS):
        rows = proto == cls
        valid = (verdict[rows] == 1) if cls == H.PROTO_PBFT else ((verdict[rows] & 0x0F) == 0x0F)
        assert 0 < valid.sum() < rows.sum()


def test_three_epochs_with_byron_spliced_in():
    raws, want = K.three_epoch_stream()
    got = H.verify_chain_cbor(raws, K.SPKP, MAGIC, epochs=K.sched3(), nonce=True, host=True)
    K.assert_chain_equal(got, want)
    proto, _status, verdict, _be, _bl, en = got
    assert list(proto[:3]) == [0, 0, 0] and list(proto[-2:]) == [0, 0]
    assert (verdict[proto == H.PROTO_TPRAOS] == K.STRICT).all()
    assert (verdict[proto == H.PROTO_PBFT] == 1).all()
    # eta_nonce = Blake2b-256 of the claimed eta output on the TPraos rows
    import hashlib

    for r, e, p in zip(raws, en, proto):
        if p == H.PROTO_TPRAOS:
            h = H.parse_header(r)
            assert e.tobytes() == hashlib.blake2b(h.eta_output, digest_size=32).digest()
    # no schedule = NeutralNonce everywhere: only the neutral epoch's rows verify
    got0 = H.verify_chain_cbor(raws, K.SPKP, MAGIC, host=True)
    t = proto == H.PROTO_TPRAOS
    assert 0 < ((got0[2][t] & 0x0C) == 0x0C).sum() < t.sum()


def _call(fn, raws, *, spkp=K.SPKP, magic=MAGIC, epochs=None, ea=None, la=None, proto=True,
          span_bug=False, devices=None):
    buf, off, ln = H.raw_triplet(raws)
    n = len(raws)
    if span_bug:
        off = off.copy()
        off[n - 1] = buf.size  # a span past the buffer
    outs = [np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8),
            np.full((n, 64), 0xEE, np.uint8), np.full((n, 64), 0xEE, np.uint8),
            np.full((n, 32), 0xEE, np.uint8)]
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    e = None if epochs is None else ctypes.byref(epochs.c_struct())
    args = (ptr(buf), buf.size, ptr(off), ptr(ln), n, spkp, magic, e, ptr(ea), ptr(la),
            ptr(outs[0]) if proto else None, *[ptr(a) for a in outs[1:]])
    if devices is not None:
        d = np.array(devices, np.int32)
        rc = fn(ptr(d), d.size, *args)
    else:
        rc = fn(*args)
    return rc, all((a == 0xEE).all() for a in outs)


@pytest.mark.parametrize("entry", ["ouro_chain_verify_cbor_host", "ouro_chain_verify_cbor",
                                   "ouro_chain_verify_cbor_multi"])
def test_argument_errors(entry):
    """every argument check runs before any work (and before a device is
    looked for): OURO_EINVAL, outputs untouched"""
    lib = _native.load()
    fn = getattr(lib, entry)
    dev = [0] if entry.endswith("_multi") else None
    raws, ea, la, _kinds, _want = K.fixtures15()
    bad = [
        (dict(epochs=K.sched3(), ea=ea, la=la), "not both"),
        (dict(ea=ea), "both VRF input arrays"),
        (dict(la=la), "both VRF input arrays"),
        (dict(proto=False), "proto"),
        (dict(span_bug=True), "span outside raw_bytes"),
        (dict(spkp=0), "zero slots per KES period"),
        (dict(magic=-2), "protocol magic"),
        (dict(magic=1 << 32), "protocol magic"),
    ]
    for kw, why in bad:
        rc, untouched = _call(fn, raws, devices=dev, **kw)
        assert rc == _native.OURO_EINVAL and untouched, kw
        assert why in lib.ouro_last_error().decode(), kw
    assert _call(fn, [], devices=dev)[0] == _native.OURO_OK  # n = 0


def test_no_device_is_an_error_not_an_accept():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _native.load()
    raws, ea, la, _kinds, _want = K.fixtures15()
    rc, untouched = _call(lib.ouro_chain_verify_cbor, raws, ea=ea, la=la)
    assert rc == _native.OURO_ENODEV and untouched
