"""The span check of every host-buffer entry that takes (raw, raw_bytes, off,
len, n), without a device (CPU suite).  Each entry rejects a span that ends
past the buffer, and an offset near 2^64 that a wrapping comparison would let
through, with OURO_EINVAL and the text "<item> <i>: span outside <bound>",
before it writes any output; and each accepts n = 0.  One table of entries,
one test body: what differs per entry is its argument list alone.
"""
import ctypes

import numpy as np
import pytest

import block_cases as BC
import ledger_cases as LC

EINVAL = -3
FILL = 0xEE


@pytest.fixture(scope="module")
def lib():
    from ouroboros_network_amd import _native

    return _native.load()


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _layout(raws):
    buf = np.frombuffer(b"".join(raws), np.uint8)
    ln = np.array([len(r) for r in raws], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    return buf, off, ln


@pytest.fixture(scope="module")
def headers(kats):
    return _layout([bytes.fromhex(h["raw"]) for h in kats["headers"][:4]])


@pytest.fixture(scope="module")
def blocks():
    return _layout([bytes.fromhex(b["raw"]) for b in BC.golden()[:3]])


class Outs:
    """Output arrays filled with FILL; untouched() after the call."""

    def __init__(self):
        self.arrays = []

    def __call__(self, count, dtype=np.uint8):
        a = np.full(max(count, 1) * np.dtype(dtype).itemsize, FILL, np.uint8)  # every byte FILL
        self.arrays.append(a)
        return a.view(dtype)

    def untouched(self):
        return all((a == FILL).all() for a in self.arrays)


def _devs():
    return np.array([0, 0], np.int32)


def _env_args():
    from ouroboros_network_amd import _native

    return ctypes.byref(_native.EnvelopeCfg(21600, 0, 0, 0, 0)), None


def _ledger_args():
    views, _ = LC.views_k(2)
    keep = (views, views.c_struct(), LC.G_CHAIN.c_struct())
    return keep, ctypes.byref(keep[1]), ctypes.byref(keep[2])


# per entry: call(lib, o, buf, nbytes, off, ln, n) -> rc, every output from o
def _tpraos(lib, o, b, nb, off, ln, n):
    return lib.ouro_tpraos_verify_cbor(P(b), nb, P(off), P(ln), n, 100, None, None, None, P(o(n)),
                                       P(o(n)), P(o(64 * n)), P(o(64 * n)), P(o(32 * n)))


def _integrity(lib, o, b, nb, off, ln, n):
    return lib.ouro_integrity_verify_cbor(P(b), nb, P(off), P(ln), n, 100, P(o(n)), P(o(n)))


def _byron(lib, o, b, nb, off, ln, n):
    return lib.ouro_byron_verify_cbor(P(b), nb, P(off), P(ln), n, -1, P(o(n)), P(o(n)))


def _chain_outs(o, n):
    return [P(o(n)), P(o(n)), P(o(n)), P(o(64 * n)), P(o(64 * n)), P(o(32 * n))]


def _chain(name):
    def call(lib, o, b, nb, off, ln, n):
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, 100, -1, None, None, None,
                                  *_chain_outs(o, n))
    return call


def _validate(name):
    def call(lib, o, b, nb, off, ln, n):
        cfg, tip = _env_args()
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, 100, -1, None, None, None, cfg, tip,
                                  *_chain_outs(o, n), P(o(32 * n)), P(o(n)), None)
    return call


def _validate_ledger(name):
    def call(lib, o, b, nb, off, ln, n):
        cfg, tip = _env_args()
        keep, views, g = _ledger_args()
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, LC.SPKP, -1, None, None, None, cfg,
                                  tip, *_chain_outs(o, n), P(o(32 * n)), P(o(n)), None, views, g,
                                  None, None, None, P(o(n)), P(o(n, np.uint32)))
    return call


def _envelope(name):
    def call(lib, o, b, nb, off, ln, n):
        cfg, tip = _env_args()
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, cfg, tip, P(o(n)), P(o(32 * n)),
                                  P(o(n)), None)
    return call


def _block_integrity(name):
    def call(lib, o, b, nb, off, ln, n):
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, BC.SPKP, P(o(n)), P(o(n)),
                                  P(o(32 * n)))
    return call


def _witness_count(name):
    def call(lib, o, b, nb, off, ln, n):
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, P(o(n)), P(o(n, np.uint32)),
                                  P(o(n, np.uint32)))
    return call


def _witness_verify(name):
    def call(lib, o, b, nb, off, ln, n):
        from ouroboros_network_amd.witness import WitnessOutC

        # (n = 0 writes the two begins' first entry: they are not outputs of `o`)
        begins = [np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)] if n == 0 else \
            [o(n + 1, np.uint64), o(n + 1, np.uint64)]
        out = WitnessOutC(8, 8, begins[0].ctypes.data, begins[1].ctypes.data, o(32 * 8).ctypes.data,
                          o(8, np.uint32).ctypes.data, o(8).ctypes.data, o(8).ctypes.data,
                          o(32 * 8).ctypes.data)
        return getattr(lib, name)(P(b), nb, P(off), P(ln), n, ctypes.byref(out), P(o(n)), P(o(n)),
                                  P(o(n, np.uint32)))
    return call


def _blake2b(name):
    def call(lib, o, b, nb, off, ln, n):
        return getattr(lib, name)(n, P(b), nb, P(off), P(ln), P(o(32 * n)))
    return call


def _tpraos_multi(lib, o, b, nb, off, ln, n):
    return lib.ouro_tpraos_verify_cbor_multi(P(_devs()), 2, P(b), nb, P(off), P(ln), n, 100, None,
                                             None, None, P(o(n)), P(o(n)), P(o(64 * n)),
                                             P(o(64 * n)), P(o(32 * n)))


def _integrity_multi(lib, o, b, nb, off, ln, n):
    return lib.ouro_integrity_verify_cbor_multi(P(_devs()), 2, P(b), nb, P(off), P(ln), n, 100,
                                                P(o(n)), P(o(n)))


def _byron_multi(lib, o, b, nb, off, ln, n):
    return lib.ouro_byron_verify_cbor_multi(P(_devs()), 2, P(b), nb, P(off), P(ln), n, -1,
                                            P(o(n)), P(o(n)))


def _chain_multi(lib, o, b, nb, off, ln, n):
    return lib.ouro_chain_verify_cbor_multi(P(_devs()), 2, P(b), nb, P(off), P(ln), n, 100, -1,
                                            None, None, None, *_chain_outs(o, n))


def _pair(name, make):
    return [(name, make(name)), (name + "_host", make(name + "_host"))]


# (entry, its call, the fixture it reads, the item word, the bound's name)
HDR, BLK, MSG = ("headers", "header", "raw_bytes"), ("blocks", "block", "raw_bytes"), \
    ("headers", "message", "msg_bytes")
ENTRIES = [(n, c) + HDR for n, c in [
    ("ouro_tpraos_verify_cbor", _tpraos), ("ouro_integrity_verify_cbor", _integrity),
    ("ouro_byron_verify_cbor", _byron)] + _pair("ouro_chain_verify_cbor", _chain) +
    _pair("ouro_chain_validate_cbor", _validate) +
    _pair("ouro_chain_validate_ledger_cbor", _validate_ledger) +
    _pair("ouro_chain_envelope_cbor", _envelope) + [
    ("ouro_tpraos_verify_cbor_multi", _tpraos_multi),
    ("ouro_integrity_verify_cbor_multi", _integrity_multi),
    ("ouro_byron_verify_cbor_multi", _byron_multi),
    ("ouro_chain_verify_cbor_multi", _chain_multi)]]
# (whole blocks go through the raw-CBOR pipeline, whose item is a header)
ENTRIES += [(n, c) + ("blocks", "header", "raw_bytes")
            for n, c in _pair("ouro_block_integrity_verify_cbor", _block_integrity)]
ENTRIES += [(n, c) + BLK for n, c in _pair("ouro_block_witness_count_cbor", _witness_count) +
            _pair("ouro_block_witness_verify_cbor", _witness_verify)]
ENTRIES += [(n, c) + MSG for n, c in _pair("ouro_blake2b256_batch", _blake2b)]


@pytest.mark.parametrize("name,call,fixture,item,bound", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_span_outside_the_buffer(lib, request, name, call, fixture, item, bound):
    buf, off, ln = request.getfixturevalue(fixture)
    n = off.size
    past = off.copy()
    past[2] = buf.size - 3  # ends past the buffer (every fixture is longer than 3 bytes)
    wrap = off.copy()
    wrap[1] = 2**64 - 8  # off + len wraps to a small number
    for bad, i in ((past, 2), (wrap, 1)):
        o = Outs()
        assert call(lib, o, buf, buf.size, bad, ln, n) == EINVAL, lib.ouro_last_error()
        assert lib.ouro_last_error() == f"{item} {i}: span outside {bound}".encode()
        assert o.untouched()
    assert call(lib, Outs(), buf, buf.size, off, ln, 0) == 0, lib.ouro_last_error()
