"""ouro_chain_validate_cbor_host (CPU-only): the combined entry's crypto
outputs equal chain_cases.expect_chain (the pinned slicers + the oracle), its
envelope equals envelope.py, and the accepted prefix is what a sequential fold
over both gives -- on a chain with real linkage across Byron, the era switch
and three TPraos epochs."""
import ctypes

import numpy as np

import chain_cases as CC
import envelope_cases as EC
from ouroboros_network_amd import _native
from ouroboros_network_amd import envelope as E
from ouroboros_network_amd import header as H

CFG = EC.VAL_CFG


def assert_validate(got, raws, want_crypto, want_env):
    crypto, hh, bits, tip, accepted = got
    CC.assert_chain_equal(crypto, want_crypto)
    assert [bytes(h) for h in hh] == want_env[1]
    assert list(bits) == want_env[2]
    assert tip == want_env[3]
    valid = [(v == 1) if p == H.PROTO_PBFT else (v & 0xF) == 0xF
             for p, v in zip(want_crypto[0], want_crypto[2])]
    assert accepted == E.first_invalid(want_env[2], valid)


def test_host_path_on_a_linked_chain_across_eras_and_epochs():
    raws, ea, la, want_crypto, want_env = EC.validate_stream()
    nb = 30
    # the chain links throughout but for the header whose signature was flipped
    # (its hash moved, so its successor's link breaks too)
    assert [i for i, b in enumerate(want_env[2]) if b != E.ENV_ALL_OK] == [nb + 6]
    assert (want_crypto[2][nb:] & 0xF).tolist().count(0xF) == len(raws) - nb - 1
    got = H.validate_chain_cbor(raws, CC.SPKP, -1, cfg=CFG, epochs=CC.sched3(), nonce=True,
                                host=True)
    assert_validate(got, raws, want_crypto, want_env)
    # the Byron golden forms carry the golden signature over other fields: PBFT
    # rejects the first regular header, and the fold stops there
    assert got[4] == 1
    # the TPraos part alone, on top of the last Byron header as the tip
    tip = E.validate_envelope(raws[:nb], E.ORIGIN, CFG)[3]
    got = H.validate_chain_cbor(raws[nb:], CC.SPKP, -1, cfg=CFG, tip=tip, epochs=CC.sched3(),
                                nonce=True, host=True)
    assert list(got[2]) == want_env[2][nb:]
    assert got[4] == 5  # up to the flipped signature
    # explicit alphas instead of the schedule: the same answers
    got = H.validate_chain_cbor(raws, CC.SPKP, -1, cfg=CFG, eta_alpha=ea, leader_alpha=la,
                                nonce=True, host=True)
    assert_validate(got, raws, want_crypto, want_env)


def test_the_existing_entry_gives_the_same_crypto_outputs():
    raws, ea, la, _, _ = EC.validate_stream()
    a = H.verify_chain_cbor(raws, CC.SPKP, -1, epochs=CC.sched3(), nonce=True, host=True)
    b = H.validate_chain_cbor(raws, CC.SPKP, -1, cfg=CFG, epochs=CC.sched3(), nonce=True,
                              host=True)[0]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_argument_checks():
    lib = _native.load()
    raws = EC.good_chain(3, 2)
    buf, off, ln = H.raw_triplet(raws)
    n = len(raws)
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    proto, st, v, hh, bits = z(n), z(n), z(n), z(n, 32), z(n)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    cfg = _native.EnvelopeCfg(byron_epoch_slots=EC.EPOCH_SLOTS)

    def call(entry, cfg_=cfg, tip_=None, hh_=hh, bits_=bits, spkp=100):
        return getattr(lib, entry)(ptr(buf), buf.size, ptr(off), ptr(ln), n, spkp, -1, None, None,
                                   None, ctypes.byref(cfg_) if cfg_ is not None else None,
                                   ctypes.byref(tip_) if tip_ is not None else None, ptr(proto),
                                   ptr(st), ptr(v), None, None, None, ptr(hh_), ptr(bits_), None)

    for entry in ("ouro_chain_validate_cbor_host", "ouro_chain_validate_cbor"):
        assert call(entry, hh_=None) == _native.OURO_EINVAL
        assert call(entry, bits_=None) == _native.OURO_EINVAL
        assert call(entry, cfg_=None) == _native.OURO_EINVAL
        assert call(entry, cfg_=_native.EnvelopeCfg()) == _native.OURO_EINVAL
        assert call(entry, tip_=_native.ChainTip(origin=1, block_no=3)) == _native.OURO_EINVAL
        assert call(entry, spkp=0) == _native.OURO_EINVAL  # the chain entry's own checks
    # an empty batch still has its tip checked
    for entry in ("ouro_chain_validate_cbor_host", "ouro_chain_validate_cbor"):
        bad = _native.ChainTip(origin=1, block_no=3)
        assert getattr(lib, entry)(ptr(buf), buf.size, ptr(off), ptr(ln), 0, 100, -1, None, None,
                                   None, ctypes.byref(cfg), ctypes.byref(bad), ptr(proto), ptr(st),
                                   ptr(v), None, None, None, ptr(hh), ptr(bits),
                                   None) == _native.OURO_EINVAL
    assert call("ouro_chain_validate_cbor_host") == _native.OURO_OK
    assert list(bits) == [E.ENV_ALL_OK] * n
