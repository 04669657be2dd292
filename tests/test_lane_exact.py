"""The lane routines -- fe25519.h, sc25519.h, lattice.h, modinv.h, sha512.h,
blake2b.h, ge25519.h and the chains of verify.h -- one call per item
(csrc/lane_items.h), against exact integer arithmetic (tests/lane_vectors.py),
bit for bit, on two backends:

  host    the items in a host loop (lib/libouro_devhost_test.so dh_lt_*): the
          vectors and references are proven on a CPU first;
  device  the same items from kernels, one item per lane
          (lib/libouro_lane_test.so lt_*, csrc/lane_test.hip), marked `gpu`.

The product's kernels reach these routines only with hash outputs in hand and
a verdict at the end; here the directed values run on the device too: p - 1,
unreduced limbs at their bounds, recoding digits of exactly +-2^(w-1), a carry
into the top window, L - 1, and a chain run with the window count of its
wave's largest item.  The test library is its own compilation of the same
source under the product's flags and launch bounds, not the product's binary."""
import ctypes
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

import edge_cases as E
import lane_vectors as V
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ouroboros-network_amd", "lib")
P, L = V.P, V.L
KIN, KOUT, KCHAIN, KED_IN, KUV_IN = 20, 20, 12, 44, 28
# csrc/lane_items.h enum Op
OPS = ["mul", "sq", "add", "sub", "sub4", "neg", "invert", "pow22523", "inv_vt", "inv_vt10",
       "inv_vt10_sel", "inv_vt30_spec", "sq_chain", "raw_words", "raw_carry", "raw_inv_vt",
       "raw_pack", "raw_mul", "raw_sq", "reduce512", "reduce256", "half_v2", "half_v1",
       "blake2b256_64", "decode", "decode_negate", "elligator2"]
OP = {name: k for k, name in enumerate(OPS)}


class Backend:
    """the lt_* entries of one library (`prefix`: dh_lt_ on the host build)"""

    def __init__(self, name):
        self.name = name
        host = os.path.join(LIBDIR, "libouro_devhost_test.so")
        if not os.path.exists(host):
            subprocess.run(["make", "-C", os.path.dirname(LIBDIR), "lib/libouro_devhost_test.so"],
                           check=True, stdout=subprocess.DEVNULL)
        self.hostlib = ctypes.CDLL(host)
        self.hostlib.dh_bound_violations.restype = ctypes.c_ulonglong
        self.hostlib.dh_untracked_loads.restype = ctypes.c_ulonglong
        self.untracked0 = self.hostlib.dh_untracked_loads()  # before this module's first item
        if name == "host":
            self.lib, self.prefix = self.hostlib, "dh_lt_"
        else:
            # a missing library is an error on a GPU run, not a skip
            self.lib, self.prefix = ctypes.CDLL(os.path.join(LIBDIR, "libouro_lane_test.so")), "lt_"
        width = ctypes.c_int()
        rest = [ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()]
        self.hostlib.dh_vrfkey_params(ctypes.byref(width), *(ctypes.byref(x) for x in rest))
        self.width = width.value

    def _fn(self, name, argtypes):
        f = getattr(self.lib, self.prefix + name)
        f.argtypes, f.restype = argtypes, ctypes.c_int
        return f

    def violations(self):
        return self.hostlib.dh_bound_violations()

    def op(self, name, recs, param=0):
        """item `name` over records of up to KIN words each; KOUT words each back"""
        a = np.zeros((len(recs), KIN), np.uint32)
        for i, r in enumerate(recs):
            a[i, :len(r)] = r
        out = np.zeros((len(recs), KOUT), np.uint32)
        f = self._fn("op", [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int])
        assert f(OP[name], len(recs), a.ctypes.data, out.ctypes.data, param) == 0
        return out

    def sha512(self, pre, buf, off, ln):
        n = len(pre)
        out = ctypes.create_string_buffer(64 * n)
        f = self._fn("sha512", [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
        o, l = np.array(off, np.uint32), np.array(ln, np.uint32)
        assert f(n, b"".join(pre), buf, len(buf), o.ctypes.data, l.ctypes.data, out) == 0
        return [out.raw[64 * i:64 * i + 64] for i in range(n)]

    def _chain(self, name, recs, words, stride, *mid):
        a = np.array(recs, np.uint32).reshape(len(recs), words)
        out = np.zeros((len(recs), KCHAIN), np.uint32)
        f = self._fn(name, [ctypes.c_int] * (2 + len(mid)) + [ctypes.c_void_p, ctypes.c_void_p])
        assert f(len(recs), stride, *mid, a.ctypes.data, out.ctypes.data) == 0
        return out

    def ed(self, recs, stride=1, variant=0):
        return self._chain("ed", recs, KED_IN, stride, variant)

    def u(self, recs, stride=1):
        return self._chain("u", recs, KUV_IN, stride)

    def v(self, recs, stride=1):
        return self._chain("v", recs, KUV_IN, stride)

    def u_table(self, keys, kidx, proofs, stride=1):
        out = np.zeros((len(kidx), KCHAIN), np.uint32)
        k = np.array(kidx, np.uint32)
        f = self._fn("u_table", [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p])
        assert f(len(keys), b"".join(keys), len(kidx), k.ctypes.data, b"".join(proofs), stride,
                 out.ctypes.data) == 0
        return out


@functools.lru_cache(maxsize=None)
def _backend(name):
    return Backend(name)


@pytest.fixture
def be(request, backend):
    if backend == "device":
        request.getfixturevalue("gpu_lib")  # torch's HIP runtime loads first (conftest.py)
    return _backend(backend)


both = pytest.mark.parametrize("backend", [pytest.param("host"),
                                           pytest.param("device", marks=pytest.mark.gpu)])


def val(row, at=0):
    return V.unwords(row[at:at + 8])


def enc(row):
    return np.asarray(row[:8], "<u4").tobytes()


def no_mismatch(bad):
    assert not bad, (len(bad), bad[:4])


# ---- references computed once, shared by the backends ---------------------------
@functools.lru_cache(maxsize=None)
def _ed():
    cases = V.ed_cases()
    recs = [V.bwords(E.enc_pt(A)) + V.bwords(E.enc_pt(R)) + V.words(abs(c0)) + V.words(c1) +
            V.words(b) + [1 if c0 < 0 else 0, bits, 0, 0] for A, R, c0, c1, b, bits in cases]
    return cases, recs, [V.ed_want(c) for c in cases]


def _uv_rec(a, b, c, s):
    return V.bwords(a) + V.bwords(b) + V.words(c, 4) + V.words(s)


@functools.lru_cache(maxsize=None)
def _u(width):
    cases = V.u_cases(width)
    return cases, [V.u_want(c) for c in cases]


@functools.lru_cache(maxsize=None)
def _v(width):
    cases = V.v_cases(width)
    return cases, [V.v_want(c) for c in cases]


# ---- field ------------------------------------------------------------------------------
@both
def test_field_ops(be):
    pairs = V.field_pairs()
    recs = [V.words(a) + V.words(b) for a, b in pairs]
    ra = [(a & V.M255) % P for a, _ in pairs]
    rb = [(b & V.M255) % P for _, b in pairs]
    want = {
        "mul": [a * b % P for a, b in zip(ra, rb)],
        "sq": [a * a % P for a in ra],
        "add": [(a + b) % P for a, b in zip(ra, rb)],
        "sub": [(a - b) % P for a, b in zip(ra, rb)],
        "sub4": [(a - b) % P for a, b in zip(ra, rb)],
        "neg": [-a % P for a in ra],
    }
    for name, w in want.items():
        out = be.op(name, recs)
        no_mismatch([(name, hex(pairs[i][0]), hex(pairs[i][1])) for i in range(len(recs))
                     if val(out[i]) != w[i]])


@both
def test_field_powers(be):
    vals = V.field_values()
    recs = [V.words(a) for a in vals]
    red = [(a & V.M255) % P for a in vals]
    inv = [pow(a, P - 2, P) for a in red]   # 0 -> 0, as the routines document
    want = {"invert": inv, "pow22523": [pow(a, 2**252 - 3, P) for a in red], "inv_vt": inv,
            "inv_vt10": inv, "inv_vt10_sel": inv, "inv_vt30_spec": inv}
    for name, w in want.items():
        out = be.op(name, recs)
        no_mismatch([(name, hex(vals[i])) for i in range(len(recs)) if val(out[i]) != w[i]])


@both
@pytest.mark.parametrize("k", [1, 2, 50, 254])
def test_squaring_chain_keeps_its_bounds(be, k):
    vals = V.field_values()
    out = be.op("sq_chain", [V.words(a) for a in vals], k)
    no_mismatch([hex(a) for i, a in enumerate(vals)
                 if val(out[i]) != pow((a & V.M255) % P, 2**k, P)])


@both
def test_raw_limbs(be):
    """fe_make inputs at and beyond the reduced bounds, each top only where the
    routine's documented input bound admits it (lane_vectors.RAW_OP_TOPS); on
    the host the bound tracker agrees that every such input is legal."""
    before = be.violations()
    for top in V.RAW_TOPS:
        limbs = V.raw_limbs(top)
        x = [V.limbs_value(l) for l in limbs]
        partner = [limbs[(7 * i + 3) % len(limbs)] for i in range(len(limbs))]
        recs = [l + g for l, g in zip(limbs, partner)] + [l + l for l in limbs]
        bad = []
        if top in V.RAW_OP_TOPS["words"]:
            out = be.op("raw_words", recs[:len(limbs)])
            bad += [("words", l) for i, l in enumerate(limbs) if val(out[i]) != x[i] % P]
        if top in V.RAW_OP_TOPS["inv_vt"]:
            out = be.op("raw_inv_vt", recs[:len(limbs)])
            bad += [("inv_vt", l) for i, l in enumerate(limbs) if val(out[i]) != pow(x[i] % P, P - 2, P)]
        if top in V.RAW_OP_TOPS["carry"]:
            out = be.op("raw_carry", recs[:len(limbs)])
            for i, l in enumerate(limbs):
                w = V.fe_carry_limbs(l)
                if list(out[i][8:18]) != w or val(out[i]) != x[i] % P:
                    bad.append(("carry", l))
        if top in V.RAW_OP_TOPS["pack"]:
            out = be.op("raw_pack", recs[:len(limbs)])
            for i, l in enumerate(limbs):
                w, back = val(out[i]), [int(v) for v in out[i][8:18]]
                ok = w % P == x[i] % P and V.limbs_value(back) == w and back[9] < 1 << 26 and \
                    all(back[j] <= V.LIMB_MASK[j] for j in range(9))
                if not ok:
                    bad.append(("pack", l))
        # a product is "Reduced" (csrc/fe25519.h): limbs within their masks but
        # limb 1 <= 2^25 + 2^18 and limb 6 <= 2^26 + 2^12
        cap = list(V.LIMB_MASK)
        cap[1], cap[6] = 2**25 + 2**18, 2**26 + 2**12
        if top in V.RAW_OP_TOPS["mul"]:
            out = be.op("raw_mul", recs)
            for i, r in enumerate(recs):
                w = V.limbs_value(r[:10]) * V.limbs_value(r[10:]) % P
                h = [int(v) for v in out[i][8:18]]
                if val(out[i]) != w or V.limbs_value(h) % P != w or any(a > c for a, c in zip(h, cap)):
                    bad.append(("mul", r))
        if top in V.RAW_OP_TOPS["sq"]:
            out = be.op("raw_sq", recs[:len(limbs)])
            for i, l in enumerate(limbs):
                h = [int(v) for v in out[i][8:18]]
                if val(out[i]) != x[i] * x[i] % P or V.limbs_value(h) % P != x[i] * x[i] % P or \
                        any(a > c for a, c in zip(h, cap)):
                    bad.append(("sq", l))
        assert not bad, (top.bit_length() - 1, len(bad), bad[:3])
    if be.name == "host":
        assert be.violations() == before
    assert 1 << 26 in V.RAW_OP_TOPS["mul"] and 1 << 26 in V.RAW_OP_TOPS["sq"] and \
        1 << 26 in V.RAW_OP_TOPS["carry"]


# ---- scalars ------------------------------------------------------------------------------
@both
def test_scalar_reduce(be):
    ins = V.reduce512_inputs()
    out = be.op("reduce512", [V.bwords(b) for b in ins])
    no_mismatch([b.hex() for i, b in enumerate(ins) if val(out[i]) != int.from_bytes(b, "little") % L])
    xs = V.reduce256_inputs()
    out = be.op("reduce256", [V.words(x) for x in xs])
    no_mismatch([hex(x) for i, x in enumerate(xs) if val(out[i]) != x % L])


@both
def test_half_scalars(be):
    """c0 = c1 h (mod 8L), c1 odd and in range, bits as documented; the
    round-6 step equals the round-1 step on this backend, and on the device
    both equal the HOST's round-1 step: lattice.h's "same quotients, same
    breaks, bit for bit" with the device's reciprocal (recip_f64)."""
    hs = V.half_inputs()
    recs = [V.words(h) for h in hs]
    v2, v1 = be.op("half_v2", recs), be.op("half_v1", recs)
    bad = []
    for i, h in enumerate(hs):
        c0, c1, neg, bits = val(v2[i]), val(v2[i], 8), int(v2[i][16]), int(v2[i][17])
        c0 = -c0 if neg else c0
        ok = c1 % 2 == 1 and 0 < c1 < L and (c0 - c1 * h) % (8 * L) == 0 and \
            bits == max(abs(c0).bit_length(), c1.bit_length()) and neg in (0, 1)
        if not ok:
            bad.append(("relation", hex(h)))
        if list(v2[i][:18]) != list(v1[i][:18]):
            bad.append(("v2 != v1", hex(h)))
    no_mismatch(bad)
    if be.name == "device":
        host_v1 = _backend("host").op("half_v1", recs)
        no_mismatch([hex(h) for i, h in enumerate(hs) if list(v2[i][:18]) != list(host_v1[i][:18])])


# ---- hashes -------------------------------------------------------------------------------
@both
def test_sha512_tail_at_every_offset(be):
    pre, buf, off, ln, want = V.sha_cases()
    got = be.sha512(pre, buf, off, ln)
    no_mismatch([(ln[i], off[i] % 8) for i in range(len(want)) if got[i] != want[i]])


@both
def test_blake2b256_64(be):
    rng = np.random.default_rng(0xb2b)
    ins = [bytes(64), b"\xff" * 64] + [rng.bytes(64) for _ in range(62)]
    out = be.op("blake2b256_64", [V.bwords(b) for b in ins])
    no_mismatch([b.hex() for i, b in enumerate(ins)
                 if enc(out[i]) != hashlib.blake2b(b, digest_size=32).digest()])


# ---- decode, Elligator2 ---------------------------------------------------------------------
@both
@pytest.mark.parametrize("negate", [False, True])
def test_decode(be, negate):
    ins = V.decode_inputs()
    out = be.op("decode_negate" if negate else "decode", [V.bwords(b) for b in ins])
    bad, undecodable = [], 0
    for i, b in enumerate(ins):
        ok, canon, small, x, y = V.decode_want(b, negate)
        undecodable += not ok
        got = (int(out[i][0]), int(out[i][1]), int(out[i][2]))
        if got != (int(ok), int(canon), int(small)) or \
                (ok and (val(out[i], 4), val(out[i], 12)) != (x, y)):
            bad.append(b.hex())
    no_mismatch(bad)
    assert 30 < undecodable < len(ins) - 30


@both
def test_elligator2(be):
    rs = V.elligator_inputs()
    out = be.op("elligator2", [V.bwords(r) for r in rs])
    no_mismatch([r.hex() for i, r in enumerate(rs) if enc(out[i]) != O.elligator2(r)])


# ---- the chains ------------------------------------------------------------------------------
def _chain_bad(out, want, label):
    """encoding == enc_pt of the exact point; identity flag == (it is the identity)"""
    return [(label[i], enc(out[i]).hex()) for i in range(len(want)) if want[i] is not None and
            (enc(out[i]) != E.enc_pt(want[i]) or int(out[i][8]) != int(want[i] == V.IDENT))]


def _ed_label(c):
    A, R, c0, c1, b, bits = c
    return (E.enc_pt(A).hex(), E.enc_pt(R).hex(), hex(c0), hex(c1), hex(b))


@both
@pytest.mark.parametrize("variant", [0, 1], ids=["dsm_lane", "dsm_lane_dsm_launch"])
def test_chain_ed(be, variant):
    cases, recs, want = _ed()
    out = be.ed(recs, 1, variant)
    no_mismatch(_chain_bad(out, want, [_ed_label(c) for c in cases]))
    assert all(int(o[9]) == 1 and int(o[10]) == 1 for o in out)
    assert sum(w == V.IDENT for w in want) >= 12


@both
def test_chain_u(be):
    cases, want = _u(be.width)
    out = be.u([_uv_rec(pk, bytes(32), c, s) for pk, c, s in cases])
    label = [(pk.hex(), hex(c), hex(s)) for pk, c, s in cases]
    decodable = [w if pk not in (V.NON_CANONICAL, V.NO_DECODE) else None
                 for (pk, _, _), w in zip(cases, want)]
    no_mismatch(_chain_bad(out, decodable, label))
    no_mismatch([label[i] for i, (pk, _, _) in enumerate(cases) if int(out[i][9]) != int(V.u_flag(pk))])


@both
def test_chain_v(be):
    cases, want = _v(be.width)
    out = be.v([_uv_rec(E.enc_pt(H), E.enc_pt(G), c, s) for H, G, c, s in cases])
    no_mismatch(_chain_bad(out, want, [(E.enc_pt(H).hex(), E.enc_pt(G).hex(), hex(c), hex(s))
                                       for H, G, c, s in cases]))
    assert all(int(o[9]) == 1 and int(o[10]) == 1 for o in out)


@both
def test_u_from_the_key_table(be):
    """the flag is the inline core's, and U is the exact [s]B - [c]Y for every
    decodable key, small-order keys included"""
    cases, want = _u(be.width)
    keys = list(dict.fromkeys(pk for pk, _, _ in cases))
    kidx = [keys.index(pk) for pk, _, _ in cases]
    proofs = [bytes(32) + c.to_bytes(16, "little") + s.to_bytes(32, "little") for _, c, s in cases]
    out = be.u_table(keys, kidx, proofs)
    inline = be.u([_uv_rec(pk, bytes(32), c, s) for pk, c, s in cases])
    label = [(pk.hex(), hex(c), hex(s)) for pk, c, s in cases]
    decodable = [w if pk not in (V.NON_CANONICAL, V.NO_DECODE) else None
                 for (pk, _, _), w in zip(cases, want)]
    no_mismatch(_chain_bad(out, decodable, label))
    no_mismatch([label[i] for i in range(len(cases)) if int(out[i][9]) != int(inline[i][9])])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["dsm_lane", "dsm_lane_dsm_launch"])
def test_chain_ed_neighbour_independence(gpu_lib, variant):
    """verify.h wave_max_small: a packed wave runs every item with the window
    count of its largest one.  Packed, one item per wave, packed in reverse
    order, and the first 1, 63 and 65 items alone: the same bytes per item
    every time, and the exact ones."""
    be = _backend("device")
    cases, recs, want = _ed()
    label = [_ed_label(c) for c in cases]
    own = [max(1, min(64, (c[5] + 4) >> 2)) for c in cases]
    packed = be.ed(recs, 1, variant)
    alone = be.ed(recs, 64, variant)
    rev = be.ed(recs[::-1], 1, variant)[::-1]
    no_mismatch(_chain_bad(packed, want, label))
    assert [int(o[11]) for o in alone] == own
    assert all(int(o[11]) >= w for o, w in zip(packed, own))
    assert sum(int(o[11]) > w for o, w in zip(packed, own)) > len(cases) // 2
    for other in (alone, rev):
        no_mismatch([label[i] for i in range(len(cases)) if list(other[i][:11]) != list(packed[i][:11])])
    for n in (1, 63, 65):
        part = be.ed(recs[:n], 1, variant)
        no_mismatch([label[i] for i in range(n) if list(part[i][:11]) != list(packed[i][:11])])


def test_zero_bound_violations():
    """Over everything the host backend ran above, every multiplier input
    stayed inside the limb bounds fe25519.h assumes and no element was loaded
    from memory the tracker had not seen written (run last in this module)."""
    be = _backend("host")
    before = be.hostlib.dh_untracked_loads()
    cases, recs, _ = _ed()
    be.ed(recs[:8], 1, 0)
    be.ed(recs[:8], 1, 1)
    ucases, _ = _u(be.width)
    be.u([_uv_rec(pk, bytes(32), c, s) for pk, c, s in ucases[:8]])
    vcases, _ = _v(be.width)
    be.v([_uv_rec(E.enc_pt(H), E.enc_pt(G), c, s) for H, G, c, s in vcases[:8]])
    assert be.hostlib.dh_untracked_loads() == before
    # ... and over every host item of this module since its backend was made
    assert be.hostlib.dh_untracked_loads() == be.untracked0
    assert be.violations() == 0
