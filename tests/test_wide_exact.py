"""The latency mode's wave-wide routines -- csrc/wide.h, wide_cores.h,
wide_inv.h, wide_blake2b.h -- against exact integer arithmetic
(tests/wide_vectors.py, lane_vectors.py), bit for bit.

  CPU   the integer model of the limb flow proves every directed vector legal
        for the routine it is fed to and holds each documented bound to its
        own arithmetic; the split forms' scalar helpers and the wide B table
        on the host build (lib/libouro_devhost_test.so dh_wide_*, dh_btab_wide_entry);
  gpu   the routines one by one, one wave per record (lib/libouro_wide_test.so
        ouro_wx_op, csrc/wide_test.hip): raw signed limbs at the documented
        bounds, four unrelated rows per wave, non-canonical zeros, every table
        digit, truncated window counts, the split forms' halves summed.

The wave-wide code is a second implementation of the field, the group and
the chains (signed radix-2^16 limbs across a DPP row), device-only, with no
bound tracker: an operand out of range wraps silently in s24().  The product
reaches it only through whole-header verdicts."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import edge_cases as E
import lane_vectors as V
import wide_vectors as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "ouroboros-network_amd", "lib")
P, L = V.P, V.L
NL = W.NL
# csrc/wide_test.hip enum WxOp
OPS = ["mul", "sq", "mul_rep", "sq_rep", "carry3", "carry2", "carry_rows", "norm", "gather", "sel4",
       "add_rows32", "add_rows64", "fe_to_fw", "to_fe", "pow_rows", "pow", "inv", "inv_sel",
       "dbl", "add", "tab", "add_p3", "is_id", "st_ld", "enc", "decode", "decode_pair",
       "dsm", "dsm_t2", "dsm_b1", "dsm_b2", "dsm_b", "dsm_t2b", "ed_half", "v_part", "blake"]
OP = {name: k for k, name in enumerate(OPS)}


def no_mismatch(bad):
    assert not bad, (len(bad), bad[:3])


# ==== CPU: the model, the vectors, the documented bounds ==================================
OPERANDS = {  # routine operand -> the documented bound of its directed vectors
    "mul_f": W.FOUR_TERM, "mul_g": W.NARROW, "rep_f": W.FOUR_TERM, "rep_g": W.NARROW,
    "sq": W.NARROW, "sq_rep": W.NARROW, "norm": W.NORM_IN,
}


@functools.lru_cache(maxsize=None)
def vectors(operand):
    if operand == "to_fe":
        return W.to_fe_vectors()
    return W.directed(OPERANDS[operand], 0x3140 + sorted(OPERANDS).index(operand))


def test_every_directed_vector_is_legal():
    for operand in list(OPERANDS) + ["to_fe"]:
        bad = [v for v in vectors(operand) if not W.legal(operand, v)]
        assert not bad, (operand, len(bad), bad[:2])
    # both operands at their bounds at once, every sign pattern
    f, g = vectors("mul_f")[:4], vectors("mul_g")[:4]
    for a in f:
        for b in g:
            W.fw_mul(a, b)
            W.fw_mul_rep(a, b)
    for b in g:
        W.fw_mul(b, b)
        W.fw_sq_rep(b)


def test_respread_preserves_the_value_and_fills_the_bound():
    rng = np.random.default_rng(0x5e5e)
    for bound in (W.CARRY3_CAP, W.CARRIED, W.NARROW, W.FOUR_TERM):
        for _ in range(50):
            x = int.from_bytes(rng.bytes(32), "little") % P
            l = W.respread(W.canon(x), bound, rng)
            assert W.value(l) == x and max(abs(v) for v in l) <= bound and min(l) < 0
    for z in W.zero_vectors(W.CARRIED, 1):
        assert W.value(z) == 0


def test_model_conversion_is_the_value_mod_p():
    for x in vectors("to_fe") + W.zero_vectors(W.TO_FE_NEG_TOP, 2):
        assert W.fw_to_fe(x) == W.value(x), x


def _within(limbs, cap):
    return max(abs(v) for v in limbs) <= cap and W.LIMB15_MIN <= limbs[15] <= W.LIMB15_MAX


def test_documented_bounds_hold_under_the_model():
    """each bound a header comment states, run through the model at its worst
    case: the accumulator caps, the carried-limb caps of every carry form, the
    narrow operand's three-term budget, fw_to_fe's negative-limb precondition"""
    # the carry forms at their accumulator caps
    for acc in W.acc_vectors(W.ACC_CAP, 0xacc1):
        assert _within(W.fw_carry3(acc), W.CARRY3_CAP), "wide.h fw_carry: limbs |l| < 2^16.01"
        assert _within(W.fw_carry2(acc), W.CARRY2_CAP), "wide.h fw_carry2: below 2^16.03"
        assert W.value(W.fw_carry2(acc)) == W.value(W.fw_carry3(acc)) == \
            sum(a << (16 * k) for k, a in enumerate(acc)) % P
    rows = W.acc_vectors(W.ROW_ACC_CAP, 0xacc2)
    for i in range(len(rows)):
        accs = [rows[(i + 5 * r) % len(rows)] for r in range(4)]
        assert _within(W.fw_carry_rows(accs), W.ROWS_CAP), "wide.h fw_carry_rows: below 2^16.13"
    for x in vectors("norm"):
        out = W.fw_norm(x)
        assert _within(out, W.NORM_CAP) and W.value(out) == W.value(x), "wide_cores.h fw_norm"
    # products of the worst-case operands: the model raises if an accumulator
    # passes its documented cap (wide.h header 2^45.1; fw_carry_rows 2^43.2 per row)
    worst = 0
    for sf in (1, -1):
        for sg in (1, -1):
            f, g = [sf * W.FOUR_TERM] * NL, [sg * W.NARROW] * NL
            assert _within(W.fw_mul(f, g), W.CARRY2_CAP)
            assert _within(W.fw_mul_rep(f, g), W.ROWS_CAP)
            worst = max(worst, max(abs(a) for acc in W.rep_accs(f, g) for a in acc))
    # ... and the per-row cap is not the 2^43.1 the comment once gave
    assert int(2 ** 43.1) < worst < W.ROW_ACC_CAP
    assert 3 * W.CARRIED <= W.NARROW, "wide.h: three carried elements fit the narrow operand"
    # fw_to_fe: legal down to -4 p_k limb by limb (checked by the vectors'
    # legality above), and the callers' two-term differences are inside
    assert W.legal("to_fe", [-2 * W.CARRIED] * 15 + [W.LIMB15_MIN - W.LIMB15_MAX])
    assert W.TO_FE_NEG_TOP == 131068 < 2 ** 17 - 1, "wide.h fw_to_fe: limb 15 takes only 4 * 0x7fff"


# ---- the split forms' scalar helpers on the host build ------------------------------------
@functools.lru_cache(maxsize=None)
def hostlib():
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libouro_devhost_test.so"))
    lib.dh_wide_recode4.restype = ctypes.c_ulonglong
    return lib


def _w8(x):
    return (ctypes.c_uint32 * 8)(*V.words(x))


def host_recode4(s):
    d = (ctypes.c_int32 * 64)()
    mask = hostlib().dh_wide_recode4(_w8(s), d)
    return list(d), mask


def host_high_from_window(which, s):
    hh = (ctypes.c_uint32 * 8)()
    K = hostlib().dh_wide_high_from_window(which, hh, _w8(s))
    return V.unwords(hh), K


def split_ks():
    ks, v3 = (ctypes.c_int * 4)(), ctypes.c_int()
    assert hostlib().dh_wide_split_ks(ks, ctypes.byref(v3)) == 4
    return list(ks), v3.value


def test_recoding_restated_in_python_is_the_codes():
    ss = V.s_directed() + V.b_directed() + W.split_scalars(48) + [2 ** 256 - 1]
    for s in ss:
        d, mask = W.recode4(s)
        assert sum(dj << (4 * j) for j, dj in enumerate(d)) == s
        assert all(-7 <= dj <= 8 for dj in d[:63])
        assert host_recode4(s) == (d, mask), hex(s)


def test_split_ks_cover_the_product_and_both_shift_shapes():
    ks, _ = split_ks()
    assert any((4 * k) % 32 == 0 for k in ks[2:]) and any((4 * k) % 32 != 0 for k in ks[2:])


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_high_from_window_sums_exactly(which):
    """windows 0..K-1 recoded from the whole s, plus hh 16^K, are s; hh is
    s >> 4K plus the carry of window K - 1"""
    K = split_ks()[0][which]
    bad = []
    for s in W.split_scalars(K):
        hh, k = host_high_from_window(which, s)
        assert k == K
        carry = hh - (s >> (4 * K))
        if carry not in (0, 1) or W.window_sum(s, 0, K) + (hh << (4 * K)) != s or \
                carry != (W.recode4(s)[1] >> K) & 1:
            bad.append(hex(s))
    no_mismatch(bad)


def test_v_parts_of_the_product_sum_exactly():
    """vrf_sh_split's cuts: s = windows 0..K-1 of s, windows 0..K2-K-1 of hh
    (or all of hh without the third part), and hh2 at 16^K2"""
    (K, K2rel, _, _), v3 = split_ks()
    bad = []
    for s in W.split_scalars(K):
        hh, _ = host_high_from_window(0, s)
        hh2, _ = host_high_from_window(1, hh)
        three = W.window_sum(s, 0, K) + (W.window_sum(hh, 0, K2rel) << (4 * K)) + (hh2 << (4 * (K + K2rel)))
        two = W.window_sum(s, 0, K) + (W.window_sum(hh, 0, 64 - K) << (4 * K))
        if three != s or two != s:
            bad.append(hex(s))
    no_mismatch(bad)
    assert v3 in (0, 1)


def test_high_half_with_carry_sums_exactly():
    bad = []
    for h in W.split_scalars(32) + V.HALF_HS:
        hh = (ctypes.c_uint32 * 8)()
        hostlib().dh_wide_high_half(hh, _w8(h))
        x = V.unwords(hh)
        if x - (h >> 128) not in (0, 1) or W.window_sum(h, 0, 32) + (x << 128) != h or \
                W.window_sum(h, 0, 32) + (W.window_sum(x, 0, 32) << 128) != h:
            bad.append(hex(h))
    no_mismatch(bad)


def test_wide_b_table_entries_are_the_exact_multiples():
    rng = np.random.default_rng(0xb7ab)
    ks = [1, 2, 3, 2 ** 15 - 1, 2 ** 15] + [int(rng.integers(4, 2 ** 15)) for _ in range(6)]
    bad = []
    for half in (0, 1):
        for k in ks:
            out = (ctypes.c_uint16 * 48)()
            assert hostlib().dh_btab_wide_entry(half, k - 1, out) == 0
            x, y = V.smul(k << (128 * half), E.BASE)
            want = W.canon(y - x) + W.canon(y + x) + W.canon(2 * E.D * x * y)
            if list(out) != want:
                bad.append((half, k))
    no_mismatch(bad)
    out = (ctypes.c_uint16 * 48)()
    assert hostlib().dh_btab_wide_entry(0, 2 ** 15, out) == -1


# ==== the device ==========================================================================
class Wx:
    def __init__(self):
        # a missing library is an error on a GPU run, not a skip
        self.lib = ctypes.CDLL(os.path.join(LIBDIR, "libouro_wide_test.so"))
        v = [ctypes.c_int() for _ in range(6)]
        assert self.lib.ouro_wx_params(*(ctypes.byref(x) for x in v)) == 0
        self.kin, self.kout, self.vwin, self.vwin2, self.v3, nops = (x.value for x in v)
        assert nops == len(OPS)
        self.lib.ouro_wx_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def run(self, name, recs):
        """recs: per wave a dict slot -> 64 int32 words; (n, kout, 64) int64 back"""
        a = np.zeros((len(recs), self.kin, 64), np.int32)
        for i, r in enumerate(recs):
            for k, w in r.items():
                a[i, k, :len(w)] = np.asarray([int(v) & 0xffffffff for v in w], np.uint32).view(np.int32)
        out = np.zeros((len(recs), self.kout, 64), np.int32)
        rc = self.lib.ouro_wx_op(OP[name], len(recs), a.ctypes.data, out.ctypes.data)
        assert rc == 0, "ouro_wx_op returned %d" % rc
        return out.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _wx():
    return Wx()


@pytest.fixture
def wx(gpu_lib):  # torch's HIP runtime loads first (conftest.py)
    return _wx()


def rows4(r0, r1, r2, r3):
    return list(r0) + list(r1) + list(r2) + list(r3)


def rep(l):
    return list(l) * 4


def row(out, i, slot, r):
    return [int(v) for v in out[i, slot, 16 * r:16 * r + 16]]


def uwords(x, n=8):
    return V.words(x, n)


def cap_ok(limbs, cap):
    return _within(limbs, cap)


# ---- products ------------------------------------------------------------------------------
def _pairs():
    f, g = vectors("mul_f"), vectors("mul_g")
    prs = [(a, g[i % len(g)]) for i, a in enumerate(f)] + \
        [(a, g[(7 * i + 3) % len(g)]) for i, a in enumerate(f)]
    prs += [(a, b) for a in f[:4] for b in g[:4]]           # both at their bounds, every sign
    return prs


@pytest.mark.gpu
def test_products_per_row(wx):
    """fw_mul and fw_sq with four unrelated rows per wave: the value of every
    row, limbs within fw_carry2's cap and equal to the model's"""
    prs = _pairs()
    prs += [prs[-1]] * (-len(prs) % 4)
    # rows of a wave drawn far apart, so a wrong row is a wrong value
    n = len(prs) // 4
    waves = [[prs[w + n * r] for r in range(4)] for w in range(n)]
    out = wx.run("mul", [{0: rows4(*[p[0] for p in wv]), 1: rows4(*[p[1] for p in wv])} for wv in waves])
    bad = []
    for i, wv in enumerate(waves):
        for r, (f, g) in enumerate(wv):
            got = row(out, i, 0, r)
            if W.value(got) != W.value(f) * W.value(g) % P or not cap_ok(got, W.CARRY2_CAP) or \
                    got != W.fw_mul(f, g):
                bad.append(("mul", r, f, g))
    no_mismatch(bad)
    sq = vectors("sq")
    sq += [sq[-1]] * (-len(sq) % 4)
    n = len(sq) // 4
    waves = [[sq[w + n * r] for r in range(4)] for w in range(n)]
    out = wx.run("sq", [{0: rows4(*wv)} for wv in waves])
    for i, wv in enumerate(waves):
        for r, f in enumerate(wv):
            got = row(out, i, 0, r)
            if W.value(got) != W.value(f) ** 2 % P or not cap_ok(got, W.CARRY2_CAP) or got != W.fw_mul(f, f):
                bad.append(("sq", r, f))
    no_mismatch(bad)


@pytest.mark.gpu
def test_products_replicated(wx):
    """fw_mul_rep and fw_sq_rep: the value, four identical rows, limbs within
    fw_carry_rows' cap and equal to the model's"""
    f, g = vectors("rep_f"), vectors("rep_g")
    prs = [(a, g[(5 * i + 1) % len(g)]) for i, a in enumerate(f)] + [(a, b) for a in f[:4] for b in g[:4]]
    out = wx.run("mul_rep", [{0: rep(a), 1: rep(b)} for a, b in prs])
    bad = []
    for i, (a, b) in enumerate(prs):
        got = [row(out, i, 0, r) for r in range(4)]
        if got[0] != W.fw_mul_rep(a, b) or any(x != got[0] for x in got) or \
                W.value(got[0]) != W.value(a) * W.value(b) % P or not cap_ok(got[0], W.ROWS_CAP):
            bad.append(("mul_rep", a, b))
    sq = vectors("sq_rep")
    out = wx.run("sq_rep", [{0: rep(a)} for a in sq])
    for i, a in enumerate(sq):
        got = [row(out, i, 0, r) for r in range(4)]
        if got[0] != W.fw_sq_rep(a) or any(x != got[0] for x in got) or \
                W.value(got[0]) != W.value(a) ** 2 % P or not cap_ok(got[0], W.ROWS_CAP):
            bad.append(("sq_rep", a))
    no_mismatch(bad)


# ---- carries -------------------------------------------------------------------------------
def _acc_slots(lanes64):
    lo = [a & 0xffffffff for a in lanes64]
    hi = [(a >> 32) & 0xffffffff for a in lanes64]
    return {0: lo, 1: hi}


@pytest.mark.gpu
def test_carries(wx):
    accs = W.acc_vectors(W.ACC_CAP, 0xacc1)
    accs += [accs[-1]] * (-len(accs) % 4)
    n = len(accs) // 4
    waves = [[accs[w + n * r] for r in range(4)] for w in range(n)]
    recs = [_acc_slots(rows4(*wv)) for wv in waves]
    bad = []
    for name, model, cap in (("carry3", W.fw_carry3, W.CARRY3_CAP), ("carry2", W.fw_carry2, W.CARRY2_CAP)):
        out = wx.run(name, recs)
        for i, wv in enumerate(waves):
            for r, acc in enumerate(wv):
                got = row(out, i, 0, r)
                if got != model(acc) or not cap_ok(got, cap) or \
                        W.value(got) != sum(a << (16 * k) for k, a in enumerate(acc)) % P:
                    bad.append((name, r, acc))
    rows = W.acc_vectors(W.ROW_ACC_CAP, 0xacc2)
    waves = [[rows[(i + 5 * r) % len(rows)] for r in range(4)] for i in range(len(rows))]
    out = wx.run("carry_rows", [_acc_slots(rows4(*wv)) for wv in waves])
    for i, wv in enumerate(waves):
        got = [row(out, i, 0, r) for r in range(4)]
        total = sum(sum(a << (16 * k) for k, a in enumerate(acc)) for acc in wv) % P
        if got[0] != W.fw_carry_rows(wv) or any(x != got[0] for x in got) or \
                not cap_ok(got[0], W.ROWS_CAP) or W.value(got[0]) != total:
            bad.append(("carry_rows", wv))
    xs = vectors("norm")
    xs += [xs[-1]] * (-len(xs) % 4)
    n = len(xs) // 4
    waves = [[xs[w + n * r] for r in range(4)] for w in range(n)]
    out = wx.run("norm", [{0: rows4(*wv)} for wv in waves])
    for i, wv in enumerate(waves):
        for r, x in enumerate(wv):
            got = row(out, i, 0, r)
            if got != W.fw_norm(x) or not cap_ok(got, W.NORM_CAP) or W.value(got) != W.value(x):
                bad.append(("norm", r, x))
    no_mismatch(bad)


# ---- row exchanges ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_row_exchanges(wx):
    """fw_gather, sel4, add_rows_i32, add_rows_u64 on four distinct rows: every
    lane's result"""
    rng = np.random.default_rng(0x6a7e)
    n = 8
    x = rng.integers(-2 ** 31, 2 ** 31, (n, 4, 64)).astype(np.int64)
    x[0, 0] = np.arange(64)                      # lane ids: a permutation shows as itself
    out = wx.run("gather", [{0: list(x[i, 0])} for i in range(n)])
    for i in range(n):
        for r in range(4):
            want = np.tile(x[i, 0, 16 * r:16 * r + 16], 4)
            assert (out[i, r] == want).all(), ("gather", r)
    out = wx.run("sel4", [{k: list(x[i, k]) for k in range(4)} for i in range(n)])
    for i in range(n):
        want = np.concatenate([x[i, r, 16 * r:16 * r + 16] for r in range(4)])
        assert (out[i, 0] == want).all(), "sel4"
    small = x >> 3                                # the sums stay inside 32 bits
    out = wx.run("add_rows32", [{0: list(small[i, 0])} for i in range(n)])
    for i in range(n):
        want = np.tile(small[i, 0].reshape(4, 16).sum(axis=0), 4)
        assert (out[i, 0] == want).all(), "add_rows_i32"
    big = [[int(a) * 2 ** 29 + int(b) for a, b in zip(x[i, 0], x[i, 1])] for i in range(n)]
    big[0] = [2 ** 61 - 1 - k for k in range(64)]
    big[1] = [(0xffffffff if k < 32 else 1) for k in range(64)]   # a carry across bit 32
    out = wx.run("add_rows64", [_acc_slots(b) for b in big])
    for i in range(n):
        tot = [sum(big[i][16 * r + j] for r in range(4)) for j in range(16)]
        for lane in range(64):
            got = (int(out[i, 0, lane]) & 0xffffffff) | (int(out[i, 1, lane]) << 32)
            assert got == tot[lane % 16], ("add_rows_u64", i, lane)


# ---- conversions -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_conversions(wx):
    """fw_to_fe of each row, fw_to_fe_own_row and the zero tests, up to the
    precondition pinned in wide_vectors (negative limbs to -4 p_k); the two
    routines agree, every lane holds the same words, and zero is reported
    exactly for the representations of zero"""
    xs = vectors("to_fe") + W.zero_vectors(W.TO_FE_NEG_TOP, 2)
    nz = sum(W.value(x) == 0 for x in xs)
    assert nz >= 16
    xs += [xs[-1]] * (-len(xs) % 4)
    n = len(xs) // 4
    waves = [[xs[w + n * r] for r in range(4)] for w in range(n)]
    out = wx.run("to_fe", [{0: rows4(*wv)} for wv in waves])
    bad = []
    for i, wv in enumerate(waves):
        flags = 0
        for r, x in enumerate(wv):
            want = V.words(W.value(x))
            flags |= (W.value(x) == 0) << r
            if [int(v) & 0xffffffff for v in out[i, r]] != want * 8:
                bad.append(("fw_to_fe", r, x))
            if [int(v) & 0xffffffff for v in out[i, 4, 16 * r:16 * r + 16]] != want * 2:
                bad.append(("own_row", r, x))
            if any(int(v) != int(W.value(x) == 0) for v in out[i, 6, 16 * r:16 * r + 16]):
                bad.append(("own_row zero", r, x))
        if any(int(v) != flags for v in out[i, 5]):
            bad.append(("fw_row_iszero", wv))
    no_mismatch(bad)
    vals = V.field_values()[:64]
    out = wx.run("fe_to_fw", [{0: uwords(v)} for v in vals])
    no_mismatch([hex(v) for i, v in enumerate(vals)
                 if any(row(out, i, 0, r) != W.canon((v & V.M255) % P) for r in range(4))])


# ---- powers ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pow_inputs():
    """at the carried bound, negative limbs included; zero in several forms"""
    return W.directed(W.CARRIED, 0x9077, 24) + W.zero_vectors(W.CARRIED, 3, 4)


@pytest.mark.gpu
def test_powers(wx):
    xs = _pow_inputs()
    bad = []
    for name, e in (("pow", 2 ** 252 - 3), ("inv", P - 2), ("inv_sel", P - 2)):
        out = wx.run(name, [{0: rep(x)} for x in xs])
        for i, x in enumerate(xs):
            got = [row(out, i, 0, r) for r in range(4)]
            if any(W.value(g) != pow(W.value(x), e, P) for g in got) or any(g != got[0] for g in got) or \
                    not cap_ok(got[0], W.CARRIED):
                bad.append((name, x))
    ys = xs + [xs[-1]] * (-len(xs) % 4)
    n = len(ys) // 4
    waves = [[ys[w + n * r] for r in range(4)] for w in range(n)]
    out = wx.run("pow_rows", [{0: rows4(*wv)} for wv in waves])
    for i, wv in enumerate(waves):
        for r, x in enumerate(wv):
            got = row(out, i, 0, r)
            if W.value(got) != pow(W.value(x), 2 ** 252 - 3, P) or not cap_ok(got, W.CARRY2_CAP):
                bad.append(("pow_rows", r, x))
    no_mismatch(bad)


# ---- points ----------------------------------------------------------------------------------
def pw_limbs(pt, rng, z=1, bound=None):
    """(x, y) as the four slots X, Y, Z, T of a wave-wide point with Z = z,
    re-spread to the carried bound"""
    x, y = pt
    co = [x * z % P, y * z % P, z % P, x * y * z % P]
    return [rep(W.respread(W.canon(c), bound or W.CARRIED, rng)) if rng is not None else rep(W.canon(c))
            for c in co]


def pw_slots(pt, rng, at=0, z=1):
    return {at + k: l for k, l in enumerate(pw_limbs(pt, rng, z))}


def pw_out(out, i, at=0, cap=W.CARRY2_CAP):
    """(affine point, consistent) of the point at slots at..at+3: the four rows
    identical, limbs within the cap, X Y = Z T"""
    co = [[row(out, i, at + k, r) for r in range(4)] for k in range(4)]
    ok = all(c[r] == c[0] for c in co for r in range(4)) and all(cap_ok(c[0], cap) for c in co)
    X, Y, Z, T = (W.value(c[0]) for c in co)
    ok = ok and X * Y % P == Z * T % P and Z != 0
    zi = pow(Z, P - 2, P)
    return (X * zi % P, Y * zi % P), ok


def enc_out(out, i, slot):
    """the encoding every lane holds (lane & 7 picks the word): all eight copies alike"""
    w = [int(v) & 0xffffffff for v in out[i, slot]]
    assert w == w[:8] * 8, "lanes disagree on an encoding"
    return np.asarray(w[:8], "<u4").tobytes()


@functools.lru_cache(maxsize=None)
def _pts():
    return [pt for pt, _ in V.chain_points()]


@pytest.mark.gpu
def test_point_operations(wx):
    """pw_dbl, pw_add (both signs), pw_cached, pw_add_p3 and the record round
    trip against exact affine arithmetic: prime-order, order-8, mixed-order
    points and the identity, doubling the identity, P + (-P), coordinates
    re-spread with Z != 1"""
    rng = np.random.default_rng(0x9017)
    pts = _pts()
    out = wx.run("dbl", [pw_slots(p, rng, z=3 + i) for i, p in enumerate(pts)])
    bad = []
    for i, p in enumerate(pts):
        got, ok = pw_out(out, i)
        if not ok or got != E.add(p, p):
            bad.append(("dbl", p))
    prs = [(p, q) for p in pts for q in pts[:4] + pts[-2:]] + [(p, V.neg(p)) for p in pts]
    recs = [{**pw_slots(p, rng, 0, z=2 + i), **pw_slots(q, rng, 4, z=5 + i)} for i, (p, q) in enumerate(prs)]
    out = wx.run("add", recs)
    out3 = wx.run("add_p3", recs)
    for i, (p, q) in enumerate(prs):
        (s, ok1), (d, ok2), (s3, ok3) = pw_out(out, i, 0), pw_out(out, i, 4), pw_out(out3, i, 0)
        if not (ok1 and ok2 and ok3) or s != E.add(p, q) or d != E.add(p, V.neg(q)) or s3 != s:
            bad.append(("add", p, q))
        # the cached operands: rows Y - X, Y + X, 2d T, 2 Z of Q (rows 0/1 swapped
        # and row 2 negated for -Q), projectively
        for slot, sign in ((8, 1), (9, -1)):
            r = [W.value(row(out, i, slot, k)) for k in range(4)]
            if sign < 0:
                r = [r[1], r[0], -r[2] % P, r[3]]
            zi = pow(r[3], P - 2, P) * 2 % P
            x, y = (r[1] - r[0]) * pow(2, P - 2, P) * zi % P, (r[1] + r[0]) * pow(2, P - 2, P) * zi % P
            if (x, y) != q or r[2] * zi % P != 2 * E.D * x * y % P:
                bad.append(("cached", sign, q))
    assert any(E.add(p, q) == V.IDENT for p, q in prs)
    recs = [{k: [int(v) for v in rng.integers(-W.CARRIED, W.CARRIED + 1, 16)] * 4 for k in range(4)}
            for _ in range(8)]
    out = wx.run("st_ld", recs)
    for i, r in enumerate(recs):
        if any([int(v) for v in out[i, k]] != r[k] for k in range(4)):
            bad.append(("st_ld", i))
    no_mismatch(bad)


@pytest.mark.gpu
def test_table_digits(wx):
    """tab_build + tab_pick for every digit -8..8: row by row the cached operand
    of the exact [d]P (digit 0 picks entry 1, as the chain's dead select does);
    an operand is a two-term sum of carried limbs at most (entry 1 is the input's)"""
    rng = np.random.default_rng(0x7ab1)
    pts = _pts()
    out = wx.run("tab", [pw_slots(p, rng, z=7 + i) for i, p in enumerate(pts)])
    half = pow(2, P - 2, P)
    bad = []
    for i, p in enumerate(pts):
        for d in range(-8, 9):
            r = [W.value(row(out, i, d + 8, k)) for k in range(4)]
            if d < 0:
                r = [r[1], r[0], -r[2] % P, r[3]]
            zi = pow(r[3], P - 2, P) * 2 % P
            x, y = (r[1] - r[0]) * half * zi % P, (r[1] + r[0]) * half * zi % P
            if (x, y) != V.smul(abs(d) or 1, p) or r[2] * zi % P != 2 * E.D * x * y % P or \
                    max(abs(v) for k in range(4) for v in row(out, i, d + 8, k)) > 2 * W.CARRIED:
                bad.append((d, p))
    no_mismatch(bad)


@pytest.mark.gpu
def test_identity_test_and_encodings(wx):
    """pw_is_identity on the identity in re-spread, non-canonical form (X a
    representation of 0, Y - Z one of 0, Z != 1) and on everything else;
    encode1_wide and encode2_wide against the exact encodings"""
    rng = np.random.default_rng(0x1d17)
    zs = W.zero_vectors(W.CARRIED, 5, 8)
    recs, want = [], []
    for i, z0 in enumerate(zs):                   # X = z0, Y = Z + (a zero), T = another zero
        zl = W.respread(W.canon(3 + 5 * i), W.CARRIED, rng)
        z1 = W.zero_vectors(W.CARRIED, 6 + i, 2)[-1]
        recs.append({0: rep(z0), 1: rep([a + b for a, b in zip(zl, z1)]), 2: rep(zl), 3: rep(zs[-1 - i])})
        want.append(1)
    for i, p in enumerate(_pts()):
        recs.append(pw_slots(p, rng, z=11 + i))
        want.append(int(p == V.IDENT))
    recs.append(pw_slots((0, P - 1), rng, z=9))   # (0, -1): X = 0 but Y = -Z
    want.append(0)
    out = wx.run("is_id", recs)
    no_mismatch([i for i, w in enumerate(want) if any(int(v) != w for v in out[i, 0])])
    pts = _pts()
    prs = [(p, pts[(3 * i + 1) % len(pts)]) for i, p in enumerate(pts)]
    out = wx.run("enc", [{**pw_slots(h, rng, 0, z=2 + i), **pw_slots(v, rng, 4, z=13 + i)}
                         for i, (h, v) in enumerate(prs)])
    bad = []
    for i, (h, v) in enumerate(prs):
        got = [enc_out(out, i, k) for k in range(4)]
        if got != [E.enc_pt(h), E.enc_pt(v), E.enc_pt(h), E.enc_pt(v)]:
            bad.append((h, v))
    no_mismatch(bad)


# ---- decode ----------------------------------------------------------------------------------
def _dec_fields(out, i, at):
    ok = [int(v) for v in out[i, at]]
    assert ok == [ok[0]] * 64
    co = []
    for k in range(1, 5):
        w = [int(v) & 0xffffffff for v in out[i, at + k]]
        assert w == w[:8] * 8
        co.append(V.unwords(w[:8]))
    return ok[0], co


@pytest.mark.gpu
@pytest.mark.parametrize("negate", [False, True])
def test_decode(wx, negate):
    """ge_decode_wide and ge_decode_pair_wide (two different inputs; swapping
    them swaps the results) against libsodium's reading"""
    ins = V.decode_inputs()
    out = wx.run("decode", [{0: V.bwords(b) + [int(negate)]} for b in ins])
    other = [ins[(5 * i + 2) % len(ins)] for i in range(len(ins))]
    pair = wx.run("decode_pair", [{0: V.bwords(a) + V.bwords(b) + [int(negate)]} for a, b in zip(ins, other)])
    swap = wx.run("decode_pair", [{0: V.bwords(b) + V.bwords(a) + [int(negate)]} for a, b in zip(ins, other)])
    bad = []

    def check(tag, got, b):
        ok, _, _, x, y = V.decode_want(b, negate)
        flag, (X, Y, Z, T) = got
        if flag != int(ok) or (ok and ((X, Y, Z) != (x, y, 1) or T != x * y % P)):
            bad.append((tag, b.hex()))

    for i, (a, b) in enumerate(zip(ins, other)):
        check("one", _dec_fields(out, i, 0), a)
        check("pair a", _dec_fields(pair, i, 0), a)
        check("pair b", _dec_fields(pair, i, 5), b)
        if _dec_fields(swap, i, 0) != _dec_fields(pair, i, 5) or _dec_fields(swap, i, 5) != _dec_fields(pair, i, 0):
            bad.append(("swap", a.hex(), b.hex()))
    no_mismatch(bad)


# ---- chains ----------------------------------------------------------------------------------
def recode16(b):
    """b's sixteen signed 16-bit digits (sc_recode_carries<16, 16>)"""
    d, c = [], 0
    for k in range(16):
        t = ((b >> (16 * k)) & 0xffff) + c
        c = 1 if t > 0x8000 else 0
        d.append(t - (c << 16 if k < 15 else 0))
    assert sum(x << (16 * k) for k, x in enumerate(d)) == b
    return d


def b_part(b, mask):
    d = recode16(b)
    return sum(d[k] << (16 * k) for k in range(16) if (mask >> (k // 8)) & 1)


def scal_slot(a1=0, a2=0, b=0, w24=0, w25=0):
    return uwords(a1) + uwords(a2) + uwords(b) + [w24, w25]


def chain_scalars():
    m = (1 << 253) - 1
    rng = np.random.default_rng(0xc4a2)
    c128 = [V.rep_digits(d, 4, 32) for d in (8, 7, 15)] + [V.rep_digits(d, 4, 33) for d in (8, 7, 15)]
    return list(dict.fromkeys(
        c128 + V.s_directed() + V.b_directed() + [0, 1, L - 1] +
        [V.rep_digits(9, 4, 63), (V.rep_digits(15, 4, 47) | 9) & m, 2 ** 192 - 1, 2 ** 196 - 1] +
        [int.from_bytes(rng.bytes(32), "little") & m for _ in range(6)]))


VARIANTS = {"dsm": (False, 0), "dsm_t2": (True, 0), "dsm_b1": (False, 1), "dsm_b2": (False, 2),
            "dsm_b": (False, 3), "dsm_t2b": (True, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_chains(wx, variant):
    """every pw_dsm instantiation wide_cores.h makes, the window counts as
    parameters: the exact [a1 windows below nw1]T1 + [a2 windows below nw2]T2 +
    [b's digits of the mask]B, digits from the Python recoding"""
    t2, mask = VARIANTS[variant]
    rng = np.random.default_rng(0xc4a3 + len(variant) + mask)
    pts, sc = _pts(), chain_scalars()
    nws = [1, 32, 33, wx.vwin, 64]
    cases = []
    for i, a1 in enumerate(sc):
        for nw1 in (nws if i < 6 else [nws[i % 5], nws[(i + 2) % 5]]):
            a2 = sc[(3 * i + 1) % len(sc)] if t2 else 0
            b = sc[(5 * i + 2) % len(sc)] if mask else 0
            nw2 = nws[(i + nw1) % 5] if t2 else 0
            cases.append((pts[(i + nw1) % len(pts)], pts[(2 * i + 3) % len(pts)], a1, nw1, a2, nw2, b))
    recs = [{**pw_slots(T1, rng, 0, z=2 + i), **pw_slots(T2, rng, 4, z=3 + i),
             8: scal_slot(a1, a2, b, nw1, nw2)} for i, (T1, T2, a1, nw1, a2, nw2, b) in enumerate(cases)]
    out = wx.run(variant, recs)
    bad = []
    for i, (T1, T2, a1, nw1, a2, nw2, b) in enumerate(cases):
        want = V.lincomb([(W.window_sum(a1, 0, nw1), T1), (W.window_sum(a2, 0, nw2), T2),
                          (b_part(b, mask), E.BASE)])
        got, ok = pw_out(out, i)
        if not ok or got != want or enc_out(out, i, 4) != E.enc_pt(want):
            bad.append((hex(a1), nw1, hex(a2), nw2, hex(b)))
    no_mismatch(bad)


# ---- split sums ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ed_halves_sum_to_the_whole(wx):
    """eds_chain's two chains: [h windows 0..31](-A) + [S digits 0..7]B and
    [sc_high_half_with_carry(h)](2^128 (-A)) + [S digits 8..15](2^128 B) sum to
    the exact [h](-A) + [S]B"""
    rng = np.random.default_rng(0xed51)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % L  # noqa: E731
    pts = _pts()
    Ss = [0x8000 << 112, 0x8001 << 112, 0xffff << 112, 2 ** 128 - 1, 2 ** 128,
          V.rep_digits(0x8000, 16, 16) & (2 ** 252 - 1), L - 1, 0] + [rnd() for _ in range(4)]
    hs = [8 << 124, 15 << 124, 9 << 120 | 8 << 124, V.rep_digits(15, 4, 32), V.rep_digits(8, 4, 63),
          2 ** 128 - 1, 2 ** 128, L - 1, 0, 1] + [rnd() for _ in range(4)]
    cases = [(pts[(i + j) % len(pts)], h, S) for i, h in enumerate(hs) for j, S in enumerate(Ss)
             if i < 3 or j < 3 or (i + j) % 4 == 0]
    lo = wx.run("ed_half", [{**pw_slots(V.neg(A), rng, 0, z=2 + i), 8: scal_slot(h, S, 0, 0)}
                            for i, (A, h, S) in enumerate(cases)])
    hi = wx.run("ed_half", [{**pw_slots(V.neg(A), rng, 0, z=3 + i), 8: scal_slot(h, S, 0, 1)}
                            for i, (A, h, S) in enumerate(cases)])
    bad = []
    for i, (A, h, S) in enumerate(cases):
        (x, ok1), (y, ok2) = pw_out(lo, i), pw_out(hi, i)
        if not (ok1 and ok2) or E.add(x, y) != V.lincomb([(-h, A), (S, E.BASE)]) or \
                x != V.lincomb([(-W.window_sum(h, 0, 32), A), (b_part(S, 1), E.BASE)]):
            bad.append((hex(h), hex(S)))
    no_mismatch(bad)


@pytest.mark.gpu
def test_v_parts_sum_to_the_whole(wx):
    """vrf_sh_split's parts from a given H: windows 0..K-1, sc_high_from_window<K>
    over 2^(4K) H (and the third part with OURO_LAT_V3) sum to the exact [s]H"""
    rng = np.random.default_rng(0x5b51)
    pts = _pts()
    ss = [s for s in W.split_scalars(wx.vwin) if s < 2 ** 253]
    parts = 3 if wx.v3 else 2
    cases = [(pts[i % len(pts)], s) for i, s in enumerate(ss)]
    outs = [wx.run("v_part", [{**pw_slots(H, rng, 0, z=2 + i + k), 8: scal_slot(s, 0, 0, k)}
                              for i, (H, s) in enumerate(cases)]) for k in range(parts)]
    bad = []
    for i, (H, s) in enumerate(cases):
        acc, ok = V.IDENT, True
        for o in outs:
            pt, k = pw_out(o, i)
            acc, ok = E.add(acc, pt), ok and k
        first, _ = pw_out(outs[0], i)
        if not ok or acc != V.smul(s, H) or first != V.lincomb([(W.window_sum(s, 0, wx.vwin), H)]):
            bad.append(hex(s))
    no_mismatch(bad)


# ---- Blake2b on the quads ----------------------------------------------------------------------
@pytest.mark.gpu
def test_blake2b_short_quad(wx):
    rng = np.random.default_rng(0xb2b4)
    msgs = [bytes(64), b"\xff" * 64] + [rng.bytes(64) for _ in range(6)]
    cases = [(m[:n] + bytes(64 - n), n) for m in msgs for n in (0, 1, 8, 39, 40, 41, 63, 64)]
    out = wx.run("blake", [{0: V.bwords(m) + [n]} for m, n in cases])
    bad = []
    for i, (m, n) in enumerate(cases):
        want = list(np.frombuffer(hashlib.blake2b(m[:n], digest_size=32).digest(), "<u4"))
        if any([int(out[i, k, lane]) & 0xffffffff for k in range(8)] != want for lane in range(64)):
            bad.append((n, m.hex()))
    no_mismatch(bad)
