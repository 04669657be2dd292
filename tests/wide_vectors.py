"""Vectors, documented bounds and an exact integer model of the latency mode's
wave-wide field arithmetic (csrc/wide.h, wide_cores.h), for
tests/test_wide_exact.py.

A wave-wide element is 16 signed limbs, radix 2^16 (2^256 = 38 mod p).  The
model follows the limb flow of the routines -- the rotation, the factor 38
where a limb wraps, the shifts -- on Python integers, and asserts what the
device code silently assumes: every argument of an s24() inside the signed
24-bit range, every 32-bit intermediate in range, the accumulators under the
caps the comments state, fw_to_fe's final carry non-negative.  A vector that
passes the model is legal for the routine it is fed to, so a mismatch on the
device is the code's or the documented bound's, never the vector's; for the
carry forms the model also gives the expected limbs."""
import numpy as np

import lane_vectors as V

P, L = V.P, V.L
NL = 16
P_LIMBS = [0xffed] + [0xffff] * 14 + [0x7fff]

# ---- the bounds the headers document ---------------------------------------------
# wide.h, header: "a carried element has |limb| <= 65,535 + 38*16 < 2^16.01"
# (fw_carry, the three-round form: "into limbs |l| < 2^16.01")
CARRY3_CAP = 65535 + 38 * 16
# wide.h fw_carry2: "one shift-and-rotate round leaves it below ... < 2^16.03"
CARRY2_CAP = int(2 ** 16.03)
# wide.h fw_carry_rows: "limbs below 2^16 + 38 * 2^7.4 < 2^16.13"
ROWS_CAP = int(2 ** 16.13)
# wide_cores.h fw_norm: "one carry round of a limb vector below 2^20: limbs
# below 2^16 + 38 * 16"
NORM_IN = 2 ** 20 - 1
NORM_CAP = 65535 + 38 * 16
# the largest carried limb of any form: what a coordinate or a chain value holds
CARRIED = max(CARRY3_CAP, CARRY2_CAP, ROWS_CAP, NORM_CAP)
# wide.h, header: the rotated operand passes v_mul_i32_i24 after it wrapped,
# "so |38 g| < 2^23": the narrow operand's limit
NARROW = (2 ** 23 - 1) // 38
# wide.h, header: the narrow operand is "<= 3 carried elements summed", "the
# broadcast operand f ... takes the 4-term sums"; fw_carry_rows: "3 of them sum
# below 220,752, the narrow operand's limit"
THREE_TERM = 3 * CARRIED
FOUR_TERM = 4 * CARRIED
assert NARROW == 220752 and THREE_TERM <= NARROW
# wide.h fw_carry: "carry an accumulator (|acc| < 2^46)"; header: a product's
# accumulator is "< 2^45.1"
ACC_CAP = 2 ** 46
MUL_ACC_CAP = int(2 ** 45.1)
# wide.h fw_carry_rows: each row's partial accumulator, "four steps: |acc_r| <
# 2^43.2" (4 * FOUR_TERM * 38 * NARROW = 2^43.13; the comment said 2^43.1 until
# test_wide_exact.py test_documented_bounds_hold_under_the_model refuted it)
ROW_ACC_CAP = int(2 ** 43.2)
# wide.h fw_to_fe: 4p is added first, so limb k may be as negative as 4 p_k:
# 4 * 0xffed at limb 0, 4 * 0xffff at limbs 1..14, but only 4 * 0x7fff at limb 15
# (the comment said "below 2^17" for every limb; limbs 14 and 15 at -(2^17 - 1)
# leave a negative final carry)
TO_FE_NEG = [4 * pk for pk in P_LIMBS]
TO_FE_NEG_LOW = min(TO_FE_NEG[:15])   # 262,068: any of limbs 0..14
TO_FE_NEG_TOP = TO_FE_NEG[15]         # 131,068: limb 15
# Limb 15 of a carried element: its carry-in is never multiplied by 38, so it
# stays within [-16, 65,535 + 15] in every form (fw_norm's input below 2^20
# hands limb 15 at most 15 and at least -16; the other forms less), and a
# two-term difference of carried elements is within fw_to_fe's limb-15 bound
LIMB15_MAX, LIMB15_MIN = 65535 + 15, -16
assert 2 * CARRIED <= TO_FE_NEG_LOW and LIMB15_MAX - LIMB15_MIN <= TO_FE_NEG_TOP


class Illegal(AssertionError):
    """an input outside what the routine's arithmetic can hold"""


def _need(ok, what):
    if not ok:
        raise Illegal(what)


def s24(x, what):
    _need(-2 ** 23 <= x < 2 ** 23, "s24 argument out of range: " + what)
    return x


def i32(x, what):
    _need(-2 ** 31 <= x < 2 ** 31, "32-bit intermediate out of range: " + what)
    return x


def value(limbs):
    return sum(int(l) << (16 * k) for k, l in enumerate(limbs)) % P


def canon(x):
    """the canonical limbs of x mod p"""
    x %= P
    return [(x >> (16 * k)) & 0xffff for k in range(NL)]


def ror(v, n=1):
    """DPP row_ror:n -- lane j takes lane j - n"""
    return [v[(j - n) % NL] for j in range(NL)]


def fac_at(j, n=1):
    """38 where a rotation by n lanes wrapped (fac, fac2, facr of wide.h lanes())"""
    return 38 if j < n else 1


# ---- the model -----------------------------------------------------------------------
def _rot_step(G):
    """G = s24(ror1(G)) * s24(fac)"""
    r = ror(G)
    return [i32(s24(r[j], "rotated narrow operand (38 g after the wrap)") * fac_at(j), "38 g")
            for j in range(NL)]


def fw_mul_acc(f, g):
    """wide.h fw_mul_steps: the sixteen-step accumulator of one row"""
    G = list(g)
    acc = [0] * NL
    for i in range(NL):
        if i:
            G = _rot_step(G)
        fi = i32(f[i], "broadcast operand")
        for j in range(NL):
            i32(G[j], "narrow operand")
            acc[j] += fi * G[j]
    for a in acc:
        _need(abs(a) < MUL_ACC_CAP, "fw_mul accumulator beyond 2^45.1 (wide.h header)")
    return acc


def fw_carry3(acc):
    """wide.h fw_carry (three rounds)"""
    for a in acc:
        _need(abs(a) < ACC_CAP, "accumulator beyond 2^46 (wide.h fw_carry)")
    lo = [a & 0xffff for a in acc]
    hi = [i32(a >> 16, "acc >> 16") for a in acc]
    r = ror(hi)
    t = [r[j] * fac_at(j) + lo[j] for j in range(NL)]
    lo = [x & 0xffff for x in t]
    hi = [i32(x >> 16, "round 1 carry") for x in t]
    r = ror(hi)
    u = [i32(s24(r[j], "fw_carry round 2") * fac_at(j) + lo[j], "round 2 sum") for j in range(NL)]
    lo = [x & 0xffff for x in u]
    r = ror([x >> 16 for x in u])
    return [s24(r[j], "fw_carry round 3") * fac_at(j) + lo[j] for j in range(NL)]


def _first_round(acc, cap, name):
    """a0 + a1 + a2 of fw_carry2 / fw_carry_rows, one row"""
    for a in acc:
        _need(abs(a) < cap, "accumulator beyond its cap (wide.h %s)" % name)
    lo32 = [a & 0xffffffff for a in acc]
    a0 = [x & 0xffff for x in lo32]
    a1 = ror([x >> 16 for x in lo32], 1)
    a2 = ror([i32(a >> 32, "acc >> 32") for a in acc], 2)
    return [i32(a0[j] + i32(s24(a1[j], name + " a1") * fac_at(j), "38 a1") +
                i32(s24(a2[j], name + " a2") * fac_at(j, 2), "38 a2"), name + " first round")
            for j in range(NL)]


def _last_round(s, name):
    r = ror([x >> 16 for x in s])
    return [(s[j] & 0xffff) + i32(s24(r[j], name + " last round") * fac_at(j), "38 carry")
            for j in range(NL)]


def fw_carry2(acc):
    return _last_round(_first_round(acc, ACC_CAP, "fw_carry2"), "fw_carry2")


def fw_carry_rows(accs):
    """wide.h fw_carry_rows: four rows' accumulators -> the one replicated element"""
    assert len(accs) == 4
    sr = [_first_round(a, ROW_ACC_CAP, "fw_carry_rows") for a in accs]
    s = [i32(i32(sr[0][j] + sr[1][j], "row sum") + i32(sr[2][j] + sr[3][j], "row sum"), "rows' sum")
         for j in range(NL)]
    return _last_round(s, "fw_carry_rows")


def fw_norm(x):
    """wide_cores.h fw_norm"""
    for v in x:
        _need(abs(v) <= NORM_IN, "fw_norm input beyond 2^20 (wide_cores.h)")
    return _last_round(list(x), "fw_norm")


def fw_mul(f, g):
    return fw_carry2(fw_mul_acc(f, g))


def rep_accs(f, g):
    """wide.h fw_mul_rep: row r takes steps 4r..4r+3, its operands rotated by 4r
    lanes; the four rows' accumulators"""
    accs = []
    for r in range(4):
        fr = [i32(f[(k + 4 * r) % NL], "broadcast operand") for k in range(NL)]
        rg = ror([s24(v, "narrow operand") for v in g], 4 * r)
        G = [i32(rg[j] * fac_at(j, 4 * r), "38 g") for j in range(NL)]
        acc = [0] * NL
        for i in range(4):
            if i:
                G = _rot_step(G)
            for j in range(NL):
                acc[j] += fr[i] * G[j]
        accs.append(acc)
    return accs


def fw_mul_rep(f, g):
    return fw_carry_rows(rep_accs(f, g))


def fw_sq_rep(f):
    """wide.h fw_sq_rep: the same flow with g = f (the rotations shared)"""
    return fw_mul_rep(f, f)


def fw_to_fe(x):
    """wide.h fw_to_fe / fw_to_fe_own_row: the canonical value"""
    h, c = [], 0
    for k in range(NL):
        t = i32(i32(x[k], "limb") + 4 * P_LIMBS[k] + c, "fw_to_fe limb + 4p + carry")
        h.append(t & 0xffff)
        c = t >> 16
    _need(c >= 0, "fw_to_fe: negative final carry (wide.h fw_to_fe precondition, limbs 14/15)")
    for _ in range(2):
        cc = c * 38
        _need(cc < 2 ** 32, "fw_to_fe fold")
        for k in range(NL):
            t = h[k] + cc
            _need(t < 2 ** 32, "fw_to_fe fold")
            h[k], cc = t & 0xffff, t >> 16
        c = cc
    _need(c == 0, "fw_to_fe: a carry left after the second fold")
    w = sum(v << (16 * k) for k, v in enumerate(h))
    return ((w & V.M255) + 19 * (w >> 255)) % P


LEGAL = {
    "mul_f": lambda x: fw_mul(x, canon(1)),
    "mul_g": lambda x: fw_mul(canon(1), x),
    "rep_f": lambda x: fw_mul_rep(x, canon(1)),
    "rep_g": lambda x: fw_mul_rep(canon(1), x),
    "sq": lambda x: fw_mul(x, x),
    "sq_rep": fw_sq_rep,
    "norm": fw_norm,
    "to_fe": fw_to_fe,
}


def legal(op, x):
    """whether x alone is inside what `op` can hold"""
    try:
        LEGAL[op](x)
        return True
    except Illegal:
        return False


# ---- directed limb vectors -------------------------------------------------------------
def respread(limbs, bound, rng):
    """the same value with t * 2^16 moved between neighbouring limbs so that
    the limbs fill +-bound (bound >= 2^16)"""
    l = [int(v) for v in limbs]
    for k in range(NL - 1):
        lo = -((bound + l[k]) // 65536)          # l[k] + 65536 t within +-bound
        hi = (bound - l[k]) // 65536
        # ... and the next limb less t within +-bound too
        lo, hi = max(lo, l[k + 1] - bound), min(hi, l[k + 1] + bound)
        t = int(rng.integers(lo, hi + 1)) if lo <= hi else 0
        l[k] += 65536 * t
        l[k + 1] -= t
    assert all(abs(v) <= bound for v in l), (limbs, bound)
    return l


def zeros():
    """representations of zero: canonical, the limbs of p, 2p, -p"""
    p2 = [0xffda] + [0xffff] * 15
    return [[0] * NL, list(P_LIMBS), p2, [-v for v in P_LIMBS]]


CANON_VALUES = [0, 1, P - 1, 2 ** 255 - 20]


def directed(bound, seed, nrand=200):
    """limb vectors within +-bound: every limb at +bound, at -bound, alternating
    signs; one limb at +-bound in each position; the pairs across the rows'
    rotation boundaries 3/4, 7/8, 11/12 (and the wrap 15/0); canonical 0, 1,
    p - 1, 2^255 - 20; the representations of zero and a re-spread p;
    re-spread and plain random vectors"""
    rng = np.random.default_rng(seed)
    out = [[bound] * NL, [-bound] * NL, [bound if k % 2 else -bound for k in range(NL)],
           [-bound if k % 2 else bound for k in range(NL)]]
    for k in range(NL):
        for sgn in (1, -1):
            out.append([sgn * bound if i == k else 0 for i in range(NL)])
    for a, b in ((3, 4), (7, 8), (11, 12), (15, 0), (0, 1)):
        for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            out.append([sa * bound if i == a else sb * bound if i == b else 0 for i in range(NL)])
    out += [canon(v) for v in CANON_VALUES] + zeros()
    out += [respread(z, bound, rng) for z in zeros()[:2] * 2]
    for _ in range(nrand // 2):
        out.append(respread(canon(int.from_bytes(rng.bytes(32), "little")), bound, rng))
    for _ in range(nrand - nrand // 2):
        out.append([int(v) for v in rng.integers(-bound, bound + 1, NL)])
    return out


def zero_vectors(bound, seed, n=12):
    """representations of zero within +-bound (canonical, p, 2p, -p, re-spread)"""
    rng = np.random.default_rng(seed)
    z = zeros()
    return z + [respread(z[i % len(z)], bound, rng) for i in range(n)]


def to_fe_vectors():
    """fw_to_fe's inputs: every positive bound the callers reach, and negative
    limbs down to the precondition pinned above, limb by limb"""
    neg = [-v for v in TO_FE_NEG]
    out = [neg, [-TO_FE_NEG_LOW] * 15 + [-TO_FE_NEG_TOP]]
    for k in range(NL):
        out.append([neg[i] if i == k else 0 for i in range(NL)])
        out.append([neg[i] if i == k else 65535 for i in range(NL)])
    out.append([0] * 14 + [neg[14], neg[15]])
    # limb 15 at its bound over a low limb just past a multiple of 2^16 less 2p's
    # limb 0: with 2p added instead of 4p the final carry is negative and its
    # fold borrows out of limb 0 (a negative carry is only wrong when it borrows)
    for x0 in range(38, 38 + 76, 5):
        out.append([x0] + [0] * 14 + [neg[15]])
        out.append([x0] + [65535, -65535] * 7 + [neg[15]])
    # two-term differences of carried elements (what the callers pass): limbs
    # 0..14 at +-2 CARRIED, limb 15 over its own range
    for s in (1, -1):
        out.append([s * 2 * CARRIED] * 15 + [LIMB15_MIN - LIMB15_MAX if s < 0 else 2 * LIMB15_MAX])
    rng = np.random.default_rng(0x70fe)
    for _ in range(60):
        out.append([int(rng.integers(-TO_FE_NEG[k], FOUR_TERM + 1)) for k in range(NL)])
    out += [[FOUR_TERM] * NL]
    out += directed(TO_FE_NEG_TOP, 0x70ff, 60) + directed(TO_FE_NEG_LOW, 0x7100, 40)
    # directed() puts -bound at limb 15 too: only within limb 15's own bound
    return [v for v in out if v[15] >= -TO_FE_NEG_TOP]


def acc_vectors(cap, seed, n=120):
    """accumulators within +-(cap - 1): the ends, one lane at an end in each
    position, 16-bit and 32-bit boundary patterns, random"""
    rng = np.random.default_rng(seed)
    m = cap - 1
    out = [[m] * NL, [-m] * NL, [m if k % 2 else -m for k in range(NL)], [0] * NL,
           [0xffffffff] * NL, [-0x100000000] * NL, [0xffff] * NL, [-1] * NL, [0x10000] * NL]
    for k in range(NL):
        for v in (m, -m):
            out.append([v if i == k else 0 for i in range(NL)])
    for _ in range(n):
        out.append([int(rng.integers(-m, m + 1)) for _ in range(NL)])
    return out


# ---- the signed width-4 recoding (csrc/sc25519.h) ----------------------------------------
def recode4(s):
    """(digits d_0..d_63, carry mask) as sc_recode_carries<4, 64> and
    sc_digit_from<4> define them: c_0 = 0, t_j = bits_j + c_j,
    c_{j+1} = (t_j > 8), d_j = t_j - 16 c_{j+1}; the last window keeps its carry"""
    assert 0 <= s < 2 ** 256
    d, mask, c = [], 0, 0
    for j in range(64):
        mask |= c << j
        t = ((s >> (4 * j)) & 15) + c
        c = 1 if t > 8 else 0
        d.append(t - (16 * c if j < 63 else 0))
    return d, mask


def window_sum(s, lo, hi):
    """sum of s's recoded digits lo..hi-1, each at its weight: what a chain
    that is given only those windows of s adds up (the top one of them keeps
    the carry it hands on, as pw_dsm does: its digit is formed with the mask)"""
    d, _ = recode4(s)
    return sum(d[j] << (4 * j) for j in range(lo, hi))


def split_scalars(K):
    """s < 2^253 for the cut at window K: window K - 1 exactly 8, 7 and 15 (a
    carry out, none, one only with a carry in), windows K..K+7 (and K..K+15) all
    0xf with a carry coming in (the add ripples through one, two 32-bit words),
    0, 16^K - 1, 16^K, L - 1, 2^253 - 1, and lane_vectors.s_directed()"""
    m = (1 << 253) - 1
    w = lambda j, v: v << (4 * j)  # noqa: E731
    out = [0, (1 << (4 * K)) - 1, 1 << (4 * K), L - 1, m]
    for top in (8, 7, 15):
        out += [w(K - 1, top), w(K - 1, top) | w(K - 2, 9) if K > 1 else 0,
                (w(K - 1, top) | w(K, 5) | (V.rep_digits(9, 4, K - 1))) & m]
    for n in (8, 16, 64):
        ones = V.rep_digits(15, 4, n) << (4 * K)
        out += [(ones | w(K - 1, 9)) & m, (ones | w(K - 1, 8) | w(K - 2, 9)) & m if K > 1 else 0,
                (ones | w(K - 1, 8)) & m]
    out += V.s_directed()
    rng = np.random.default_rng(0x5917 + K)
    out += [int.from_bytes(rng.bytes(32), "little") & m for _ in range(40)]
    out += [int.from_bytes(rng.bytes(40), "little") % L for _ in range(20)]
    return list(dict.fromkeys(out))
