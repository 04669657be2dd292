"""Vectors and exact references for the lane routines (tests/test_lane_exact.py),
shared by the host and the device backend, and the directed generators the
host tests (test_devcode_host.py, test_vrfkey_tables.py) use.  Python integers
only: field and scalar values by `%`, points by the complete twisted-Edwards
addition on exact integers, hashes by hashlib.  Fixed seeds; sizes are the
smallest that still reach the edges."""
import hashlib

import numpy as np

import edge_cases as E

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
M255 = 2**255 - 1
# the limb exponents of csrc/fe25519.h: limb i weighs 2^ceil(25.5 i)
LIMB_E = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
LIMB_MASK = [(1 << (26 if i % 2 == 0 else 25)) - 1 for i in range(10)]

# ---- generators shared with the host tests ------------------------------------
# test_devcode_host.py test_field_ops / test_invert_vartime
FIELD_SPECIALS = [0, 1, 2, P - 1, P - 2, 19, 2**255 - 20, 2**254, (P - 1) // 2]
INVERT_SPECIALS = [0, 1, 2, 3, 19, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**254, 2**255 - 20,
                   2**128 - 1, 2**30, 2**30 - 1, 2**240 + 1, 5**100 % P]
# test_table_entry_packing's fixed limb vectors
PACKING_CASES = [[(1 << 28) - 1] * 10, [0] * 10, [(1 << 26) - 1, (1 << 25) - 1] * 5,
                 [1 << 26, 1 << 25] * 5,
                 [(1 << 26) - 19] + [(1 << 25) - 1, (1 << 26) - 1] * 4 + [(1 << 25) - 1]]
# test_scalar_reduce's fixed 64-byte inputs
REDUCE_INPUTS = [b"\xff" * 64, bytes(64), L.to_bytes(64, "little"), (L - 1).to_bytes(64, "little"),
                 (2 * L).to_bytes(64, "little")]
# test_half_scalars_v2_equals_v1's structured h
HALF_HS = [0, 1, 2, 3, 8, L - 1, L - 2, 2**252, 2**253 - 1, 2**128, 2**128 + 1, 2**127,
           (L - 1) // 2, 8 * 3**80 % L, 2**200 + 7, 2**129 - 1, 3 * 2**160 + 5]
# test_vrfkey_tables.py: the order-8 y coordinate (csrc/ge25519.h
# ge_has_small_order) and the keys that fail the key checks
Y8 = int.from_bytes(np.array([0x8f95e826, 0xb027b2c2, 0x89f4c345, 0xf098eff2, 0x05acdfd5,
                              0x3933c6d3, 0x880238b1, 0x05fc536d], np.uint32).tobytes(), "little")
SMALL_ORDER = [(1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little"),
               bytes(32), bytes(31) + b"\x80",
               Y8.to_bytes(32, "little"), (Y8 | 1 << 255).to_bytes(32, "little"),
               (P - Y8).to_bytes(32, "little"), ((P - Y8) | 1 << 255).to_bytes(32, "little")]
NON_CANONICAL = b"\xff" * 31 + b"\x7f"   # y = 2^255 - 1 >= p
NO_DECODE = b"\x02" + bytes(31)          # y = 2: (y^2 - 1) / (d y^2 + 1) is not a square


def directed(width):
    """c where carries ripple, where a digit is exactly +-2^(w-1) or zero, and
    where the top window takes the carry."""
    m = (1 << 128) - 1
    half = 1 << (width - 1)
    rep = lambda d: sum(d << (width * k) for k in range(128 // width + 1)) & m  # noqa: E731
    return [0, 1, m, int.from_bytes(b"\x80" * 16, "little"), int.from_bytes(b"\x7f" * 16, "little"),
            int.from_bytes(b"\x81" * 16, "little"), int.from_bytes(b"\x00\xff" * 8, "little"),
            rep(half), rep(half - 1), rep(half + 1)]


# ---- words ------------------------------------------------------------------------
def words(x, n=8):
    """x as n little-endian 32-bit words"""
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def bwords(b):
    return list(np.frombuffer(b, dtype="<u4"))


def unwords(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def rep_digits(d, width, count):
    return sum(d << (width * k) for k in range(count))


# ---- field ------------------------------------------------------------------------
def limbs_value(l):
    return sum(int(v) << LIMB_E[i] for i, v in enumerate(l))


def single_limb_patterns():
    """every limb at its mask with the others zero, all limbs at their masks,
    and the two limbs a reduced element may hold above their masks at theirs
    (csrc/fe25519.h "Reduced")"""
    out = [[LIMB_MASK[i] if i == k else 0 for i in range(10)] for k in range(10)]
    out.append(list(LIMB_MASK))
    out.append([0, 2**25 + 2**18] + [0] * 8)
    out.append([0] * 6 + [2**26 + 2**12] + [0] * 3)
    return out


def field_values():
    """32-byte inputs as fe_from_words reads them (bit 255 ignored): the host
    tests' specials, the non-canonical p, p + 18 and 2^255 - 1, the limb
    patterns as values, and 300 random ones"""
    rng = np.random.default_rng(0x1a9e)
    vals = list(dict.fromkeys(FIELD_SPECIALS + INVERT_SPECIALS)) + [P, P + 18, M255]
    vals += [limbs_value(l) & M255 for l in single_limb_patterns()]
    vals += [int.from_bytes(rng.bytes(32), "little") & M255 for _ in range(300)]
    return vals


def field_pairs():
    """each value with itself and with a permuted partner"""
    vals = field_values()
    return [(x, x) for x in vals] + [(x, vals[(7 * i + 3) % len(vals)]) for i, x in enumerate(vals)]


RAW_TOPS = [1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 31]
# The tops each raw-limb item runs with: its documented input bound, and for
# fe_mul / fe_sq / fe_carry the tops at which the host bound tracker counts no
# violation over the set (test_raw_limbs asserts that on the host backend).
# fe_mul and fe_sq take the bounds of "Reduced" elements and of their sums:
# from 2^28 the tracker objects (19 g_i no longer fits 32 bits); fe_carry
# takes any 32-bit sum that does not wrap, 2^31 included.
RAW_OP_TOPS = {
    "words": RAW_TOPS, "inv_vt": RAW_TOPS,
    "pack": [1 << 25, 1 << 26, 1 << 27, 1 << 28],
    "mul": [1 << 25, 1 << 26, 1 << 27],
    "sq": [1 << 25, 1 << 26, 1 << 27],
    "carry": RAW_TOPS,
}


def raw_limbs(top):
    """limb vectors below `top`: the fixed cases whose largest limb needs this
    top, then 500 random ones"""
    rng = np.random.default_rng(0x11b5 + top.bit_length())
    need = lambda l: min(t for t in RAW_TOPS if max(l) < t)  # noqa: E731
    out = [l for l in PACKING_CASES + single_limb_patterns() if need(l) == top]
    out += [[int(rng.integers(0, top)) for _ in range(10)] for _ in range(500)]
    return out


def fe_carry_limbs(l):
    """csrc/fe25519.h fe_carry: one sequential 32-bit pass, the carry out of
    limb 9 wrapped into limb 0 (x 19) without a second pass"""
    out, c = [], 0
    for i in range(10):
        t = l[i] + c
        assert t < 2**32
        c = t >> (26 if i % 2 == 0 else 25)
        out.append(t & LIMB_MASK[i])
    out[0] += 19 * c
    return out


# ---- scalars ------------------------------------------------------------------------
def reduce512_inputs():
    rng = np.random.default_rng(0x5c01)
    fixed = REDUCE_INPUTS + [(L << 256).to_bytes(64, "little"), (2**252).to_bytes(64, "little")]
    return fixed + [rng.bytes(64) for _ in range(200)]


def reduce256_inputs():
    rng = np.random.default_rng(0x5c02)
    fixed = [0, 1, L - 1, L, L + 1, 2 * L, 2**252, 2**256 - 1, 15 * L, 2**256 - L]
    return fixed + [int.from_bytes(rng.bytes(32), "little") for _ in range(200)]


def half_inputs():
    """h < 2^253: the structured values, 2,000 uniform and 2,000 below L"""
    rng = np.random.default_rng(0x4a1f)
    hs = list(HALF_HS)
    hs += [int.from_bytes(rng.bytes(32), "little") >> 3 for _ in range(2000)]
    hs += [int.from_bytes(rng.bytes(64), "little") % L for _ in range(2000)]
    return hs


# ---- SHA-512 --------------------------------------------------------------------------
SHA_LENS = [0, 1, 47, 48, 49, 63, 64, 65, 111, 112, 113, 127, 128, 129, 175, 176, 177, 239, 240,
            241, 544, 1000]
SHA_PAD = 16


def sha_cases():
    """(prefixes, buffer, offsets, lengths, digests): every tail length at
    every start offset 0..7 of a 16-byte-aligned region, 16 bytes of (random)
    padding on both sides of each tail"""
    rng = np.random.default_rng(0x5a51)
    buf = bytearray()
    pre, off, ln, want = [], [], [], []
    for n in SHA_LENS:
        for o in range(8):
            base = len(buf)
            assert base % 16 == 0
            p, m = rng.bytes(64), rng.bytes(n)
            region = rng.bytes(SHA_PAD + o) + m + rng.bytes(SHA_PAD)
            buf += region + bytes(-len(region) % 16)
            pre.append(p)
            off.append(base + SHA_PAD + o)
            ln.append(n)
            want.append(hashlib.sha512(p + m).digest())
    return pre, bytes(buf), off, ln, want


# ---- points ---------------------------------------------------------------------------
IDENT = (0, 1)
D2 = 2 * E.D % P


def _ext_add(p, q):
    # add-2008-hwcd-3 (a = -1): complete on this curve (d is a non-square),
    # torsion points included
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A = (Y1 - X1) * (Y2 - X2) % P
    B = (Y1 + X1) * (Y2 + X2) % P
    C = T1 * D2 % P * T2 % P
    Dd = 2 * Z1 * Z2 % P
    Ee, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (Ee * F % P, G * H % P, F * G % P, Ee * H % P)


def smul(k, pt):
    """[k]pt for k >= 0 in extended coordinates on exact integers; the affine
    result.  (edge_cases.smul inverts twice per addition: seconds per chain.)"""
    acc = (0, 1, 1, 0)
    q = (pt[0], pt[1], 1, pt[0] * pt[1] % P)
    while k:
        if k & 1:
            acc = _ext_add(acc, q)
        q = _ext_add(q, q)
        k >>= 1
    zi = pow(acc[2], P - 2, P)
    return (acc[0] * zi % P, acc[1] * zi % P)


def neg(pt):
    return ((-pt[0]) % P, pt[1])


def lincomb(terms):
    """sum of [k]pt over (k, pt), k any integer"""
    acc = IDENT
    for k, pt in terms:
        acc = E.add(acc, smul(k, pt) if k >= 0 else neg(smul(-k, pt)))
    return acc


def chain_points():
    """(point, discrete log to BASE or None): BASE, the identity, an order-8
    point, -BASE, four random prime-order points, two of mixed order"""
    rng = np.random.default_rng(0xc4a1)
    pts = [(E.BASE, 1), (IDENT, 0), (E.T8, None), (neg(E.BASE), L - 1)]
    for _ in range(4):
        k = int.from_bytes(rng.bytes(40), "little") % L
        pts.append((smul(k, E.BASE), k))
    pts.append((E.add(pts[4][0], E.T8), None))
    pts.append((E.add(E.BASE, smul(3, E.T8)), None))
    return pts


# ---- decode / Elligator2 -------------------------------------------------------------
def decode_inputs():
    rng = np.random.default_rng(0xdec0)
    enc = list(E.small_order_encodings())
    enc += [E.enc_int(2), E.enc_int(2, 1), E.enc_int(E.non_square_y()), E.enc_int(E.non_square_y(), 1)]
    enc += [E.enc_int(y, s) for y in (P - 1, P, P + 1, M255) for s in (0, 1)]
    enc += [E.enc_int(1, 1)]                       # x = 0 with the sign bit set
    enc += [E.enc_pt(pt) for pt, _ in chain_points()]
    enc += [rng.bytes(32) for _ in range(100)]     # about half of them do not decode
    return list(dict.fromkeys(enc))


def decode_want(b, negate):
    """(ok, canonical, small order, x, y) as libsodium 1.0.18 reads b"""
    y_raw = int.from_bytes(b, "little") & M255
    sign = b[31] >> 7
    x = E.recover_x(y_raw % P, sign)
    if x is not None and negate:
        x = (-x) % P
    return (x is not None, y_raw < P, y_raw in E.SMALL_Y, x, y_raw % P)


def elligator_inputs():
    """test_gpu_wide.py test_wide_elligator2_matches_oracle's values"""
    vals = [0, 1, 2, 3, 4, 5, P - 1, P, P + 1, P + 7, M255]
    rs = [v.to_bytes(32, "little") for v in vals]
    rng = np.random.default_rng(11)
    for _ in range(245):
        r = bytearray(rng.bytes(32))
        r[31] &= 0x7F
        rs.append(bytes(r))
    return rs


# ---- the chains ------------------------------------------------------------------------
def b_directed():
    """b < 2^253 with every 16-bit digit at, just below and far above half the
    window (the top digit cut to the scalar's range), and around the split of
    the fixed-base multiplication at bit 128"""
    m = (1 << 253) - 1
    return [0, 1, L - 1, 2**128 - 1, 2**128, 2**128 + 1] + \
        [rep_digits(d, 16, 16) & m for d in (0x8000, 0x7fff, 0xffff)]


def short_pair(h):
    """(c0, c1) with c0 = c1 h (mod 8L), c1 odd and positive, both about half
    size: Euclid on (8L, h) down to the first remainder below 2^127, taking a
    neighbouring row when that one's cofactor is even"""
    r0, r1, t0, t1 = 8 * L, h % (8 * L), 0, 1
    while r1 >= 2**127:
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    c0, c1 = (r1, t1) if t1 % 2 else (r0 + r1, t0 + t1) if (t0 + t1) % 2 else (r0, t0)
    if c1 < 0:
        c0, c1 = -c0, -c1
    assert c1 % 2 == 1 and c1 > 0 and (c0 - c1 * h) % (8 * L) == 0
    return c0, c1


def ed_cases():
    """96 x (A, R, c0, c1, b, bits), c0 signed: the chain must give
    [b]B - [c0]A - [c1]R.  Ordered so that a packed wave mixes bits = 253,
    bits near 128 and bits = 1."""
    rng = np.random.default_rng(0xed25)
    pts = chain_points()
    rnd = lambda n: int.from_bytes(rng.bytes(n), "little")  # noqa: E731
    pick = lambda: pts[int(rng.integers(0, len(pts)))][0]  # noqa: E731
    bd = b_directed()
    mid, big, tiny = [], [], []
    # real signatures: A = [a]B, R = [r]B, S = r + h a, and b = c1 S: the
    # chain's result is the identity
    for k in range(12):
        (A, a), (R, r) = pts[4 + k % 4], pts[4 + (k + 1) % 4]
        h = rnd(64) % L
        c0, c1 = short_pair(h)
        mid.append((A, R, c0, c1, c1 * ((r + h * a) % L) % L))
    # the same relation over any points, b random, directed or wrong
    for k in range(28):
        h = rnd(64) % L
        c0, c1 = short_pair(h)
        mid.append((pick(), pick(), c0, c1, bd[k % len(bd)] if k < 18 else rnd(64) % L))
    # every 4-bit digit 8, 7 and 15, at 32 digits, both signs of c0
    for d in (8, 7, 15):
        v = rep_digits(d, 4, 32)
        mid.append((pick(), pick(), v, v, rnd(64) % L))
        mid.append((pick(), pick(), -v, v, rnd(64) % L))
    # the fallback shape (h, 1), bits = 253; 63 digits of 8, 7 and 15
    for k, h in enumerate([L - 1, 2**252, 2**253 - 1, 2**252 + 1] + [rnd(32) >> 4 | 1 << 252 for _ in range(16)]):
        big.append((pick(), pick(), h if k % 3 else -h, 1, bd[k % len(bd)] if k < 12 else rnd(64) % L))
    for d in (8, 7, 15):
        v = rep_digits(d, 4, 63)
        big.append((pick(), pick(), v, v, rnd(64) % L))
        big.append((pick(), pick(), -v, v, rnd(64) % L))
    # tiny pairs
    for k in range(8):
        for c0 in (0, 1, -1):
            tiny.append((pick(), pick(), c0, 1, [0, 1, L - 1, rnd(64) % L][k % 4]))
    out = []
    lists = [big, mid, tiny]
    while any(lists):
        for l in lists:
            if l:
                out.append(l.pop(0))
    assert len(out) == 96, len(out)
    return [(A, R, c0, c1, b, max(abs(c0).bit_length(), c1.bit_length())) for A, R, c0, c1, b in out]


def ed_want(case):
    A, R, c0, c1, b, _ = case
    return lincomb([(b, E.BASE), (-c0, A), (-c1, R)])


def s_directed():
    """s < L: the ends, every 16-bit digit at, below and above half the window
    (cut to 252 bits), every 4-bit digit 8, 7 and 15"""
    m = (1 << 252) - 1
    return [0, 1, L - 1] + [rep_digits(d, 16, 16) & m for d in (0x8000, 0x7fff, 0xffff)] + \
        [rep_digits(d, 4, 63) for d in (8, 7, 15)]


def c_values(width):
    """the directed c at the chain's width 4 and at the table's width"""
    return list(dict.fromkeys(directed(4) + directed(width)))


def valid_keys():
    return [E.enc_pt(pt) for pt, _ in chain_points()[4:7]]


def u_cases(width):
    """96 x (key, c, s): three valid keys, the eight small-order encodings, a
    non-canonical key and one that does not decode"""
    rng = np.random.default_rng(0x0cf5)
    rnd = lambda n: int.from_bytes(rng.bytes(n), "little")  # noqa: E731
    cs, ss = c_values(width), s_directed()
    out = []
    for pk in valid_keys():
        for k in range(24):
            c = cs[k % len(cs)] if k < 18 else rnd(16)
            s = ss[(k // 2) % 6] if k < 12 else rnd(64) % L
            out.append((pk, c, s))
    for k, pk in enumerate(SMALL_ORDER):
        out.append((pk, cs[(3 * k) % len(cs)], rnd(64) % L))
        out.append((pk, rnd(16), ss[k % 6]))
    for pk in (NON_CANONICAL, NO_DECODE):
        out += [(pk, 5, 7), (pk, (1 << 128) - 1, L - 1), (pk, rnd(16), rnd(64) % L), (pk, 0, 0)]
    assert len(out) == 96, len(out)
    return out


def u_want(case):
    """[s]B - [c]Y, or None where the key is not a point"""
    pk, c, s = case
    Y = E.dec_pt(pk)
    if Y[0] is None:
        return None
    Y = (Y[0], Y[1] % P)
    return lincomb([(s % L, E.BASE), (-c, Y)])


def u_flag(pk):
    y = int.from_bytes(pk, "little") & M255
    return y < P and y not in E.SMALL_Y and E.recover_x(y % P, 0) is not None


def v_cases(width):
    """64 x (H, Gamma, c, s): [s]H - [c]Gamma"""
    rng = np.random.default_rng(0x0cf6)
    rnd = lambda n: int.from_bytes(rng.bytes(n), "little")  # noqa: E731
    pts = [pt for pt, _ in chain_points()]
    cs, ss = c_values(width), s_directed()
    out = []
    for k in range(64):
        c = cs[k % len(cs)] if k < 40 else rnd(16)
        s = ss[k % len(ss)] if k < 27 or k >= 54 else rnd(64) % L
        out.append((pts[k % len(pts)], pts[(3 * k + 1) % len(pts)], c, s))
    return out


def v_want(case):
    H, G, c, s = case
    return lincomb([(s % L, H), (-c, G)])
