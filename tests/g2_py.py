"""The twist of BN254 in Python integers, for tests: Fq2 = Fq[u] / (u^2 + 1) and y^2 = x^3 + 3 / (9 + u) in affine coordinates, None = infinity.  The plain reference of
the G2 fixed-base products (tests/test_gpu_fixed_mul.py, which pins it on 2 G2, r G2 = infinity and (a + b) P = a P + b P) and of the device pairing path
(tests/test_gpu_pairing_dev.py): membership in G2 by its definition [r]Q = infinity, points of the twist outside G2 (with a large and with a small order), and the closed
form of a weighted pairing product over multiples of the generators.  tests/test_pairing_refs_cpu.py holds these references against each other before a kernel is held
against them."""
import ctypes
import oracle_lib as ol

R, Q = ol.R, ol.Q

f2add = lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
f2sub = lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
f2mul = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def g2_add(p, q):
    if p is None: return q
    if q is None: return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if f2add(y1, y2) == (0, 0): return None
        lam = f2mul(f2mul((3, 0), f2mul(x1, x1)), f2inv(f2add(y1, y1)))
    else:
        lam = f2mul(f2sub(y2, y1), f2inv(f2sub(x2, x1)))
    x3 = f2sub(f2sub(f2mul(lam, lam), x1), x2)
    return (x3, f2sub(f2mul(lam, f2sub(x1, x3)), y1))


def g2_mul(p, k):
    acc = None
    for bit in bin(k)[2:]:
        acc = g2_add(acc, acc)
        if bit == '1': acc = g2_add(acc, p)
    return acc


def g2_mul_many(p, ks):
    """g2_mul for many scalars of one base: the doublings 2^i p are made once, a product is the sum of those its bits select (right to left)"""
    dbl = [p]
    for _ in range(max(ks).bit_length() - 1):
        dbl.append(g2_add(dbl[-1], dbl[-1]))
    out = []
    for k in ks:
        acc = None
        for i in range(k.bit_length()):
            if (k >> i) & 1: acc = g2_add(acc, dbl[i])
        out.append(acc)
    return out


def g2_bytes(p):
    return bytes(128) if p is None else b''.join(c.to_bytes(32, 'little') for c in (p[0][0], p[0][1], p[1][0], p[1][1]))


def g2_point(b):
    c = [int.from_bytes(b[32 * i:32 * i + 32], 'little') for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


G2_TWICE = ((18029695676650738226693292988307914797657423701064905010927197838374790804409, 14583779054894525174450323658765874724019480979794335525732096752006891875705),
            (2140229616977736810657479771656733941598412651537078903776637920509952744750, 11474861747383700316476719153975578001603231366361248090558603872215261634898))


def g2_neg(p):
    return None if p is None else (p[0], f2sub((0, 0), p[1]))


def on_twist(p):
    """y^2 = x^3 + 3 / (9 + u); infinity counts"""
    if p is None: return True
    b = f2mul((3, 0), f2inv((9, 1)))
    return f2mul(p[1], p[1]) == f2add(f2mul(f2mul(p[0], p[0]), p[0]), b)


def in_g2(p):
    """The definition: [r]p = infinity (p on the twist)"""
    return g2_mul(p, R) is None


# The twist has r h points, h = 2q - r, and h = 10069 x (a 241-bit rest).
TWIST_H = 2 * Q - R
SMALL_ORDER = 10069


def outside_points(count, start=1):
    """`count` points ol.twist_point_outside_g2 returns for growing starts, with distinct x0, each one classified by in_g2 as NOT in G2 (a start that yields a member is
    passed over)"""
    out, x0 = [], start
    while len(out) < count:
        p = ol.twist_point_outside_g2(x0)
        x0 = p[0][0] + 1
        if not in_g2(p):
            out.append(p)
    return out


_small = []


def small_order_point():
    """T of order 10069 on the twist: [(r h) / 10069] X for the first X of ol.twist_point_outside_g2 that does not give infinity.  Its order is coprime to r, so no
    multiple of T but infinity lies in G2, and Q + T is outside G2 for every Q in G2."""
    if not _small:
        assert TWIST_H % SMALL_ORDER == 0
        x0 = 1
        while True:
            X = ol.twist_point_outside_g2(x0)
            T = g2_mul(X, R * TWIST_H // SMALL_ORDER)
            if T is not None: break
            x0 = X[0][0] + 1
        assert g2_mul(T, SMALL_ORDER) is None and on_twist(T)
        _small.append(T)
    return _small[0]


# ---- the closed form of a pairing product ----
UNIT12 = (1).to_bytes(32, 'little') + bytes(352)         # 1 in Fq12, in zkc_pairing_bin's layout


def pairing_bin(g1, g2):
    """zkc_pairing_bin (host only; pinned to snarkjs' vk_alphabeta_12 by tests/test_host_abi_cpu.py): e(P, Q) as 384 bytes"""
    from zkcensus_amd import _native
    out = ctypes.create_string_buffer(384)
    assert _native.load().zkc_pairing_bin(bytes(g1), bytes(g2), out) == 0
    return out.raw


_pair_of = {}


def pairing_of_exponent(s):
    """e([s]G1, G2) for s mod r, the unit element written directly for s = 0; computed once per s"""
    from zkcensus_amd import engines
    s %= R
    if s == 0:
        return UNIT12
    if s not in _pair_of:
        _pair_of[s] = pairing_bin(ol.g1_mul(engines.G1_GENERATOR, s), engines.G2_GENERATOR)
    return _pair_of[s]


def expected_product(ws, as_, bs):
    """prod_i e(-w_i P_i, Q_i) for P_i = a_i G1 and Q_i = b_i G2 (a_i = 0 / b_i = 0: the point at infinity) by bilinearity: e([s]G1, G2) with
    s = -(sum_i w_i a_i b_i) mod r.  No Fq12 arithmetic of this file's own: one G1 product of the oracle and one host pairing."""
    return pairing_of_exponent(-sum(w * a * b for w, a, b in zip(ws, as_, bs)))
