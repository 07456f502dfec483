"""Curve points whose coordinates sit at the edges of the base field, for tests: GPU-free, no library, Python integers only (tests/g2_py.py for the twist).

Every point a test fed a kernel so far was k G or came out of a toxic-waste setup, so its coordinates were uniform in [0, q).  The kernels keep coordinates in the
lazily reduced nine-limb form of csrc/zkc_f29*.h, whose bounds are tightest for operands at the top of [0, q) -- and a coordinate enters that form as the Montgomery
residue a .zkey / .ptau stores (mont = True) or as a standard value the kernel converts on entry.  So the pools below hold ON-CURVE points with a coordinate that IS one
of EDGE_RESIDUES, either as its Montgomery residue (x = m 2^-256 mod q) or as its standard value:

    g1_pool()   x at an edge as a Montgomery residue | x at an edge as a standard value | y at an edge as a Montgomery residue (x a cube root of y^2 - 3)
    g2_pool()   twist points whose x has one or both components at an edge as Montgomery residues (x.c0 = 0 and x.c1 = 0 among them), tagged by g2_py.in_g2

each point next to its negation.  BN254 has q = 3 mod 4 (square roots by one power) and q - 1 = 9 t with 3 not dividing t (cube roots: a^(1/3 mod t) times a ninth root
of unity; every root is checked by cubing).  Plain affine G1 add / mul / msm are here too; the writers give both byte forms; patch_zkey puts pool points into the point
sections of a key image, which the key loader takes as they are."""
import collections
import random
import struct
import g2_py
from g2_py import f2add, f2mul, f2inv

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
assert (g2_py.R, g2_py.Q) == (R, Q)
MONT = 1 << 256
MONT_INV = pow(MONT, -1, Q)
POW2 = (0, 1, 28, 29, 31, 32, 58, 64, 128, 231, 232, 253)
_TOP = Q >> 232                                              # the ninth limb of q in radix 2^29
_ONES = (1 << 232) - 1                                       # eight limbs of 29 one-bits


def _dedupe(xs):
    return list(dict.fromkeys(xs))


# q - t (t = 1 .. 64), q - 2^k and 2^k, eight all-ones limbs under a top limb of 0, 1, half of q's and q's less one, and 0 .. 3.  May grow, never shrink.
EDGE_RESIDUES = _dedupe([Q - t for t in range(1, 65)] + [Q - (1 << k) for k in POW2] + [1 << k for k in POW2] +
                        [(top << 232) | _ONES for top in (0, 1, _TOP // 2, _TOP - 1)] + [0, 1, 2, 3])
assert all(0 <= m < Q for m in EDGE_RESIDUES) and len(EDGE_RESIDUES) == 92      # the 96 listed values; q - 1, q - 2, 1 and 2 are listed twice
# the residues the twist pool pairs up, 13 x 13 candidates for (x.c0, x.c1)
G2_RESIDUES = [0, 1, 2, Q - 1, Q - 2, Q - 64, 1 << 29, Q - (1 << 29), 1 << 232, Q - (1 << 232), Q - (1 << 253), _ONES, ((_TOP - 1) << 232) | _ONES]
assert set(G2_RESIDUES) <= set(EDGE_RESIDUES) and len(G2_RESIDUES) == 13

to_mont = lambda v: v * MONT % Q
from_mont = lambda m: m * MONT_INV % Q

G1Entry = collections.namedtuple('G1Entry', 'point group coord form residue')        # point (x, y); coord 'x' / 'y'; form 'mont' / 'std'; residue: that coordinate in that form
G2Entry = collections.namedtuple('G2Entry', 'point group coord form residue in_g2')   # point ((x0, x1), (y0, y1)); coord 'x'; residue (m0, m1)
G1_GROUPS = ('x-mont', 'x-std', 'y-mont')


# ---- G1 in affine coordinates, None = infinity ----
def on_curve(p):
    return p is None or (p[1] * p[1] - p[0] * p[0] * p[0] - 3) % Q == 0


def neg(p):
    return None if p is None else (p[0], -p[1] % Q)


def add(p, q):
    if p is None: return q
    if q is None: return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % Q == 0: return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return (x3, (lam * (x1 - x3) - y1) % Q)


def mul(p, k):
    acc = None
    for bit in bin(k)[2:] if k else '':
        acc = add(acc, acc)
        if bit == '1': acc = add(acc, p)
    return acc


def mul_many(p, ks):
    """mul for many scalars of one base: the doublings 2^i p are made once (as g2_py.g2_mul_many)"""
    dbl = [p]
    for _ in range(max(ks).bit_length() - 1):
        dbl.append(add(dbl[-1], dbl[-1]))
    out = []
    for k in ks:
        acc = None
        for i in range(k.bit_length()):
            if (k >> i) & 1: acc = add(acc, dbl[i])
        out.append(acc)
    return out


def _msm(add_, points, scalars):
    """sum k_i P_i bit by bit from the top: double the sum, then add the points whose scalar has that bit (the doublings are shared, nothing else is clever)"""
    ks = [k % R for k in scalars]
    acc = None
    for bit in range(max(ks, default=0).bit_length() - 1, -1, -1):
        acc = add_(acc, acc)
        for p, k in zip(points, ks):
            if (k >> bit) & 1: acc = add_(acc, p)
    return acc


def msm(points, scalars):
    return _msm(add, points, scalars)


def g2_msm(points, scalars):
    return _msm(g2_py.g2_add, points, scalars)


# ---- the inverse transform over points, step by step over the INTEGERS ----
def root_of_unity(logn):
    """the 2^logn-th root of unity of Fr the transforms use: 5^((r - 1) / 2^28), squared down"""
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - logn):
        w = w * w % R
    return w


def dit_lagrange(points, logn, add_, mul_many_, neg_):
    """out[c] = 1/n sum_i w^(-c i) P_i as csrc/zkc_ecntt.hip computes it, with every scalar the canonical integer below r of its residue: each input times 1/n mod r,
    stored at the bit-reversed index; then stage s (half = 2^s) takes P = v[a], Q = v[a + half] to (P + t Q, P - t Q), t = w_(2 half)^(-k) for k = a mod half,
    no product at k = 0.  On points of order r this is the MSM with the scalars w^(-c i) / n mod r whatever the steps; on a twist point outside G2, where [k]T and
    [k + r]T differ, only these steps say what the result is.  Products that share a base share its doublings (mul_many_)."""
    n = 1 << logn
    assert len(points) == n
    ninv = pow(n, -1, R)
    v = [None] * n
    for i, p in enumerate(points):
        if p is not None:
            v[int(format(i, '0%db' % logn)[::-1], 2) if logn else 0] = mul_many_(p, [ninv])[0]
    for s in range(logn):
        half = 1 << s
        wi = pow(root_of_unity(s + 1), -1, R)
        jobs = collections.defaultdict(list)                                       # base -> [(index of Q, twiddle)]
        for a in range(n):
            k = a & (half - 1)
            if not a & half and k and v[a + half] is not None:
                jobs[v[a + half]].append((a + half, pow(wi, k, R)))
        tq = {}
        for base, lst in jobs.items():
            for (b, _), prod in zip(lst, mul_many_(base, [t for _, t in lst])):
                tq[b] = prod
        for a in range(n):
            if not a & half:
                b = a + half
                q = tq.get(b, v[b])
                v[a], v[b] = add_(v[a], q), add_(v[a], neg_(q))
    return v


# ---- roots ----
def sqrt(a):
    """a square root of a mod q (q = 3 mod 4), or None"""
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


_T9 = (Q - 1) // 9
assert 9 * _T9 == Q - 1 and _T9 % 3
_ZETA9 = next(z for z in (pow(g, _T9, Q) for g in range(2, 50)) if pow(z, 3, Q) != 1)        # a primitive ninth root of unity


def cube_roots(a):
    """all x with x^3 = a mod q: three of them, or none (0 has the one root 0).  c = a^(1/3 mod t) has c^3 = a z for a cube root of unity z when a is a cube; a ninth
    root of unity takes z away.  Every root is checked by cubing."""
    a %= Q
    if a == 0: return [0]
    c = pow(a, pow(3, -1, _T9), Q)
    out = [x for x in (c * pow(_ZETA9, j, Q) % Q for j in range(9)) if pow(x, 3, Q) == a]
    assert len(out) in (0, 3) and len(set(out)) == len(out)
    assert (len(out) == 3) == (pow(a, (Q - 1) // 3, Q) == 1)
    return sorted(out)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1: r = f2mul(r, a)
        a = f2mul(a, a); e >>= 1
    return r


def f2sqrt(a):
    """a square root of a in Fq2 by the complex method for q = 3 mod 4 (as oracle_lib.twist_point_outside_g2), or None"""
    if a == (0, 0): return a
    a1 = f2pow(a, (Q - 3) // 4); alpha = f2mul(f2mul(a1, a1), a); x0 = f2mul(a1, a)
    y = f2mul((0, 1), x0) if alpha == (Q - 1, 0) else f2mul(f2pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2), x0)
    return y if f2mul(y, y) == a else None


TWIST_B = f2mul((3, 0), f2inv((9, 1)))

# ---- the pools ----
_pools = {}


def g1_pool():
    """list of G1Entry, a point and then its negation (the negation carries the same record: the edge coordinate of group 'y-mont' is that of the first of the two)"""
    if 'g1' in _pools: return _pools['g1']
    out = []
    for m in EDGE_RESIDUES:                                                        # x at an edge
        for form, x in (('mont', from_mont(m)), ('std', m)):
            if form == 'std' and m == 0: continue                                  # 0 is 0 in both forms: listed once
            y = sqrt(x * x * x + 3)
            if y:                                                                  # (y = 0 would be a point of order 2; the curve has none)
                y = min(y, Q - y)
                out += [G1Entry((x, y), 'x-' + form, 'x', form, m), G1Entry((x, Q - y), 'x-' + form, 'x', form, m)]
    for m in EDGE_RESIDUES:                                                        # y at an edge
        y = from_mont(m)
        if y and Q - m not in EDGE_RESIDUES[:EDGE_RESIDUES.index(m)]:              # q - m earlier in the list gave these same points as its negations
            for x in cube_roots(y * y - 3):
                out += [G1Entry((x, y), 'y-mont', 'y', 'mont', m), G1Entry((x, Q - y), 'y-mont', 'y', 'mont', Q - m)]
    out.sort(key=lambda e: G1_GROUPS.index(e.group))
    counts = g1_counts(out)
    assert counts['x-mont'] >= 40 and counts['x-std'] >= 40 and counts['y-mont'] >= 20, counts
    assert len({e.point for e in out}) == len(out)
    assert all(on_curve(e.point) and e.point[1] != 0 for e in out)                # none of order 2
    for a, b in zip(out[0::2], out[1::2]):
        assert b.point == neg(a.point)
    _pools['g1'] = out
    return out


def g1_counts(pool):
    return {g: sum(e.group == g for e in pool) for g in G1_GROUPS}


def g2_pool():
    """list of G2Entry, a point and then its negation; in_g2 is g2_py.in_g2 of the point, the tag a membership test compares against"""
    if 'g2' in _pools: return _pools['g2']
    out = []
    for m0 in G2_RESIDUES:
        for m1 in G2_RESIDUES:
            x = (from_mont(m0), from_mont(m1))
            y = f2sqrt(f2add(f2mul(f2mul(x, x), x), TWIST_B))
            if y is None: continue
            assert y != (0, 0)                                                     # none of order 2 (the twist has odd order r (2q - r))
            tag = g2_py.in_g2((x, y))
            for p in ((x, y), g2_py.g2_neg((x, y))):
                out.append(G2Entry(p, 'x-mont', 'x', 'mont', (m0, m1), tag))
    assert len(out) >= 64 and len({e.point for e in out}) == len(out)
    assert all(g2_py.on_twist(e.point) for e in out)
    assert any(e.residue[0] == 0 for e in out) and any(e.residue[1] == 0 for e in out)
    assert sum(not e.in_g2 for e in out) >= len(out) - 2                           # almost all outside G2: the subgroup is one part in 2q - r of the twist
    _pools['g2'] = out
    return out


# ---- bytes ----
_le = lambda v: v.to_bytes(32, 'little')


def g1_std(p):
    """64 B, standard form; all zero = infinity"""
    return bytes(64) if p is None else _le(p[0]) + _le(p[1])


def g1_mont(p):
    """64 B, Montgomery little-endian as a .zkey / .ptau stores a point; all zero = infinity"""
    return bytes(64) if p is None else _le(to_mont(p[0])) + _le(to_mont(p[1]))


def g2_std(p):
    return g2_py.g2_bytes(p)


def g2_mont(p):
    return bytes(128) if p is None else b''.join(_le(to_mont(c)) for c in (p[0][0], p[0][1], p[1][0], p[1][1]))


def g1_from_std(b):
    return None if not any(b) else (int.from_bytes(b[:32], 'little'), int.from_bytes(b[32:64], 'little'))


def g2_from_std(b):
    return None if not any(b) else g2_py.g2_point(b)


# ---- a key image with chosen bases ----
ZKEY_POINT_SECTIONS = {5: 64, 6: 64, 7: 128, 8: 64}          # A, B1, B2, C: bytes per point


def zkey_sections(image):
    """{type: (offset of the payload, size)}: the section walk of tests/host/top_fold_child.py sections()"""
    nsec = struct.unpack_from('<I', image, 8)[0]
    at, out = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from('<IQ', image, at)
        out[typ] = (at + 12, size)
        at += 12 + size
    return out


def patch_zkey(image, pools, seed):
    """-> (image, {section type: the points written, None = infinity}).  pools = (G1 points, twist points).  Point i of sections 5 (A), 6 (B1), 7 (B2) and 8 (C)
    becomes a pool point drawn by `seed`, in Montgomery form, about one in 50 the point at infinity; the pools are shorter than the sections, so the key also holds
    equal and opposite bases.  Header, H and everything else stay."""
    g1s, g2s = pools
    rng = random.Random(seed)
    img = bytearray(image)
    sec = zkey_sections(image)
    written = {}
    for typ, psz in ZKEY_POINT_SECTIONS.items():
        at, size = sec[typ]
        assert size % psz == 0
        pool, enc = (g2s, g2_mont) if psz == 128 else (g1s, g1_mont)
        pts = [None if rng.randrange(50) == 0 else pool[rng.randrange(len(pool))] for _ in range(size // psz)]
        img[at:at + size] = b''.join(enc(p) for p in pts)
        written[typ] = pts
    assert len(img) == len(image)
    return bytes(img), written
