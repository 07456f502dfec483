"""CPU: the pools of tests/edge_points.py and the references the GPU tests hold kernels against (tests/test_gpu_point_edges.py), before a kernel is held against them.
Every pool point satisfies its curve equation, written out here once more; the coordinate a record names has the residue it names, in the form it names; the counts hold.
The Python G1 arithmetic and g2_py's agree with the C oracle's products and MSMs ON THE POOLS, which runs the oracle on edge coordinates for the first time; the oracle
parses a patched key image back to exactly the points written; and the host pairing takes pool points and is bilinear on them."""
import random
import pytest
import oracle_lib as ol
import g2_py
import edge_points as ep
import msm_cases as mc

R, Q = ol.R, ol.Q
le = lambda v: v.to_bytes(32, 'little')


@pytest.fixture(scope='module')
def g1():
    return ep.g1_pool()


@pytest.fixture(scope='module')
def g2():
    return ep.g2_pool()


def test_residue_list():
    want = [Q - t for t in range(1, 65)] + [0, 1, 2, 3]
    for k in (0, 1, 28, 29, 31, 32, 58, 64, 128, 231, 232, 253):
        want += [1 << k, Q - (1 << k)]
    ones = (1 << 232) - 1
    want += [ones, (1 << 232) | ones, ((Q >> 232) // 2 << 232) | ones, ((Q >> 232) - 1 << 232) | ones]
    assert set(want) <= set(ep.EDGE_RESIDUES) and len(set(want)) == 92
    assert all(0 <= m < Q for m in ep.EDGE_RESIDUES) and len(set(ep.EDGE_RESIDUES)) == len(ep.EDGE_RESIDUES)


def test_g1_pool_points_are_on_the_curve_with_the_stated_residue(g1):
    for e in g1:
        x, y = e.point
        assert 0 <= x < Q and 0 < y < Q and (y * y - (x * x * x + 3)) % Q == 0
        v = {'x': x, 'y': y}[e.coord]
        assert (v * (1 << 256) % Q if e.form == 'mont' else v) == e.residue
        assert e.group == e.coord + '-' + e.form
    first = g1[0::2]
    assert all(e.residue in ep.EDGE_RESIDUES for e in first)                       # of each pair, the first sits at the edge (for x both do)
    assert all(e.residue in ep.EDGE_RESIDUES for e in g1 if e.coord == 'x')
    assert [b.point for b in g1[1::2]] == [(a.point[0], Q - a.point[1]) for a in first]
    counts = ep.g1_counts(g1)
    assert counts['x-mont'] >= 40 and counts['x-std'] >= 40 and counts['y-mont'] >= 20 and sum(counts.values()) == len(g1) == len({e.point for e in g1})
    # the limb patterns the nine-limb form is tightest at are really there: a residue within 64 of q, one below 4, and eight all-ones limbs, in each form of x
    for form in ('mont', 'std'):
        rs = [e.residue for e in g1 if e.coord == 'x' and e.form == form]
        assert any(Q - r <= 64 for r in rs) and any(r < 4 for r in rs) and any(r & ((1 << 232) - 1) == (1 << 232) - 1 for r in rs), form


def test_g2_pool_points_are_on_the_twist_with_the_stated_residue(g2):
    b = g2_py.f2mul((3, 0), g2_py.f2inv((9, 1)))
    sq = lambda a: ((a[0] * a[0] - a[1] * a[1]) % Q, 2 * a[0] * a[1] % Q)
    for e in g2:
        x, y = e.point
        x3 = g2_py.f2mul(sq(x), x)
        assert sq(y) == ((x3[0] + b[0]) % Q, (x3[1] + b[1]) % Q) and y != (0, 0)
        assert (x[0] * (1 << 256) % Q, x[1] * (1 << 256) % Q) == e.residue and set(e.residue) <= set(ep.EDGE_RESIDUES)
    assert len(g2) >= 64 and len({e.point for e in g2}) == len(g2)
    assert [b_.point for b_ in g2[1::2]] == [g2_py.g2_neg(a.point) for a in g2[0::2]]
    assert any(e.residue[0] == 0 for e in g2) and any(e.residue[1] == 0 for e in g2)
    # the tags: the definition [r]Q = infinity once more on a sample, and what -Q must share with Q
    for e in g2[::17]:
        assert e.in_g2 == (g2_py.g2_mul(e.point, R) is None)
    assert all(a.in_g2 == b_.in_g2 for a, b_ in zip(g2[0::2], g2[1::2]))
    assert sum(not e.in_g2 for e in g2) >= len(g2) - 2


def test_cube_and_square_roots():
    rng = random.Random(5)
    for a in [0, 1, 8, 27, Q - 1, Q - 8] + [pow(rng.randrange(Q), 3, Q) for _ in range(5)]:
        roots = ep.cube_roots(a)
        assert len(roots) == (1 if a == 0 else 3) and all(pow(x, 3, Q) == a for x in roots)
    assert ep.cube_roots(2) == [] or all(pow(x, 3, Q) == 2 for x in ep.cube_roots(2))
    assert sum(bool(ep.cube_roots(a)) for a in range(2, 62)) in range(8, 35)       # a third of the field are cubes
    assert ep.sqrt(4) in (2, Q - 2) and ep.sqrt(Q - 1) is None                      # q = 3 mod 4: -1 is no square
    for a in ((0, 1), (5, 0), (Q - 1, 0), (3, 7)):
        y = ep.f2sqrt(g2_py.f2mul(a, a))
        assert y in (a, ((-a[0]) % Q, (-a[1]) % Q))


def test_python_g1_agrees_with_the_oracle_on_the_pool(g1):
    rng = random.Random(6)
    pts = [e.point for e in g1]
    G = (1, 2)
    assert ep.g1_std(ep.mul(G, 7)) == ol.g1_mul(ep.g1_std(G), 7) and ep.mul(G, R) is None and ep.mul(G, 0) is None
    edge = [1, 2, 3, R - 1, R - 2, 1 << 128, (1 << 253) + 1]
    for i, p in enumerate(pts):
        assert ep.mul(p, R) is None if i % 40 == 0 else True                       # order r: the curve has no other
        k = edge[i % len(edge)] if i % 2 else rng.randrange(1, R)
        assert ep.g1_std(ep.mul(p, k)) == ol.g1_mul(ep.g1_std(p), k), (i, hex(k))
        assert ep.g1_from_std(ep.g1_std(p)) == p
    assert ep.add(pts[0], pts[1]) is None and ep.add(pts[0], pts[0]) == ep.mul(pts[0], 2)
    # MSMs over the whole pool: full-size scalars, small ones (every term a low multiple of an edge point), all equal (P and -P cancel throughout: infinity)
    bases = b''.join(ep.g1_std(p) for p in pts)
    for ks in ([rng.randrange(R) for _ in pts], [rng.randrange(1, 1 << 12) for _ in pts], [R - 1] * (len(pts) - 1) + [5], [9] * len(pts)):
        got = ep.msm(pts, ks)
        assert ep.g1_std(got) == ol.msm_g1(bases, b''.join(le(k) for k in ks))
    assert ep.msm(pts, [9] * len(pts)) is None
    some = pts[::9] + [None, None]
    ks = [rng.randrange(R) for _ in some]
    ref = None
    for p, k in zip(some, ks):
        ref = ep.add(ref, ep.mul(p, k))                                            # the shared-doubling MSM against the sum of products
    assert ep.msm(some, ks) == ref and ep.g1_std(ref) == ol.msm_g1(b''.join(ep.g1_std(p) for p in some), b''.join(le(k) for k in ks))


def test_python_g2_agrees_with_the_oracle_on_the_pool(g2):
    rng = random.Random(7)
    pts = [e.point for e in g2]
    edge = [1, 2, 3, R - 1, R - 2, 1 << 128]
    for i, p in enumerate(pts):
        k = edge[i % len(edge)] if i % 2 else rng.randrange(1, R)
        assert ep.g2_std(g2_py.g2_mul(p, k)) == ol.msm_g2(ep.g2_std(p), le(k)), (i, hex(k))
        assert ep.g2_from_std(ep.g2_std(p)) == p
    bases = b''.join(ep.g2_std(p) for p in pts)
    for ks in ([rng.randrange(R) for _ in pts], [rng.randrange(1, 1 << 12) for _ in pts]):
        assert ep.g2_std(ep.g2_msm(pts, ks)) == ol.msm_g2(bases, b''.join(le(k) for k in ks))
    ks = [rng.randrange(1 << 64) for _ in range(4)] + [0, R - 1]
    assert g2_py.g2_mul_many(pts[0], ks) == [g2_py.g2_mul(pts[0], k) if k else None for k in ks]


def test_stepwise_transform_is_the_transform_on_points_of_order_r(g1):
    """edge_points.dit_lagrange, the reference of the G2 transform on twist points outside G2, against the oracle's n MSMs with the scalars w^(-c i) / n where both
    mean the same: G1 pool points and multiples of the G2 generator, with infinity, equal and opposite inputs among them"""
    import ptau_lib as pl
    from zkcensus_amd import engines
    assert all(ep.root_of_unity(k) == pl.root_of_unity(k) and pow(ep.root_of_unity(k), 1 << k, R) == 1 for k in (1, 3, 7))
    rng = random.Random(8)
    G2 = g2_py.g2_point(engines.G2_GENERATOR)
    for logn in (0, 1, 3, 4):
        n = 1 << logn
        wi, ninv = pow(ep.root_of_unity(logn), -1, R), pow(n, -1, R)
        rows = [b''.join(le(pow(wi, c * i, R) * ninv % R) for i in range(n)) for c in range(n)]
        p1 = [e.point for e in rng.sample(g1, n)]
        p2 = g2_py.g2_mul_many(G2, [rng.randrange(1, R) for _ in range(n)])
        if n >= 8:
            p1[2] = p2[2] = None
            p1[5], p1[6], p1[7] = g1[0].point, g1[1].point, g1[0].point            # P, -P, P
            p2[5], p2[6], p2[7] = p2[0], g2_py.g2_neg(p2[0]), p2[0]
        std1, std2 = b''.join(ep.g1_std(p) for p in p1), b''.join(ep.g2_std(p) for p in p2)
        assert [ep.g1_std(p) for p in ep.dit_lagrange(p1, logn, ep.add, ep.mul_many, ep.neg)] == [ol.msm_g1(std1, row) for row in rows], logn
        assert [ep.g2_std(p) for p in ep.dit_lagrange(p2, logn, g2_py.g2_add, g2_py.g2_mul_many, g2_py.g2_neg)] == [ol.msm_g2(std2, row) for row in rows], logn


def test_byte_forms(g1, g2):
    p, t = g1[0].point, g2[0].point
    assert ep.g1_std(None) == ep.g1_mont(None) == bytes(64) and ep.g2_std(None) == ep.g2_mont(None) == bytes(128)
    assert ep.g1_std(p) == le(p[0]) + le(p[1]) and ep.g1_mont(p)[:32] == le(g1[0].residue) and g1[0].group == 'x-mont'
    assert ep.g2_mont(t)[:64] == le(g2[0].residue[0]) + le(g2[0].residue[1])
    std = b''.join(le(int.from_bytes(ep.g2_mont(t)[32 * i:32 * i + 32], 'little') * pow(1 << 256, -1, Q) % Q) for i in range(4))
    assert std == ep.g2_std(t)


@pytest.fixture(scope='module')
def small_key(tmp_path_factory):
    from test_generic_circuit import random_instance, setup_key
    r1, _ = random_instance(tmp_path_factory.mktemp('edgekey'), 300, 200, 3, seed=41)
    zk, _ = setup_key(r1, 77)
    return zk


def test_patched_key_parses_back_to_the_written_points(small_key, g1, g2):
    pools = ([e.point for e in g1], [e.point for e in g2])
    img, written = ep.patch_zkey(small_key, pools, seed=9)
    again, written2 = ep.patch_zkey(small_key, pools, seed=9)
    assert img == again and written == written2 and img != ep.patch_zkey(small_key, pools, seed=10)[0]
    z0, z = ol.zkey_parse(small_key), ol.zkey_parse(img)
    assert (z.nVars, z.nPublic, z.domainSize, z.nCoeffs) == (z0.nVars, z0.nPublic, z0.domainSize, z0.nCoeffs) == (200, 3, 512, z0.nCoeffs)
    assert [len(written[t]) for t in (5, 6, 7, 8)] == [200, 200, 200, 196]
    for which, typ in ((0, 5), (1, 6), (2, 7)):
        raw, std = mc.section_points(z, which, z.nVars)
        enc_m, enc_s = (ep.g2_mont, ep.g2_std) if typ == 7 else (ep.g1_mont, ep.g1_std)
        assert raw == b''.join(enc_m(p) for p in written[typ]) and std == b''.join(enc_s(p) for p in written[typ])
    import ctypes
    assert ctypes.string_at(z.pointsC, 64 * 196) == b''.join(ep.g1_mont(p) for p in written[8])
    # everything outside the four sections is as it was
    sec = ep.zkey_sections(small_key)
    keep = bytearray(len(img))
    for typ in ep.ZKEY_POINT_SECTIONS:
        at, size = sec[typ]
        keep[at:at + size] = b'\x01' * size
    assert all(a == b for a, b, k in zip(small_key, img, keep) if not k) and ep.zkey_sections(img) == sec
    assert sum(k for k in keep) == 64 * (200 + 200 + 196) + 128 * 200
    for typ in (5, 6, 7, 8):
        pts = written[typ]
        assert any(p is None for p in pts) and len(set(pts)) < len(pts)            # infinity and repeated bases are in
    neg = {ep.neg(p) for p in written[5] if p}
    assert neg & set(written[5])                                                   # and opposite ones


def test_host_pairing_takes_pool_points_and_is_bilinear_on_them(g1):
    from zkcensus_amd import engines
    G2 = g2_py.g2_point(engines.G2_GENERATOR)
    five_g2 = g2_py.g2_bytes(g2_py.g2_mul(G2, 5))
    picks = [next(e for e in g1 if e.group == g) for g in ep.G1_GROUPS]
    seen = set()
    for e in picks:
        lhs = g2_py.pairing_bin(ep.g1_std(e.point), five_g2)
        rhs = g2_py.pairing_bin(ep.g1_std(ep.mul(e.point, 5)), engines.G2_GENERATOR)
        assert lhs == rhs != g2_py.UNIT12, e.group
        assert g2_py.pairing_bin(ep.g1_std(ep.mul(e.point, 4)), engines.G2_GENERATOR) != lhs
        seen.add(lhs)
    assert len(seen) == 3
