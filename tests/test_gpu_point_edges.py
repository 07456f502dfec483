"""GPU: the group kernels on points whose COORDINATES sit at the edges of the base field.  Every point another test feeds a kernel is k G or comes from a toxic-waste
setup, so its coordinates are uniform in [0, q); here they come from the pools of tests/edge_points.py: on-curve points with x or y a Montgomery residue (or x a standard
value) within 64 of q, q - 2^k, 2^k, 0 .. 3 or eight all-ones 29-bit limbs, and twist points (outside G2) with such x components, x.c0 = 0 and x.c1 = 0 among them.  That
is where the lazily reduced nine-limb form of csrc/zkc_f29*.h has its tightest bounds, and tests/test_f29_host.py reaches it on the host only.

The C oracle is the reference everywhere (tests/test_edge_points_cpu.py holds it against Python on these very pools first); exact Python integers are the reference as
well wherever a few hundred points suffice.  Scalars on twist points outside G2 are plain integers below r on both sides (such a point's order does not divide r).
Shapes are the smallest that reach a kernel's branches: the 1024-scalar tile of the bucketing from both sides, the 128-pair threshold of the pairing fold, one wave of
butterflies and one past it."""
import random
import pytest
import oracle_lib as ol
import g2_py
import edge_points as ep
import msm_cases as mc
import ptau_lib as pl
from test_gpu_msm_edges import _kinds, c_for

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
KINDS = ('low-window', 'equal', 'uniform', 'r-1', 'half', 'zero')
le = lambda v: v.to_bytes(32, 'little')
scalars_le = lambda ks: b''.join(le(k) for k in ks)


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


@pytest.fixture(scope='module')
def g1():
    return ep.g1_pool()


@pytest.fixture(scope='module')
def g2():
    return ep.g2_pool()


def _dev(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _six(g1):
    """two pool entries per group, from both ends of each group's residue list"""
    out = []
    for g in ep.G1_GROUPS:
        es = [e for e in g1 if e.group == g]
        out += [es[0], es[-1]]
    return out


def _kinds_of(n, rng, wires=None):
    """the scalar kinds of KINDS for n bases at the window width the engine picks for them (for a key's section: by the key's wire count)"""
    return [(k, ss) for k, ss in _kinds(n, None, rng, c_for(wires or n)) if k in KINDS]


# ---- zkc_msm_g1_load_dev / zkc_msm_g1_dev ----
def test_msm_over_the_pool_alone(gpu, g1):
    """n = len(pool): every base an edge point, each next to its negation; against Python and the oracle.  `low-window` makes every addition take a window-0 row, which
    is the caller's own coordinates."""
    ctx, torch = gpu
    from zkcensus_amd import engines
    pts = [e.point for e in g1]
    n = len(pts); assert n < 1024
    bases = b''.join(ep.g1_std(p) for p in pts)
    d_bases = _dev(torch, bases)
    tbl = engines.G1Bases(ctx, d_bases.data_ptr(), n)
    try:
        kinds = _kinds_of(n, random.Random(n))
        assert [k for k, _ in kinds] == ['zero', 'equal', 'uniform', 'r-1', 'half', 'low-window']
        for name, ss in kinds:
            if name in ('equal', 'r-1'):
                ss = ss[:-1] + [5]                                                 # every P sits next to -P: all equal scalars would cancel to infinity whatever the buckets held
            got = tbl.multiExpAffine(_dev(torch, scalars_le(ss)).data_ptr())
            exp = ep.msm(pts, ss)
            assert (exp is None) == (name == 'zero'), name
            assert got == ol.msm_g1(bases, scalars_le(ss)), name + ' (oracle)'
            assert got == ep.g1_std(exp), name + ' (Python)'
    finally:
        tbl.close()


@pytest.mark.parametrize('n', [1025, 4097])
def test_msm_pool_cycled_off_the_tile(gpu, g1, n):
    """the pool cycled over n slots off the 1024-scalar tile (12-bit windows), a quarter of the slots k G; every scalar kind on one handle, against the oracle"""
    ctx, torch = gpu
    from zkcensus_amd import engines
    rng = random.Random(n)
    G = ep.g1_std((1, 2))
    pool = [ep.g1_std(e.point) for e in g1]
    slots = [None if i % 4 == 3 else pool[i % len(pool)] for i in range(n)]
    kg = ol.pmap(lambda k: ol.g1_mul(G, k), [rng.randrange(1, R) for s in slots if s is None])
    it = iter(kg)
    bases = b''.join(s if s is not None else next(it) for s in slots)
    d_bases = _dev(torch, bases)
    tbl = engines.G1Bases(ctx, d_bases.data_ptr(), n)
    try:
        kinds = _kinds_of(n, rng)
        got = [tbl.multiExpAffine(_dev(torch, scalars_le(ss)).data_ptr()) for _, ss in kinds]
        exp = ol.pmap(lambda ks: ol.msm_g1(bases, scalars_le(ks[1])), kinds)
        for (name, _), g, e in zip(kinds, got, exp):
            assert g == e, '%s scalars, n = %d' % (name, n)
        assert len({e for e in exp}) >= 5 and exp[0] == bytes(64)                  # zero: infinity; the other kinds tell each other apart
    finally:
        tbl.close()


# ---- the products of one base ----
def _batch_scalars(rng, n=64):
    edge = [0, 1, 2, R - 1, R - 2] + [1 << k for k in (1, 7, 8, 28, 29, 64, 128, 252, 253)]
    return edge + [rng.randrange(R) for _ in range(n - len(edge))]


def _run(gpu, fn, base, ks, width):
    ctx, torch = gpu
    d_k = _dev(torch, scalars_le(ks))
    d_out = torch.full((width * len(ks),), 0xA5, dtype=torch.uint8, device='cuda')
    fn(ctx, base, d_k.data_ptr(), len(ks), d_out.data_ptr())
    raw = d_out.cpu().numpy().tobytes()
    return [raw[width * i:width * (i + 1)] for i in range(len(ks))]


def test_g1_products_of_edge_bases(gpu, g1):
    """zkc_g1_mul_batch_dev (double and add) and zkc_g1_fixed_mul_dev (window table of the base) on six pool bases, 64 scalars each, against Python"""
    from zkcensus_amd import engines
    rng = random.Random(61)
    for e in _six(g1):
        ks = _batch_scalars(rng)
        assert len(ks) == 64
        exp = [ep.g1_std(p) for p in ep.mul_many(e.point, ks)]
        for fn in (engines.g1_mul_batch, engines.g1_fixed_mul):
            got = _run(gpu, fn, ep.g1_std(e.point), ks, 64)
            bad = [hex(k) for k, g, x in zip(ks, got, exp) if g != x]
            assert not bad, (fn.__name__, e.group, hex(e.residue), bad[:4])
        assert exp[0] == bytes(64) and exp[1] == ep.g1_std(e.point) and exp[3] == ep.g1_std(ep.neg(e.point))


def test_g2_fixed_products_of_edge_bases(gpu, g2):
    """zkc_g2_fixed_mul_dev on six twist-pool bases (x.c0 = 0, x.c1 = 0, both at q - 1 ... none in G2: integer scalars), 32 scalars below 2^64 and 8 of full size"""
    from zkcensus_amd import engines
    rng = random.Random(62)
    picks = [next(e for e in g2 if e.residue[0] == 0), next(e for e in g2 if e.residue[1] == 0), g2[-1], g2[len(g2) // 2], g2[len(g2) // 3 | 1],
             max(g2, key=lambda e: min(e.residue))]
    assert len({e.point for e in picks}) == 6
    for e in picks:
        ks = [0, 1, 2, (1 << 64) - 1, 1 << 63] + [rng.randrange(1 << 64) for _ in range(27)] + [R - 1, R - 2, 1 << 253] + [rng.randrange(R) for _ in range(5)]
        assert len(ks) == 40
        exp = [ep.g2_std(p) for p in g2_py.g2_mul_many(e.point, ks)]
        got = _run(gpu, engines.g2_fixed_mul, ep.g2_std(e.point), ks, 128)
        bad = [hex(k) for k, g, x in zip(ks, got, exp) if g != x]
        assert not bad, ([hex(m) for m in e.residue], bad[:4])


# ---- zkc_g1_scale_dev ----
def test_g1_scale_of_the_whole_pool(gpu, g1):
    """the whole pool and three infinities times one scalar, standard and Montgomery form, out of place and in place, against Python"""
    ctx, torch = gpu
    from zkcensus_amd import engines
    pts = [e.point for e in g1]
    pts = pts[:7] + [None] + pts[7:200] + [None] + pts[200:] + [None]
    k_rand = random.Random(63).randrange(3, R - 2)
    twice = [ep.add(p, p) for p in pts]
    expected = {1: pts, 2: twice, R - 2: [ep.neg(p) for p in twice], R - 1: [ep.neg(p) for p in pts],       # the curve has prime order r
                k_rand: [ep.mul(p, k_rand) if p else None for p in pts]}
    for i in (0, len(pts) // 2, len(pts) - 2):
        assert ep.mul(pts[i], R - 2) == expected[R - 2][i] and ep.mul(pts[i], R - 1) == expected[R - 1][i]
    for mont in (False, True):
        enc = ep.g1_mont if mont else ep.g1_std
        src = b''.join(enc(p) for p in pts)
        for k, exp in expected.items():
            want = b''.join(enc(p) for p in exp)
            for inplace in (False, True):
                d_in = _dev(torch, src)
                d_out = d_in if inplace else torch.full((len(src),), 0xA5, dtype=torch.uint8, device='cuda')
                engines.g1_scale(ctx, d_in.data_ptr(), len(pts), k, d_out.data_ptr(), mont=mont)
                got = d_out.cpu().numpy().tobytes()
                bad = [i for i in range(len(pts)) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
                assert not bad, ('k = %x, mont %s, in place %s: points' % (k, mont, inplace), bad[:8])
                if not inplace:
                    assert d_in.cpu().numpy().tobytes() == src


# ---- zkc_g1_lagrange_dev / zkc_g2_lagrange_dev ----
def _lagrange_scalars(logn):
    """row c: the scalars w^(-c i) / n of output c"""
    n = 1 << logn
    wi, ninv = pow(pl.root_of_unity(logn), -1, R), pow(n, -1, R)
    return [[pow(wi, c * i, R) * ninv % R for i in range(n)] for c in range(n)]


@pytest.mark.parametrize('logn', [3, 7])
def test_g1_lagrange_of_pool_points(gpu, g1, logn):
    """out[c] = sum_i (w^(-c i) / n) P_i is n MSMs of n points for the oracle; at logn 3 for Python as well.  Both coordinate forms, out of place and in place."""
    ctx, torch = gpu
    from zkcensus_amd import engines
    n = 1 << logn
    rng = random.Random(70 + logn)
    pts = [e.point for e in rng.sample(g1, n - 1)]
    pts.insert(n // 2, None)                                                       # one input at infinity
    if logn == 3:
        pts[1], pts[2] = g1[0].point, g1[1].point                                  # P and -P side by side
    rows = _lagrange_scalars(logn)
    std = b''.join(ep.g1_std(p) for p in pts)
    exp = ol.pmap(lambda row: ol.msm_g1(std, scalars_le(row)), rows)
    if logn == 3:
        assert exp == [ep.g1_std(ep.msm(pts, row)) for row in rows]
    for mont in (False, True):
        a, e = (pl.to_mont(std), pl.to_mont(b''.join(exp))) if mont else (std, b''.join(exp))
        for inplace in (False, True):
            d_in = _dev(torch, a)
            d_out = d_in if inplace else torch.full((64 * n,), 0xA5, dtype=torch.uint8, device='cuda')
            engines.g1_lagrange(ctx, d_in.data_ptr(), logn, d_out.data_ptr(), mont=mont)
            got = d_out.cpu().numpy().tobytes()
            bad = [c for c in range(n) if got[64 * c:64 * c + 64] != e[64 * c:64 * c + 64]]
            assert not bad, ('logn %d, mont %s, in place %s: outputs' % (logn, mont, inplace), bad[:8])


def _g2_vectors(g2, logn):
    """input vectors of twist-pool points for the G2 transform.  logn 3: dense, every lane of the load a pool point, with infinity and T, -T side by side among them.
    logn 7: finite at the indices 0, 1 and n/2 alone -- stage 0 adds the first and the third, the stages between pass sums on beside infinity, and the last stage
    forms P + t Q for all 63 non-unit twiddles on the second; the reference then costs one base's doublings per vector."""
    rng = random.Random(90 + logn)
    n = 1 << logn
    zero = [e.point for e in g2 if 0 in e.residue]
    if logn == 3:
        vs = [[e.point for e in rng.sample(g2, n)] for _ in range(4)]
        vs[0][3] = None
        vs[1][4], vs[1][5] = g2[0].point, g2[1].point
        vs[2][:4] = zero[:4]
        return vs
    vs = []
    for k in range(3):
        v = [None] * n
        v[0], v[1], v[n // 2] = [e.point for e in rng.sample(g2, 3)]
        if k == 0: v[1] = zero[0]
        vs.append(v)
    return vs


@pytest.mark.parametrize('logn', [3, 7])
def test_g2_lagrange_of_pool_points(gpu, g2, logn):
    """The transform's scalars w^(-c i) / n are residues mod r, which mean something on points of order r only, and no pool point lies in G2: on a twist point T
    outside G2, [k]T and [k + r]T differ and the oracle's MSM is no reference.  The kernel's own steps over the integers are exact, though (csrc/zkc_ecntt.hip: each
    input times the canonical integer of 1/n mod r, then radix-2 butterflies P +- t Q with the canonical integer of each twiddle), and edge_points.dit_lagrange takes
    them in Python integers; tests/test_edge_points_cpu.py holds it against the oracle's MSMs on points of order r.  Both coordinate forms, out of place and in place."""
    ctx, torch = gpu
    from zkcensus_amd import engines
    n = 1 << logn
    for vi, pts in enumerate(_g2_vectors(g2, logn)):
        exp = ep.dit_lagrange(pts, logn, g2_py.g2_add, g2_py.g2_mul_many, g2_py.g2_neg)
        assert sum(p is not None for p in exp) >= n - 1
        for mont in (False, True):
            enc = ep.g2_mont if mont else ep.g2_std
            a, e = b''.join(enc(p) for p in pts), b''.join(enc(p) for p in exp)
            for inplace in ((False, True) if vi == 0 else (False,)):
                d_in = _dev(torch, a)
                d_out = d_in if inplace else torch.full((128 * n,), 0xA5, dtype=torch.uint8, device='cuda')
                engines.g2_lagrange(ctx, d_in.data_ptr(), logn, d_out.data_ptr(), mont=mont)
                got = d_out.cpu().numpy().tobytes()
                bad = [c for c in range(n) if got[128 * c:128 * c + 128] != e[128 * c:128 * c + 128]]
                assert not bad, ('vector %d, logn %d, mont %s, in place %s: outputs' % (vi, logn, mont, inplace), bad[:8])


def test_g2_lagrange_passes_pool_points_through(gpu, g2):
    """n = 1, out = in: the entry and exit paths of zkc_g2_lagrange_dev alone, in both coordinate forms, where the components at 0, 1, q - 1 and the all-ones limbs enter
    and leave the limb form; a fifth of the pool and six points with a zero component"""
    ctx, torch = gpu
    from zkcensus_amd import engines
    picks = g2[::5] + [e for e in g2 if 0 in e.residue][:6]
    for mont in (False, True):
        enc = ep.g2_mont if mont else ep.g2_std
        src = b''.join(enc(e.point) for e in picks)
        for i, e in enumerate(picks):
            d_in = _dev(torch, src[128 * i:128 * i + 128])
            d_out = torch.full((128,), 0xA5, dtype=torch.uint8, device='cuda')
            engines.g2_lagrange(ctx, d_in.data_ptr(), 0, d_out.data_ptr(), mont=mont)
            assert d_out.cpu().numpy().tobytes() == enc(e.point), ([hex(m) for m in e.residue], mont)


# ---- zkc_debug_pairing_dev ----
@pytest.fixture(scope='module')
def pairs(g1):
    """130 members (P_i, b_i, w_i): P_i a pool point, Q_i = b_i G2 with small b_i (two at infinity), 128-bit weights and 1, r - 1, 2^255 at the end, where a batch of
    3 finds them.  -> (members, {b: bytes of b G2})"""
    from zkcensus_amd import engines
    rng = random.Random(64)
    entries = [e for grp in ep.G1_GROUPS for e in [x for x in g1 if x.group == grp][:44]][:130]
    assert len(entries) == 130 and {e.group for e in entries} == set(ep.G1_GROUPS)
    bs = [rng.randrange(1, 24) for _ in range(130)]
    bs[5] = bs[128] = 0
    ws = [rng.randrange(1, 1 << 128) for _ in range(127)] + [1, R - 1, 1 << 255]
    q = dict(zip(range(1, 24), g2_py.g2_mul_many(g2_py.g2_point(engines.G2_GENERATOR), list(range(1, 24)))))
    q[0] = None
    return [(e.point, b, w) for e, b, w in zip(entries, bs, ws)], {b: ep.g2_std(p) for b, p in q.items()}


@pytest.mark.parametrize('N', [130, 3])
def test_pairing_fold_of_pool_points(gpu, pairs, N):
    """folded_out = w_i P_i from Python; product_out = e(-sum_i w_i b_i P_i, G2): the sum in Python, one host pairing.  N = 130 is above the 128-pair threshold."""
    ctx, _ = gpu
    from zkcensus_amd import groth16, engines
    members, qs = pairs
    batch = members[-N:]
    assert sum(b == 0 for _, b, _ in batch) == (2 if N == 130 else 1)
    g1b = b''.join(ep.g1_std(p) for p, _, _ in batch)
    g2b = b''.join(qs[b] for _, b, _ in batch)
    prod, bad, folded, _, _ = groth16.debug_pairing_dev(ctx, g1b, g2b, scalars_le(w for _, _, w in batch), folded=True)
    for i, (p, _, w) in enumerate(batch):
        assert folded[64 * i:64 * i + 64] == ep.g1_std(ep.mul(p, w % R)), ('folded', i, hex(w))
    assert bad == 0
    s = ep.msm([p for p, _, _ in batch], [w * b for _, b, w in batch])
    assert s is not None
    assert prod == g2_py.pairing_bin(ep.g1_std(ep.neg(s)), engines.G2_GENERATOR)


def test_membership_of_the_twist_pool(gpu, g2):
    """the twist pool as g2, the generator as every P: member_out and *bad_out against the pool's in_g2 tags; a few multiples of G2 (tagged the same way) sit among them"""
    ctx, _ = gpu
    from zkcensus_amd import groth16, engines
    inside = g2_py.g2_mul_many(g2_py.g2_point(engines.G2_GENERATOR), [1, 2, R - 1, 12345])
    assert all(g2_py.in_g2(p) for p in inside)
    batch = [(e.point, e.in_g2) for e in g2]
    for k, p in enumerate(inside):
        batch.insert(1 + 43 * k, (p, True))
    batch.insert(64, (None, True))
    for lo in range(0, len(batch), 130):                                           # 130 (above the threshold) and the rest
        part = batch[lo:lo + 130]
        _, bad, _, flags, _ = groth16.debug_pairing_dev(ctx, engines.G1_GENERATOR * len(part), b''.join(ep.g2_std(p) for p, _ in part), None, members=True)
        assert flags == [0 if tag else 1 for _, tag in part], lo
        assert (bad != 0) == any(not tag for _, tag in part)
    members = [(p, t) for p, t in batch if t]
    _, bad, _, flags, _ = groth16.debug_pairing_dev(ctx, engines.G1_GENERATOR * len(members), b''.join(ep.g2_std(p) for p, _ in members), None, members=True)
    assert bad == 0 and flags == [0] * len(members)


# ---- the section MSMs of a key whose bases are pool points ----
@pytest.fixture(scope='module')
def edge_key(gpu, tmp_path_factory):
    import zkcensus_amd
    ctx, _ = gpu
    zk = mc.edge_key(mc.edge_key_dir(tmp_path_factory))                            # the image tests/test_00_gpu_msm_forms.py left there, if it ran
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    yield zk, pk
    pk.close()


def _section(z, which):
    """(count, standard-form bytes) of section 0 (A), 1 (B1), 2 (B2), 3 (C) of a parsed key"""
    import ctypes
    if which < 3:
        return z.nVars, mc.section_points(z, which, z.nVars)[1]
    cnt = z.nVars - z.nPublic - 1
    raw = ctypes.string_at(z.pointsC, 64 * cnt)
    return cnt, b''.join(le(ep.from_mont(int.from_bytes(raw[i:i + 32], 'little'))) for i in range(0, len(raw), 32))


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_section_msms_over_a_patched_key(gpu, edge_key, g1, g2, which):
    """zkc_msm_debug over sections whose every base is a pool point or infinity, Montgomery residues as the loader found them, equal and opposite bases throughout:
    the scalar kinds and the heavy-bucket mix against the oracle's MSM over the patched bytes; a low-window set over the first 150 points alone against Python"""
    ctx, torch = gpu
    zk, pk = edge_key
    z = ol.zkey_parse(zk)
    assert pk.n_vars == 3000
    cnt, std = _section(z, which)
    psz = 128 if which == 2 else 64
    pool = {ep.g2_std(e.point) for e in g2} if which == 2 else {ep.g1_std(e.point) for e in g1}
    pts = [std[psz * i:psz * i + psz] for i in range(cnt)]
    assert all(p in pool or not any(p) for p in pts) and len(set(pts)) > len(pool) // 2 and 20 < sum(not any(p) for p in pts) < 120
    msm = ol.msm_g2 if which == 2 else ol.msm_g1
    rng = random.Random(80 + which)
    sets = [(name, scalars_le(ss)) for name, ss in _kinds_of(cnt, rng, wires=pk.n_vars)] + [('heavy mix', mc.heavy_mix(cnt, rng))]
    low = [rng.randrange(1, 1 << 12) for _ in range(150)]
    sets.append(('low-window over 150 points', scalars_le(low + [0] * (cnt - 150))))
    got = [pk.msm_debug(which, _dev(torch, scb).data_ptr(), cnt) for _, scb in sets]
    exp = ol.pmap(lambda s: msm(std, s[1]), sets)
    for (name, _), g, e in zip(sets, got, exp):
        assert g == e, 'section %d, %s scalars' % (which, name)
    if which == 2:
        py = ep.g2_std(ep.g2_msm([ep.g2_from_std(p) for p in pts[:150]], low))
    else:
        py = ep.g1_std(ep.msm([ep.g1_from_std(p) for p in pts[:150]], low))
    assert got[-1] == py, 'section %d, the first 150 points against Python' % which
