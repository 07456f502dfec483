"""GPU: is a powers-of-tau file the powers of one tau?  (include/zkcensus_ptau_verify.h, csrc/zkc_ptau_verify.hip).  The two engines -- (sum w_i P_i, sum w_i P_(i+1)) over
consecutive points -- are held against tests/edge_points.py's plain affine sums in Python: at every count of terms at which the kernels take another path (a segment is 16
terms, a workgroup 64 segments, a reduction step sums 32 partial sums: 16, 1024, 512 and 16384 terms are the boundaries, each with a value at either side), with weights
random, 0, 1, 2^128 - 1 and all equal, over generic points, one point repeated, P and -P alternating (partial sums return to infinity), infinities inside, and in G2 a twist
point outside G2 (the additions are complete on the whole twist), with mont 0 and 1.  Then the file: the verdicts of tests/test_ptau_verify_cpu.py at powers 1, 3 and 6 on
the device, the device's sums byte for byte the host threads', and from_ptau(verify=True)."""
import os, random
import pytest
import oracle_lib as ol
import g2_py
import edge_points as ep
import ptau_lib as pl
import ptau_prep_lib as pp
import ptau_verify_lib as pv

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
SEED = bytes(range(7, 39))
SEG, WAVE, RED = 16, 64, 32                                    # csrc/zkc_ptau_verify.hip SEG, the lanes of a workgroup, csrc/zkc_point_red.h POINT_RED
TERMS = sorted({1, 2, 3, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097} | {b + d for b in (SEG, SEG * RED, SEG * WAVE, SEG * RED * RED) for d in (-1, 0, 1)})
FULL_MSM_UP_TO = 65                                            # terms up to which the reference is the sum over every term; above, equal points are collected first
MAXW = (1 << 128) - 1


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    import zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield {'ctx': ctx, 'dir': tmp_path_factory.mktemp('ptau_verify')}
    ctx.close()


# ---- the engines ----
_points = {}


def generator_multiples(ctx, width, count):
    """(k_i, k_i G as Python points -- the first FULL_MSM_UP_TO + 1 of them, None beyond: the long sets are only used through their exponents --, the standard-form bytes)
    for the same seeded k_i at every count, from the fixed-base engines"""
    if width not in _points:
        rng = random.Random(900 + width)
        ks = [rng.randrange(1, R) for _ in range(max(TERMS) + 1)]
        raw = pl._points_gpu(ctx, width, ks)
        dec = ep.g1_from_std if width == 64 else ep.g2_from_std
        _points[width] = (ks, raw, [dec(raw[width * i:width * i + width]) for i in range(FULL_MSM_UP_TO + 1)])
    ks, raw, pts = _points[width]
    return ks[:count], (pts + [None] * count)[:count], raw[:width * count]


def weight_kinds(nt, seed):
    rng = random.Random(seed); same = rng.getrandbits(128) | 1
    edge = [0, 1, MAXW, 1 << 127, 2, (1 << 64) - 1, 1 << 64, rng.getrandbits(128)]
    return {'random': [rng.getrandbits(128) for _ in range(nt)], 'zero': [0] * nt, 'one': [1] * nt, 'max': [MAXW] * nt, 'equal': [same] * nt,
            'edges': [edge[(i * 5 + i // 8) % len(edge)] for i in range(nt)]}


def collected(msm_, pts, ws):
    """sum w_i P_i with the weights of equal points added up first (as integers: no reduction, the twist points outside G2 have another order than r; the sums stay below
    2^144 < r, so edge_points' own reduction mod r changes nothing either)"""
    d = {}
    for p, w in zip(pts, ws):
        if p is not None and w:
            d[p] = d.get(p, 0) + w
    assert len(d) <= FULL_MSM_UP_TO + 1 and all(w < R for w in d.values())
    return msm_(list(d), list(d.values()))


def on_device(b):
    import numpy as np, torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def run_engine(ctx, width, d_points, n, ws, mont):
    import torch
    from zkcensus_amd import engines
    assert len(ws) == n - 1
    d_w = on_device(pv.w16(ws))
    before = d_points.clone()
    out = (engines.g1_wsum_pair if width == 64 else engines.g2_wsum_pair)(ctx, d_points.data_ptr(), n, d_w.data_ptr(), mont=mont)
    assert torch.equal(d_points, before)                        # the input is left alone
    return out


def point_sets(ctx, width, nt):
    """name -> (the nt + 1 points as Python objects, their bytes in standard form, their exponents or None).  The sets without exponents hold few distinct points"""
    enc, neg = (ep.g1_std, ep.neg) if width == 64 else (ep.g2_std, g2_py.g2_neg)
    ks, pts, raw = generator_multiples(ctx, width, nt + 1)
    P = pts[0]
    as_bytes = lambda ps: b''.join(enc(p) for p in ps)
    alt = [P if i % 2 == 0 else neg(P) for i in range(nt + 1)]
    holes = {0, 1, nt // 2, nt} if nt > 3 else {nt % 2}
    sets = {'generic': (pts, raw, ks), 'same': ([P] * (nt + 1), enc(P) * (nt + 1), None), 'alternating': (alt, as_bytes(alt), None),
            'infinities': ([None if i in holes else p for i, p in enumerate(pts)], b''.join(bytes(width) if i in holes else raw[width * i:width * i + width] for i in range(nt + 1)),
                           [0 if i in holes else k for i, k in enumerate(ks)])}
    if width == 128:
        T = g2_py.small_order_point(); O = next(e.point for e in ep.g2_pool() if not e.in_g2)
        assert not g2_py.in_g2(T) and g2_py.on_twist(O)
        cyc = [T, pts[1], O, g2_py.g2_neg(T), T, P]
        tw = [cyc[i % len(cyc)] for i in range(nt + 1)]
        sets['twist-outside-g2'] = (tw, as_bytes(tw), None)
    return sets


@pytest.mark.parametrize('width', [64, 128])
@pytest.mark.parametrize('nt', TERMS)
def test_engine_is_the_pair_of_sums(env, nt, width):
    """The reference is edge_points' affine sum in Python: over every term for the generic sets up to FULL_MSM_UP_TO terms (with random, edge and zero weights: an affine
    addition in Python is not free), over the few distinct points of the other sets with the weights of equal points added up, at every size and with every kind of
    weight; the generic sets above FULL_MSM_UP_TO terms go through their exponents: (sum w_i k_i) G"""
    ctx = env['ctx']
    msm_, enc, gen = (ep.msm, ep.g1_std, (1, 2)) if width == 64 else (ep.g2_msm, ep.g2_std, g2_py.g2_point(pl.G2_GEN))
    kinds = weight_kinds(nt, 1000 * nt + width)
    for sname, (pts, raw, ks) in point_sets(ctx, width, nt).items():
        d_pts = {False: on_device(raw), True: on_device(pl.to_mont(raw))}
        by_terms = ks is None or nt <= FULL_MSM_UP_TO
        for wname in (['random', 'edges', 'zero'] if ks is not None and by_terms else list(kinds)):
            ws = kinds[wname]
            if by_terms:
                exp = (collected(msm_, pts[:-1], ws), collected(msm_, pts[1:], ws))
            else:
                exp = tuple(msm_([gen], [sum(w * k for w, k in zip(ws, ks[off:off + nt])) % R]) for off in (0, 1))
            exp = (enc(exp[0]), enc(exp[1]))
            for mont in (False, True):
                got = run_engine(ctx, width, d_pts[mont], nt + 1, ws, mont)
                assert got == exp, '%s, weights %s, %d terms, mont %s: %s differ' % (sname, wname, nt, mont, [k for k in (0, 1) if got[k] != exp[k]])


@pytest.mark.parametrize('width', [64, 128])
def test_engine_refuses_bad_points_and_arguments(env, width):
    import numpy as np, torch
    from zkcensus_amd import engines, _native
    ctx = env['ctx']; n = 100
    eng = engines.g1_wsum_pair if width == 64 else engines.g2_wsum_pair
    _, _, good = generator_multiples(ctx, width, n)
    d_w = on_device(pv.w16([3] * (n - 1)))
    for mont in (False, True):
        src = bytearray(pl.to_mont(good) if mont else good)
        src[width * 77 + 1] ^= 1                                     # off the curve
        src[width * 40 + width - 32:width * 40 + width] = Q.to_bytes(32, 'little')      # a coordinate = q, at the smaller index
        d_in = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).cuda()
        with pytest.raises(_native.ZkcError) as ei:
            eng(ctx, d_in.data_ptr(), n, d_w.data_ptr(), mont=mont)
        assert ei.value.code == 5 and 'point 40 has a coordinate >= q or is not on the ' + ('curve' if width == 64 else 'twist') in str(ei.value)
    d = torch.zeros(2 * width, dtype=torch.uint8, device='cuda')
    for args in ((0, 2, d_w.data_ptr()), (d.data_ptr(), 2, 0), (d.data_ptr(), 1, d_w.data_ptr()), (d.data_ptr(), 0, d_w.data_ptr())):      # NULL pointers, fewer than two points
        with pytest.raises(_native.ZkcError) as ei:
            eng(ctx, *args)
        assert ei.value.code == 4
    assert eng(ctx, d.data_ptr(), 2, d_w.data_ptr()) == (bytes(width), bytes(width))      # two infinities: infinity


# ---- the file ----
def write(env, name, img):
    p = str(env['dir'] / name); open(p, 'wb').write(img)
    return p


@pytest.mark.parametrize('waste', pv.WASTE_NAMES)
@pytest.mark.parametrize('power', [1, 3, 6])
def test_every_waste_is_a_valid_file_on_the_device(env, power, waste):
    from zkcensus_amd import setup
    ctx = env['ctx']
    unprepared, expected, _ = pp.images(power, pp.wastes(power)[waste], ctx)
    for img in (unprepared, expected):
        path = write(env, 'f.ptau', img)
        assert setup.verify_ptau(path, ctx=ctx, seed=SEED) == (True, 0, 0, 0, '')
        assert setup.verify_ptau(path, ctx=ctx) == (True, 0, 0, 0, '')
    ms = setup.ptau_verify_stats()
    assert all(v > 0 for v in ms.values()), ms


@pytest.mark.parametrize('power', [1, 3, 6])
def test_each_check_fires_on_the_device(env, power):
    from zkcensus_amd import setup
    ctx = env['ctx']
    muts = pv.mutations(power)
    for name in (pv.POWER_1_MUTATIONS if power == 1 else sorted(muts)):
        change, check, section, index = muts[name]
        secs = pv.monomial(power, pp.PLAIN, ctx)
        change(secs)
        path = write(env, 'm.ptau', pl.assemble(secs))
        got = setup.verify_ptau(path, ctx=ctx, seed=SEED)
        assert got[:2] == (False, check), (name, got)
        if section is not None:
            assert got[2] == section, (name, got)
        if index is not None:
            assert got[3] == index, (name, got)
        assert got == setup.verify_ptau(path, seed=SEED), name      # and the host threads say the same, to the letter


@pytest.mark.parametrize('power', [3, 6])
def test_device_sums_are_the_host_sums(env, power):
    """the 126 terms of section 2 at power 6 are four segments; the chunk sizes 1, 7 and 64 cut them into 126, 18 and 2 chunks that share one point each"""
    from zkcensus_amd import setup
    ctx = env['ctx']
    for waste in ('plain', 'minus-one', 'on-domain'):
        w = pp.wastes(power)[waste]
        path = write(env, 's.ptau', pp.images(power, w, ctx)[0])
        for wname, ws in pv.weight_sets(power).items():
            if power == 6 and waste != 'plain' and wname not in ('random', 'ones'):
                continue
            host_verdict, host = setup.debug_verify_ptau(path, pv.w16(ws))
            if power == 3:
                assert host == pv.expected_sums(power, w, ws), (waste, wname)
            # chunks of one term are a few hundred rounds of launches at power 6: once there, with the honest file and random weights
            for chunk in ((0, 1, 7, 64) if power == 3 or (waste, wname) == ('plain', 'random') else (0, 7, 64)):
                verdict, sums = setup.debug_verify_ptau(path, pv.w16(ws), ctx=ctx, chunk_terms=chunk)
                assert [k for k in range(0, 640, 64) if sums[k:k + 64] != host[k:k + 64]] == [] and verdict == host_verdict, (waste, wname, chunk)


def test_from_ptau_with_verify_on_the_device(env):
    from zkcensus_amd import setup, _native
    ctx, d = env['ctx'], env['dir']
    power = 3
    r = pl.write_r1cs(str(d / 'tiny.r1cs'), *pv.TINY_CIRCUIT)
    hole = setup.prepare_ptau(write(env, 'hole_u.ptau', pl.assemble(pv.hole_sections(power, ctx))), str(d / 'hole.ptau'), ctx=ctx)
    assert setup.check_prepared(hole, ctx=ctx) == (True, 0, 0, '')
    setup.from_ptau(r, hole, d / 'hole.zkey', None, ctx=ctx)                                # the hole: accepted
    with pytest.raises(_native.ZkcError) as ei:
        setup.from_ptau(r, hole, d / 'never.zkey', d / 'never.json', ctx=ctx, verify=True)
    assert ei.value.code == 5 and 'section 2 is not the powers of one tau: sameRatio(R1, R2; G2, tauG2[1]) fails' in str(ei.value)
    assert not (d / 'never.zkey').exists() and not (d / 'never.json').exists()
    good = setup.prepare_ptau(write(env, 'good_u.ptau', pp.images(power, pp.PLAIN, ctx)[0]), str(d / 'good.ptau'), ctx=ctx)
    setup.from_ptau(r, good, d / 'a.zkey', d / 'a.json', ctx=ctx)
    setup.from_ptau(r, good, d / 'b.zkey', d / 'b.json', ctx=ctx, verify=True)
    assert open(d / 'a.zkey', 'rb').read() == open(d / 'b.zkey', 'rb').read() and open(d / 'a.json', 'rb').read() == open(d / 'b.json', 'rb').read()
