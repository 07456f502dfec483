"""GPU: zkc_g1_scale_each_dev / zkc_g2_scale_each_dev (include/zkcensus_ptau_contribute.h, csrc/zkc_scale_each.hip), n points EACH times its own scalar, byte for byte
against the CPU oracle (oracle_lib.g1_mul, and its one-term G2 MSM): both groups, both coordinate forms, in place and out of place, and both kernel forms through the hook
(0: the shipped windowed form, 1: bit-serial double-and-add).  Sizes around the wave; the scalars at which the signed 4-bit recoding carries through every window, where a
digit is zero and an operand of the complete addition is infinity, and k = r - 2, the one scalar whose last addition meets equal operands; the field-edge points of
tests/edge_points.py, which in G2 lie almost all outside the subgroup; one point under many scalars, many points under one scalar against zkc_g1_scale_dev; the refusals.
And n = 1000, sixteen workgroups with a partial last one, where the stride of the entry-major table and the lane split of the batched inversion are no longer those of
one or two waves: a_i G under k_i against (a_i k_i mod r) G from the fixed-base engines, the scheme of tests/test_gpu_phase2_scale.py."""
import functools, random
import pytest
import oracle_lib as ol
import edge_points as ep
import ptau_lib as pl

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
SIZES = [1, 63, 64, 65, 130]
WIDTH = {False: 64, True: 128}
GEN = {False: pl.G1_GEN, True: pl.G2_GEN}
NIB8, NIBF = int('8' * 64, 16), int('f' * 64, 16)
EDGE_SCALARS = list(dict.fromkeys([0, 1, 2, 7, 8, 9, 15, 16, 17] + [1 << k for k in (4, 32, 128, 252, 253)] + [(1 << k) - 1 for k in (4, 32, 128, 252, 253)] +
                # the recoding's carry through every window and into the top one: the nibbles 8 .. 8 and f .. f under r's top nibble, and reduced below r; 7 .. 7 and 9 .. 9 beside them
                [NIB8 & ((1 << 252) - 1), (2 << 252) | (NIB8 & ((1 << 252) - 1)), NIBF >> 4, (2 << 252) | (NIBF >> 4), NIB8 % R, NIBF % R, int('7' * 63, 16), int('9' * 63, 16)] +
                [(R - 1) // 2, (R + 1) // 2] + [R - t for t in range(1, 18)]))       # 2^4 and 2^4 - 1 are listed twice: once each
assert all(0 <= k < R for k in EDGE_SCALARS) and len(EDGE_SCALARS) == 43
CASES = [(g2, mont, in_place, form) for g2 in (False, True) for mont in (False, True) for in_place in (False, True) for form in (0, 1)]


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


def _dev(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _le(x):
    return x.to_bytes(32, 'little')


@functools.lru_cache(maxsize=None)
def oracle(g2, pt, k):
    """k * pt, standard form in and out; computed once per (point, scalar) and shared by every test and every form"""
    if not any(pt) or k == 0:
        return bytes(WIDTH[g2])
    return ol.msm_g2(pt, _le(k)) if g2 else ol.g1_mul(pt, k)


def scale(gpu, g2, pts, ks, mont, in_place, form, hook=True):
    """pts: standard form; the device sees them in the form under test, the result comes back in standard form"""
    from zkcensus_amd import engines
    ctx, torch = gpu
    w, n = WIDTH[g2], len(pts)
    src = b''.join(pl.to_mont(p) if mont else p for p in pts)
    d_in = _dev(torch, src); d_k = _dev(torch, b''.join(_le(k) for k in ks))
    d_out = d_in if in_place else torch.full((w * n,), 0xA5, dtype=torch.uint8, device='cuda')
    if hook:
        engines.debug_scale_each(ctx, g2, d_in.data_ptr(), n, d_k.data_ptr(), d_out.data_ptr(), mont=mont, form=form)
    else:
        (engines.g2_scale_each if g2 else engines.g1_scale_each)(ctx, d_in.data_ptr(), n, d_k.data_ptr(), d_out.data_ptr(), mont=mont)
    raw = d_out.cpu().numpy().tobytes()
    if not in_place:
        assert d_in.cpu().numpy().tobytes() == src                            # the inputs are left alone
    assert d_k.cpu().numpy().tobytes() == b''.join(_le(k) for k in ks)
    if mont:
        inv = pow(1 << 256, -1, Q)
        raw = b''.join(_le(int.from_bytes(raw[i:i + 32], 'little') * inv % Q) for i in range(0, len(raw), 32))
    return [raw[w * i:w * i + w] for i in range(n)]


def check(gpu, g2, pts, ks, cases=None):
    want = [oracle(g2, p, k) for p, k in zip(pts, ks)]
    for c_g2, mont, in_place, form in cases or CASES:
        if c_g2 != g2:
            continue
        got = scale(gpu, g2, pts, ks, mont, in_place, form)
        for i in range(len(pts)):
            assert got[i] == want[i], 'g2 %d mont %d in place %d form %d: lane %d, k = %x' % (g2, mont, in_place, form, i, ks[i])


@functools.lru_cache(maxsize=None)
def random_points(g2, n):
    rng = random.Random(77 + g2)
    return tuple(oracle(g2, GEN[g2], rng.randrange(1, R)) for _ in range(n))


@pytest.mark.parametrize('g2', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_random_points_and_scalars(gpu, g2, n):
    rng = random.Random(1000 + n)
    pts = list(random_points(g2, max(SIZES))[:n]); ks = [rng.randrange(R) for _ in range(n)]
    if n > 2: pts[1] = bytes(WIDTH[g2]); ks[2] = 0                            # infinity in, and infinity out
    if n > 64: pts[64] = bytes(WIDTH[g2]); ks[63] = R - 2
    check(gpu, g2, pts, ks)
    # the product calls are form 0 of the hook
    assert scale(gpu, g2, pts, ks, False, False, 0, hook=False) == [oracle(g2, p, k) for p, k in zip(pts, ks)]


@pytest.mark.parametrize('g2', [False, True])
def test_one_point_under_every_edge_scalar(gpu, g2):
    """the same point in every lane: the generator, then an edge point (in G2 one outside the subgroup), then infinity"""
    pool = ep.g2_pool() if g2 else ep.g1_pool()
    edge = (ep.g2_std if g2 else ep.g1_std)(pool[len(pool) // 2].point)
    for pt in (GEN[g2], edge):
        check(gpu, g2, [pt] * len(EDGE_SCALARS), EDGE_SCALARS)
    check(gpu, g2, [bytes(WIDTH[g2])] * len(EDGE_SCALARS), EDGE_SCALARS, cases=[(g2, True, True, 0), (g2, False, False, 1)])


@pytest.mark.parametrize('g2', [False, True])
def test_edge_points(gpu, g2):
    """every field-edge point of tests/edge_points.py under a scalar of its own, and under r - 2 and r - 1"""
    pool = ep.g2_pool() if g2 else ep.g1_pool()
    pts = [(ep.g2_std if g2 else ep.g1_std)(e.point) for e in pool]
    rng = random.Random(9)
    cases = [(g2, True, False, 0), (g2, False, True, 0), (g2, True, True, 1)]
    check(gpu, g2, pts, [rng.randrange(1, R) for _ in pts], cases)
    check(gpu, g2, pts, [R - 2 if i % 2 else R - 1 for i in range(len(pts))], cases)


@pytest.mark.parametrize('g2', [False, True])
def test_a_thousand_points_against_the_fixed_base_engines(gpu, g2):
    """P_i = a_i G from the fixed-base engine, k_i full-width: every lane must be (a_i k_i mod r) G from that engine, which shares no code with the kernel; 16 sampled
    lanes and the special ones also against the oracle's product of the input point.  Infinity in and the scalars 0, 1, r - 2 sit at index 0, at index 999 and at both
    edges of a wave."""
    n, w = 1000, WIDTH[g2]
    ctx, _ = gpu
    rng = random.Random(4000 + g2)
    a = [rng.randrange(1, R) for _ in range(n)]; ks = [rng.randrange(1, R) for _ in range(n)]
    for i in (0, 64, 191, 999): a[i] = 0                                      # the all-zero point first, last, in the first and in the last lane of a wave
    for i, k in ((1, 0), (2, 1), (3, R - 2), (63, R - 2), (127, 0), (128, 1), (192, R - 2), (960, 0), (996, R - 2), (997, 1), (998, 0), (999, R - 2)): ks[i] = k
    special = [0, 1, 2, 3, 63, 64, 127, 128, 191, 192, 960, 996, 997, 998, 999]
    raw = pl._points_gpu(ctx, w, a)
    pts = [raw[w * i:w * i + w] for i in range(n)]
    assert all(pts[i] == bytes(w) for i in (0, 64, 191, 999)) and pts[1] != bytes(w)
    raw = pl._points_gpu(ctx, w, [x * k % R for x, k in zip(a, ks)])
    want = [raw[w * i:w * i + w] for i in range(n)]
    for i in sorted(set(random.Random(n).sample(range(n), 16) + special)):
        assert want[i] == oracle(g2, pts[i], ks[i]), 'the expectation itself, lane %d' % i
    runs = [(mont, in_place, 0, True) for mont in (False, True) for in_place in (False, True)] + [(True, False, 0, False)] + ([] if g2 else [(True, True, 1, True)])
    for mont, in_place, form, hook in runs:
        got = scale(gpu, g2, pts, ks, mont, in_place, form, hook=hook)
        for i in range(n):
            assert got[i] == want[i], 'g2 %d mont %d in place %d form %d hook %d: lane %d, k = %x' % (g2, mont, in_place, form, hook, i, ks[i])


def test_many_points_under_one_scalar_against_the_one_scalar_engine(gpu):
    from zkcensus_amd import engines
    ctx, torch = gpu
    pts = list(random_points(False, max(SIZES))); n = len(pts)
    pts[5] = bytes(64)
    for k in (R - 2, 12345, (1 << 253) + 9, EDGE_SCALARS[20]):
        d_in = _dev(torch, b''.join(pts)); d_out = torch.zeros(64 * n, dtype=torch.uint8, device='cuda')
        engines.g1_scale(ctx, d_in.data_ptr(), n, k, d_out.data_ptr())
        raw = d_out.cpu().numpy().tobytes()
        want = [raw[64 * i:64 * i + 64] for i in range(n)]
        for form in (0, 1):
            assert scale(gpu, False, pts, [k] * n, False, False, form) == want, hex(k)


@pytest.mark.parametrize('g2', [False, True])
def test_refusals(gpu, g2):
    import zkcensus_amd
    from zkcensus_amd import engines
    ctx, torch = gpu
    w, n = WIDTH[g2], 100
    pts = list(random_points(g2, max(SIZES))[:n]); ks = [5 + i for i in range(n)]
    fn = engines.g2_scale_each if g2 else engines.g1_scale_each
    d_in = _dev(torch, b''.join(pts)); d_k = _dev(torch, b''.join(_le(k) for k in ks)); d_out = torch.zeros(w * n, dtype=torch.uint8, device='cuda')

    def fails(code, *a, **kw):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            fn(ctx, *a, **kw)
        assert ei.value.code == code
        return str(ei.value)
    fails(4, None, n, d_k.data_ptr(), d_out.data_ptr()); fails(4, d_in.data_ptr(), n, None, d_out.data_ptr()); fails(4, d_in.data_ptr(), n, d_k.data_ptr(), None)
    fails(4, d_in.data_ptr(), 0, d_k.data_ptr(), d_out.data_ptr())
    # a scalar = r at index 41 (and again at 90: the smallest index is named), in both kernel forms
    bad_k = list(ks); bad_k[41] = R; bad_k[90] = (1 << 256) - 1
    d_bk = _dev(torch, b''.join(_le(k) for k in bad_k))
    assert 'element 41 ' in fails(5, d_in.data_ptr(), n, d_bk.data_ptr(), d_out.data_ptr())
    for form in (0, 1):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            engines.debug_scale_each(ctx, g2, d_in.data_ptr(), n, d_bk.data_ptr(), d_out.data_ptr(), form=form)
        assert ei.value.code == 5 and 'element 41 ' in str(ei.value)
    # a point off its curve (y + 1) and a coordinate >= q, each at index 37, in both coordinate forms; a second bad point further on does not move the index
    for mont in (False, True):
        base = [pl.to_mont(p) for p in pts] if mont else list(pts)
        c = [int.from_bytes(base[37][32 * j:32 * j + 32], 'little') for j in range(w // 32)]
        off = list(c); off[-1] = (off[-1] + 1) % Q
        big = list(c); big[0] += Q
        for bad37 in (b''.join(_le(v) for v in off), b''.join(_le(v) for v in big), base[37][:w - 32] + b'\xff' * 32):
            p = list(base); p[37] = bad37; p[80] = bad37
            d_bad = _dev(torch, b''.join(p))
            assert 'element 37 ' in fails(5, d_bad.data_ptr(), n, d_k.data_ptr(), d_out.data_ptr(), mont=mont)
    assert d_out.cpu().numpy().tobytes() == bytes(w * n)                      # a refused call writes nothing
    # in place: a refused call leaves the points as they were
    p = list(pts); p[3] = p[3][:w - 32] + _le((int.from_bytes(p[3][w - 32:], 'little') + 1) % Q)
    d_p = _dev(torch, b''.join(p))
    assert 'element 3 ' in fails(5, d_p.data_ptr(), n, d_k.data_ptr(), d_p.data_ptr())
    assert d_p.cpu().numpy().tobytes() == b''.join(p)
