"""GPU: zkc_g1_scale_dev (include/zkcensus_phase2.h), n points times ONE scalar, byte for byte.  The points are a_i G from the fixed-base engine, with the all-zero point
at index 0, at the last index and at a wave boundary; the expected value of every lane is (k a_i mod r) G from BOTH existing one-base-many-scalars engines
(zkc_g1_fixed_mul_dev, zkc_g1_mul_batch_dev), neither of which shares code with the new kernel, and for 16 sampled lanes also the CPU oracle's product of the input point.
Both coordinate forms, out of place and in place.  k = r - 2 is the one scalar whose chain meets the incomplete addition's exceptional case (csrc/zkc_phase2.hip)."""
import random
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
SIZES = [1, 63, 64, 65, 1000]
_rng = random.Random(31)
SCALARS = [1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, (1 << 253) - 1,
           int('55' * 32, 16) & ((1 << 253) - 1), int('aa' * 32, 16) & ((1 << 253) - 1)] + [_rng.randrange(1, R) for _ in range(8)]
assert all(0 < k < R for k in SCALARS) and len(SCALARS) == 19
MONT = 1 << 256


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


def _base_products(gpu, fn, ks):
    from zkcensus_amd import engines
    ctx, torch = gpu
    d_k = _dev(torch, b''.join(_le(k) for k in ks))
    d_out = torch.full((64 * len(ks),), 0xA5, dtype=torch.uint8, device='cuda')
    fn(ctx, engines.G1_GENERATOR, d_k.data_ptr(), len(ks), d_out.data_ptr())
    raw = d_out.cpu().numpy().tobytes()
    return [raw[64 * i:64 * i + 64] for i in range(len(ks))]


def _to_mont(pt):
    if pt == bytes(64): return pt
    return b''.join(_le(int.from_bytes(pt[32 * c:32 * c + 32], 'little') * MONT % Q) for c in range(2))


def _from_mont(pt):
    if pt == bytes(64): return pt
    inv = pow(MONT, -1, Q)
    return b''.join(_le(int.from_bytes(pt[32 * c:32 * c + 32], 'little') * inv % Q) for c in range(2))


def _scale(gpu, pts, k, mont, in_place):
    from zkcensus_amd import engines
    ctx, torch = gpu
    d_in = _dev(torch, b''.join(pts))
    d_out = d_in if in_place else torch.full((64 * len(pts),), 0xA5, dtype=torch.uint8, device='cuda')
    engines.g1_scale(ctx, d_in.data_ptr(), len(pts), k, d_out.data_ptr(), mont=mont)
    raw = d_out.cpu().numpy().tobytes()
    if not in_place:
        assert d_in.cpu().numpy().tobytes() == b''.join(pts)                          # the inputs are left alone
    return [raw[64 * i:64 * i + 64] for i in range(len(pts))]


@pytest.fixture(scope='module')
def multipliers():
    rng = random.Random(5)
    return [rng.randrange(1, R) for _ in range(max(SIZES))]


@pytest.mark.parametrize('n', SIZES)
def test_scale_against_both_one_base_engines(gpu, multipliers, n):
    from zkcensus_amd import engines
    a = list(multipliers[:n])
    if n > 1: a[0] = 0; a[n - 1] = 0                          # the all-zero point first and last (a batch of one keeps its finite point) ...
    if n > 64: a[64] = 0                                      # ... and at a wave boundary
    if n > 2: a[1] = 1                                        # the generator itself
    pts = _base_products(gpu, engines.g1_fixed_mul, a)
    assert n == 1 or (pts[0] == bytes(64) and pts[n - 1] == bytes(64))
    pts_m = [_to_mont(p) for p in pts]
    sample = sorted(set(random.Random(n).sample(range(n), min(n, 16)) + [0, n - 1]))
    for j, k in enumerate(SCALARS):
        want = [k * x % R for x in a]
        exp = _base_products(gpu, engines.g1_fixed_mul, want)
        assert exp == _base_products(gpu, engines.g1_mul_batch, want)
        got = _scale(gpu, pts, k, False, in_place=(j % 2 == 1))
        for i in range(n):
            assert got[i] == exp[i], 'k = %x, lane %d' % (k, i)
        got_m = _scale(gpu, pts_m, k, True, in_place=(j % 2 == 0))
        assert [_from_mont(p) for p in got_m] == exp, 'Montgomery form, k = %x' % k
        for i in sample[:16]:
            assert got[i] == (bytes(64) if a[i] == 0 else ol.g1_mul(pts[i], k)), 'oracle, k = %x, lane %d' % (k, i)


def test_scale_contract(gpu):
    import zkcensus_amd
    from zkcensus_amd import engines
    ctx, torch = gpu
    a = list(range(1, 101))
    pts = _base_products(gpu, engines.g1_fixed_mul, a)
    assert _scale(gpu, pts, 0, False, False) == [bytes(64)] * 100 and _scale(gpu, pts, 0, True, True) == [bytes(64)] * 100
    d_in = _dev(torch, b''.join(pts)); d_out = torch.zeros(6400, dtype=torch.uint8, device='cuda')

    def fails(code, d_points, n, k, out, mont=False):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            engines.g1_scale(ctx, d_points, n, k, out, mont=mont)
        assert ei.value.code == code
        return str(ei.value)
    fails(4, d_in.data_ptr(), 100, R, d_out.data_ptr())                              # k = r
    fails(4, d_in.data_ptr(), 100, (1 << 256) - 1, d_out.data_ptr())
    fails(4, None, 100, 5, d_out.data_ptr()); fails(4, d_in.data_ptr(), 100, 5, None); fails(4, d_in.data_ptr(), 0, 5, d_out.data_ptr())
    assert ctx._lib.zkc_g1_scale_dev(ctx._h, d_in.data_ptr(), 100, None, 0, d_out.data_ptr()) == 4 and ctx._lib.zkc_g1_scale_dev(None, d_in.data_ptr(), 100, _le(5), 0, d_out.data_ptr()) == 4
    # a point off the curve (y + 1) and a coordinate >= q, each at index 37 of 100, in both forms; a second bad point further on does not move the index
    for mont in (False, True):
        base = [_to_mont(q) for q in pts] if mont else list(pts)
        x37, y37 = (int.from_bytes(base[37][32 * c:32 * c + 32], 'little') for c in range(2))
        for bad37 in (_le(x37) + _le((y37 + 1) % Q), _le(x37 + Q) + _le(y37), _le(x37) + b'\xff' * 32):
            p = list(base); p[37] = bad37; p[80] = bad37
            d_bad = _dev(torch, b''.join(p))
            msg = fails(5, d_bad.data_ptr(), 100, 7, d_out.data_ptr(), mont=mont)
            assert 'point 37 ' in msg, msg
    assert d_out.cpu().numpy().tobytes() == bytes(6400)                               # a refused call writes nothing
