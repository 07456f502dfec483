"""GPU: the windowed fixed-base batch products zkc_g1_fixed_mul_dev / zkc_g2_fixed_mul_dev (include/zkcensus_setup.h), byte for byte.
G1 against the oracle's scalar multiplication and against the double-and-add engine zkc_g1_mul_batch_dev on the same inputs.  G2 against an affine double-and-add over
Fq2 in Python integers (tests/g2_py.py; the oracle exports no G2 product), itself pinned on 2 G2 (a constant, and the oracle's one-term G2 MSM), r G2 = infinity and
(a + b) P = a P + b P (the 257 expected points of a base share its doublings: g2_mul_many, checked against g2_mul).  One list of 257 scalars serves every size: the edge values sit at its END and a batch of n takes the last n, so every batch but n = 1 holds all
of them at lanes that change with n (wave and block edges: 63, 64, 65, 257); the expected points are computed once per base."""
import random
import pytest
import oracle_lib as ol
from g2_py import f2sub, g2_add, g2_mul, g2_mul_many, g2_bytes, g2_point, G2_TWICE

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
SIZES = [1, 63, 64, 65, 257]


def edge_scalars(w):
    """the values the kernel's digit walk can trip over, for window width w"""
    top = (R.bit_length() - 1) // w                                  # the highest window a scalar below r reaches
    mid = top // 2
    digits = [(R >> (w * j)) & ((1 << w) - 1) for j in range(top + 1)]
    all_max = ((digits[top] - 1) << (w * top)) | ((1 << (w * top)) - 1)       # below r, every digit under the top one 2^w - 1
    assert all_max < R and all(((all_max >> (w * j)) & ((1 << w) - 1)) == (1 << w) - 1 for j in range(top))
    e = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (1 << w) - 1, 1 << w, 1 << (w * mid), 1 << (w * top), ((1 << w) - 1) << (w * mid), (1 << (w * mid)) - 1,
         all_max, 1 << 253]
    assert all(0 <= k < R for k in e)
    return e


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


@pytest.fixture(scope='module')
def scalars():
    from zkcensus_amd import engines
    e = edge_scalars(engines.fixed_mul_window())
    rng = random.Random(8)
    return [rng.randrange(R) for _ in range(max(SIZES) - len(e))] + e


def _dev(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _run(gpu, fn, base, ks, width):
    ctx, torch = gpu
    d_k = _dev(torch, b''.join(k.to_bytes(32, 'little') for k in ks))
    d_out = torch.full((width * len(ks),), 0xA5, dtype=torch.uint8, device='cuda')
    fn(ctx, base, d_k.data_ptr(), len(ks), d_out.data_ptr())
    raw = d_out.cpu().numpy().tobytes()
    return [raw[width * i:width * (i + 1)] for i in range(len(ks))]


@pytest.fixture(scope='module')
def g1_bases():
    from zkcensus_amd import engines
    return {'G': engines.G1_GENERATOR, '7G': ol.g1_mul(engines.G1_GENERATOR, 7)}


@pytest.fixture(scope='module')
def g1_expected(scalars, g1_bases):
    return {name: [ol.g1_mul(b, k) for k in scalars] for name, b in g1_bases.items()}


@pytest.fixture(scope='module')
def g2_bases():
    from zkcensus_amd import engines
    return {'G': engines.G2_GENERATOR, '7G': g2_bytes(g2_mul(g2_point(engines.G2_GENERATOR), 7))}


@pytest.fixture(scope='module')
def g2_expected(scalars, g2_bases):
    return {name: [g2_bytes(p) for p in g2_mul_many(g2_point(b), scalars)] for name, b in g2_bases.items()}


def test_python_g2_reference_is_sound():
    from zkcensus_amd import engines
    G = g2_point(engines.G2_GENERATOR)
    assert g2_mul(G, 2) == G2_TWICE
    assert g2_bytes(G2_TWICE) == ol.msm_g2(engines.G2_GENERATOR, (2).to_bytes(32, 'little'))       # the oracle's MSM of one term
    assert g2_mul(G, R) is None and g2_mul(G, R - 1) == (G[0], f2sub((0, 0), G[1]))
    rng = random.Random(2)
    for _ in range(3):
        a, b = rng.randrange(R), rng.randrange(R)
        assert g2_add(g2_mul(G, a), g2_mul(G, b)) == g2_mul(G, (a + b) % R)
    ks = [rng.randrange(R) for _ in range(3)] + [0, 1, R - 1]
    assert g2_mul_many(G, ks) == [g2_mul(G, k) for k in ks]
    k = ks[0]
    assert g2_bytes(g2_mul(G, k)) == ol.msm_g2(engines.G2_GENERATOR, k.to_bytes(32, 'little'))


@pytest.mark.parametrize('base', ['G', '7G'])
@pytest.mark.parametrize('n', SIZES)
def test_g1_fixed_mul(gpu, scalars, g1_bases, g1_expected, n, base):
    from zkcensus_amd import engines
    ks = scalars[-n:]
    got = _run(gpu, engines.g1_fixed_mul, g1_bases[base], ks, 64)
    exp = g1_expected[base][-n:]
    for i in range(n):
        assert got[i] == exp[i], 'k = %x' % ks[i]
    assert got == _run(gpu, engines.g1_mul_batch, g1_bases[base], ks, 64)          # the double-and-add engine, same inputs
    if n > 1:
        assert got[ks.index(0)] == bytes(64)


@pytest.mark.parametrize('base', ['G', '7G'])
@pytest.mark.parametrize('n', SIZES)
def test_g2_fixed_mul(gpu, scalars, g2_bases, g2_expected, n, base):
    from zkcensus_amd import engines
    ks = scalars[-n:]
    got = _run(gpu, engines.g2_fixed_mul, g2_bases[base], ks, 128)
    exp = g2_expected[base][-n:]
    for i in range(n):
        assert got[i] == exp[i], 'k = %x' % ks[i]
    if n > 1:
        assert got[ks.index(0)] == bytes(128)


def test_fixed_mul_edge_arguments(gpu):
    ctx, torch = gpu
    import zkcensus_amd
    from zkcensus_amd import engines
    le = lambda x: x.to_bytes(32, 'little')
    d_k = _dev(torch, le(0) + le(5)); d_out = torch.zeros(256, dtype=torch.uint8, device='cuda')
    # scalar 0 alone: all-zero bytes, in both groups
    assert _run(gpu, engines.g1_fixed_mul, engines.G1_GENERATOR, [0], 64) == [bytes(64)]
    assert _run(gpu, engines.g2_fixed_mul, engines.G2_GENERATOR, [0], 128) == [bytes(128)]
    g2 = engines.G2_GENERATOR
    bad = [(engines.g1_fixed_mul, b'\xff' * 32 + le(2), 2),                                   # x >= q
           (engines.g1_fixed_mul, le(1) + le(Q), 2),                                          # y = q
           (engines.g1_fixed_mul, le(1) + le(3), 2),                                          # (1, 3) is not on y^2 = x^3 + 3
           (engines.g2_fixed_mul, g2[:96] + b'\xff' * 32, 2),                                 # y.c1 >= q
           (engines.g2_fixed_mul, g2[:64] + le((int.from_bytes(g2[64:96], 'little') + 1) % Q) + g2[96:], 2),      # off the twist
           (engines.g2_fixed_mul, engines.G1_GENERATOR + engines.G1_GENERATOR, 2),            # a G1 point is not on the twist
           (engines.g1_fixed_mul, engines.G1_GENERATOR, 0), (engines.g2_fixed_mul, g2, 0)]    # n = 0
    for fn, base, n in bad:
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            fn(ctx, base, d_k.data_ptr(), n, d_out.data_ptr())
        assert ei.value.code == 4                                                             # ZKC_ERR_BAD_ARG
    assert d_out.cpu().numpy().tobytes() == bytes(256)                                        # a refused call writes nothing
