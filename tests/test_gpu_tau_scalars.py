"""GPU: zkc_tau_scalars (csrc/zkc_scale_each.hip) BY VALUE through the hook zkc_debug_tau_scalars_dev (include/zkcensus_ptau_contribute.h): out[i] = mult * tau^(first + i)
mod r against Python integers, every lane of every case.  A contribution at the powers the suite can afford reads six rows of the 32-row table tau^(2^k) in one
workgroup; here the exponents start at the product's chunk edge (2^20), end where power 28 ends (2^29 - 2), cross bit 31 inside a batch and end at 2^32 - 1, where every
row is read at once, over one lane, a workgroup less one, a workgroup, one more, and four workgroups with a partial last one.  The hook fills the table and launches the
kernel with the two functions a contribution uses."""
import pytest
import oracle_lib as ol
import ptau_lib as pl
from ptau_contrib_lib import S1

pytestmark = pytest.mark.gpu
R = ol.R
FIRST = {'0': lambda n: 0, '1': lambda n: 1, '255': lambda n: 255, '2^20-1': lambda n: (1 << 20) - 1, '2^20': lambda n: 1 << 20,
         '2^29-2-n': lambda n: (1 << 29) - 2 - n,              # the last exponents of a file of power 28
         '2^31-3': lambda n: (1 << 31) - 3,                    # bit 31 turns on inside the batch
         '2^32-n': lambda n: (1 << 32) - n}                    # the last lane reads every row of the table
TAU = {'one': 1, 'minus_one': R - 1, 'two': 2, 'full': S1[0], 'root28': pl.root_of_unity(28)}      # root28: the powers wrap round the largest domain
MULT = {'one': 1, 'minus_one': R - 1, 'full': S1[1]}
# (n, first, tau, mult): every value of an axis meets at least two values of every other axis (asserted below)
CASES = [(1, '0', 'one', 'minus_one'), (256, '0', 'root28', 'full'), (256, '1', 'one', 'minus_one'), (1000, '1', 'full', 'one'),
         (255, '255', 'full', 'full'), (256, '255', 'one', 'one'), (255, '2^20-1', 'minus_one', 'minus_one'), (1000, '2^20-1', 'root28', 'full'),
         (257, '2^20', 'minus_one', 'one'), (1000, '2^20', 'full', 'minus_one'), (1, '2^29-2-n', 'one', 'minus_one'), (1000, '2^29-2-n', 'minus_one', 'full'),
         (257, '2^29-2-n', 'root28', 'one'), (1, '2^31-3', 'two', 'full'), (255, '2^31-3', 'full', 'minus_one'), (1000, '2^31-3', 'full', 'full'),
         (257, '2^32-n', 'two', 'minus_one'), (1000, '2^32-n', 'root28', 'one')]
for _a, _values in enumerate(([1, 255, 256, 257, 1000], list(FIRST), list(TAU), list(MULT))):
    for _b in range(4):
        for _v in _values:
            assert _a == _b or len({c[_b] for c in CASES if c[_a] == _v}) >= 2, (_a, _v, _b)


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


def scalars(gpu, tau, mult, first, n):
    from zkcensus_amd import engines
    ctx, torch = gpu
    d_out = torch.full((32 * n + 32,), 0xA5, dtype=torch.uint8, device='cuda')
    engines.debug_tau_scalars(ctx, tau, mult, first, n, d_out.data_ptr())
    raw = d_out.cpu().numpy().tobytes()
    assert raw[32 * n:] == b'\xa5' * 32                                      # nothing behind the last lane
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(n)]


@pytest.mark.parametrize('n,first,tau,mult', CASES)
def test_scalars_by_value(gpu, n, first, tau, mult):
    f, t, m = FIRST[first](n), TAU[tau], MULT[mult]
    assert 0 <= f and f + n <= 1 << 32
    got = scalars(gpu, t, m, f, n)
    for i in range(n):
        assert got[i] == m * pow(t, f + i, R) % R, 'lane %d: exponent %d = 0x%x' % (i, f + i, f + i)


def test_refusals(gpu):
    import zkcensus_amd
    from zkcensus_amd import engines
    ctx, torch = gpu
    d_out = torch.full((32 * 1000,), 0xA5, dtype=torch.uint8, device='cuda')

    def refused(tau, mult, first, n, out=d_out.data_ptr()):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            engines.debug_tau_scalars(ctx, tau, mult, first, n, out)
        assert ei.value.code == 4
        return str(ei.value)
    # the table serves 32 bits of exponent: first + n = 2^32 + 1 is one lane too many, from either side
    assert 'first + n exceeds 2^32' in refused(3, 5, (1 << 32) - 999, 1000)
    refused(3, 5, 1 << 32, 1); refused(3, 5, (1 << 32) + 7, 1); refused(3, 5, (1 << 64) - 1, 2)
    refused(3, 5, 0, 0); refused(3, 5, 0, 10, out=None)
    for bad in (0, R):
        assert 'must be in [1, r)' in refused(bad, 5, 0, 10)
        assert 'must be in [1, r)' in refused(3, bad, 0, 10)
    assert ctx._lib.zkc_debug_tau_scalars_dev(ctx._h, None, ol.le32(5), 0, 10, d_out.data_ptr()) == 4
    assert ctx._lib.zkc_debug_tau_scalars_dev(ctx._h, ol.le32(3), None, 0, 10, d_out.data_ptr()) == 4
    assert ctx._lib.zkc_debug_tau_scalars_dev(None, ol.le32(3), ol.le32(5), 0, 10, d_out.data_ptr()) == 4
    assert d_out.cpu().numpy().tobytes() == b'\xa5' * 32000                   # a refused call writes nothing
    # and the largest batch that is allowed ends at 2^32 - 1
    assert scalars(gpu, 3, 5, (1 << 32) - 1, 1) == [5 * pow(3, (1 << 32) - 1, R) % R]
