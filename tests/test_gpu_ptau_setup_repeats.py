"""GPU: keys from a prepared powers-of-tau file on the device for the circuit of tests/repeat_circuits.py, whose rows repeat one point: every exceptional addition of
csrc/zkc_point_ops.h in BOTH groups -- add_point's doubling (P + P) and its return to infinity (P - P) in zkc_ptau_acc, lean additions onto what the doubling left, equal
products of two scale jobs -- equal and opposite partial sums in zkc_ptau_red at the first, second and third reduction step, rows of 32 767, 32 768 and 32 769 terms
(1024 segments against 1025: two steps against three) beside rows of 0 and 1 partial sums, and both sides of the sign rule of Builder::add.  The B side of a constraint is
the G2 row, so each shape goes through G1Ops and G2Ops alike.  The device key must be the host key (pinned by tests/test_ptau_setup_repeats_cpu.py), and every wire's four
points the CPU oracle's multiple of its exponent.  Three wastes: plain, alpha = beta (the K rows double once more), and tau the root of unity at which L_LONG = 1: the long
rows then sum the generator itself and every other point of the file is infinity.  One device and one host from_ptau per waste."""
import time
import pytest
import oracle_lib as ol
import ptau_lib as pl
import repeat_circuits as rc

pytestmark = pytest.mark.gpu
R = ol.R
TAU, ALPHA, BETA = 0x3c6ef372fe94f82ba54ff53a5f1d36f1510e527fade682d19b05688c2b3e6c1f % R, 0x1f83d9abfb41bd6b5be0cd19137e2179cbbb9d5dc1059ed8629a292a367cd507 % R, 0x9159015a3070dd17152fecd8f70e593967332667ffc00b318eb44a8768581511 % R
WASTES = {'plain': (TAU, ALPHA, BETA), 'alpha=beta': (TAU, ALPHA, ALPHA), 'tau=root': (pow(pl.root_of_unity(rc.POWER), rc.LONG, R), ALPHA, BETA)}


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    import zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    d = tmp_path_factory.mktemp('repeats')
    yield {'ctx': ctx, 'dir': d, 'r1cs': rc.write(str(d / 'repeats.r1cs'))}
    ctx.close()


@pytest.fixture(scope='module', params=list(WASTES))
def keys(request, env):
    from zkcensus_amd import setup
    d, i = env['dir'], list(WASTES).index(request.param)
    waste = WASTES[request.param]
    ptau = pl.write(str(d / ('w%d.ptau' % i)), rc.POWER, *waste, ctx=env['ctx'])
    hz, hv, dz, dv = [str(d / ('w%d_%s' % (i, x))) for x in ('h.zkey', 'h.json', 'd.zkey', 'd.json')]
    t0 = time.perf_counter()
    setup.from_ptau(env['r1cs'], ptau, dz, dv, ctx=env['ctx'])
    t1 = time.perf_counter()
    dev_ms = setup.ptau_stats()
    setup.from_ptau(env['r1cs'], ptau, hz, hv)
    print('%s: device from_ptau %.0f ms %r, host from_ptau %.0f ms' % (request.param, 1e3 * (t1 - t0), dev_ms, 1e3 * (time.perf_counter() - t1)))
    return {'name': request.param, 'waste': waste, 'files': (hz, hv, dz, dv), 'dev_ms': dev_ms}


def same_files(hz, hv, dz, dv):
    a, b = pl.zkey_sections(open(hz, 'rb').read()), pl.zkey_sections(open(dz, 'rb').read())
    for s in range(1, 11):
        assert a[s] == b[s], 'section %d of the device key differs from the host key' % s
    assert open(hz, 'rb').read() == open(dz, 'rb').read() and open(hv, 'rb').read() == open(dv, 'rb').read()


def test_every_wire_on_the_device_is_its_exponent_times_the_generator(keys):
    """independent of the host path: the exponents are summed over terms in Python, the points are the CPU oracle's"""
    s = pl.zkey_sections(open(keys['files'][2], 'rb').read())
    A, B, K = rc.exponents(*keys['waste'])
    assert len(s[5]) == 64 * rc.N_WIRES and len(s[6]) == 64 * rc.N_WIRES and len(s[7]) == 128 * rc.N_WIRES and len(s[8]) == 64 * (rc.N_WIRES - 1)
    wrong = []
    for w in range(rc.N_WIRES):
        got, want = rc.key_points(s, w), rc.oracle_points(A, B, K, w)
        wrong += [('wire %d' % w if w == 0 else [n for n in rc.WIRE if rc.WIRE[n] == w][0], sec) for sec, g, e in zip(('A', 'B1', 'B2', 'K'), got, want) if g != e]
    assert wrong == []
    for name in rc.ZERO_ROWS:
        assert rc.key_points(s, rc.WIRE[name]) == (bytes(64), bytes(64), bytes(128), bytes(64)), name
    long_rows = [n for n, terms in rc.CASES if any(c == rc.LONG for c, _, _ in terms)]
    assert set(long_rows) == {'red_eq', 'red_eq2', 'red3_eq', 'red3_lo', 'red3_at', 'red3_hi'}
    for name, w in rc.WIRE.items():
        if keys['name'] == 'tau=root':                           # the long rows are multiples of the generator, every other row is infinity
            assert (A[w] != 0) == (name in long_rows) and (name in long_rows or not any(b''.join(rc.key_points(s, w)))), name
        else:
            assert (A[w] != 0 and B[w] != 0 and K[w] != 0) == (name not in rc.ZERO_ROWS), name
    if keys['name'] == 'tau=root':
        assert A[rc.WIRE['red3_eq']] == 65536 and A[rc.WIRE['red_eq2']] == 2048 and A[rc.WIRE['red_eq']] == 64 and A[rc.WIRE['red3_hi']] == 2 * 8192


def test_device_key_equals_host_key(keys):
    same_files(*keys['files'])


def test_every_stage_was_timed(keys):
    assert all(v > 0 for v in keys['dev_ms'].values()), keys['dev_ms']
