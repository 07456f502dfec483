"""GPU: a contribution to a powers-of-tau file on the device (include/zkcensus_ptau_contribute.h, csrc/zkc_scale_each.hip).  contribute_ptau(ctx) writes the bytes of
contribute_ptau(ctx = None) and sections 2 .. 6 are tests/ptau_lib.py's at the product of the wastes: at power 5, where section 2 is 63 points, with chunks of 5, 16 and
64 points and the default (chunk edges inside a section, a chunk that is no multiple of the wave, a section in one chunk) and both kernel forms; at power 1, the smallest
file; with tau' = 1, r - 1 and on the domain; and verify_ptau_contributions(ctx) gives the host's verdicts on the chain and on three of the ways it is rejected."""
import pytest
import oracle_lib as ol
import ptau_lib as pl
import ptau_verify_lib as pv
import ptau_contrib_lib as pc
from ptau_contrib_lib import S1, S2, S3, read_sections, write_sections

pytestmark = pytest.mark.gpu
R = ol.R
SEED = bytes(range(11, 43))
W0 = (pv.TAU, pv.ALPHA, pv.BETA)


@pytest.fixture(scope='module')
def gpu():
    import zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope='module')
def power5(tmp_path_factory):
    """the source file, the host path's output and ptau_lib's expectation, once"""
    from zkcensus_amd import setup
    d = tmp_path_factory.mktemp('p5')
    src = pl.write(str(d / 's.ptau'), 5, *W0)
    host = str(d / 'host.ptau')
    h = setup.contribute_ptau(src, host, secrets=S1, name='p5')
    want = pl.sections(5, *pc.product([W0, S1]))
    got, _ = read_sections(host)
    for i in range(2, 7):
        assert got[i] == want[i], i
    return src, open(host, 'rb').read(), h


@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('chunk', [5, 16, 64, 0])
def test_device_writes_the_hosts_bytes(gpu, power5, tmp_path, chunk, form):
    from zkcensus_amd import setup
    src, host_bytes, host_hash = power5
    dst = str(tmp_path / 'd.ptau')
    h = setup.debug_contribute_ptau(src, dst, ctx=gpu, secrets=S1, name='p5', chunk_points=chunk, form=form)
    assert open(dst, 'rb').read() == host_bytes and h == host_hash
    if chunk == 0 and form == 0:
        assert setup.contribute_ptau(src, dst, ctx=gpu, secrets=S1, name='p5') == host_hash and open(dst, 'rb').read() == host_bytes
        ms = setup.ptau_contribute_stats()
        assert ms['scale_g1'] > 0 and ms['scale_g2'] > 0
        # the hook's chunk size reaches the host path as well
        assert setup.debug_contribute_ptau(src, dst, secrets=S1, name='p5', chunk_points=7) == host_hash and open(dst, 'rb').read() == host_bytes


EDGES = {'tau_one': (1, 5, 7), 'tau_minus_one': (R - 1, 5, 7), 'tau_on_domain': (pl.root_of_unity(2), 5, 7), 'alpha_is_beta': (S2[0], 99, 99)}


@pytest.mark.parametrize('edge', sorted(EDGES))
def test_edge_secrets_and_the_smallest_file(gpu, tmp_path, edge):
    from zkcensus_amd import setup
    s = EDGES[edge]
    for power in (1, 3):
        src = pl.write(str(tmp_path / ('s%d.ptau' % power)), power, *W0)
        dev, host = str(tmp_path / 'dev.ptau'), str(tmp_path / 'host.ptau')
        assert setup.contribute_ptau(src, dev, ctx=gpu, secrets=s) == setup.contribute_ptau(src, host, secrets=s)
        assert open(dev, 'rb').read() == open(host, 'rb').read()
        got, _ = read_sections(dev)
        want = pl.sections(power, *pc.product([W0, s]))
        for i in range(2, 7):
            assert got[i] == want[i], (power, i)


def test_bad_point_is_refused_with_section_and_index(gpu, tmp_path):
    import zkcensus_amd
    from zkcensus_amd import setup
    secs = pl.sections(3, *W0)
    secs[3][2 * 128 + 96] ^= 1; secs[3][6 * 128 + 96] ^= 1
    src = write_sections(tmp_path / 's.ptau', secs); dst = tmp_path / 'd.ptau'
    for chunk in (0, 3):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            setup.debug_contribute_ptau(src, str(dst), ctx=gpu, secrets=S1, chunk_points=chunk)
        assert ei.value.code == 5 and 'section 3 point 2 has a coordinate >= q, is not on the twist or is at infinity' in str(ei.value)
        assert sorted(p.name for p in tmp_path.iterdir()) == ['s.ptau']


def test_chain_verdicts_are_the_hosts(gpu, tmp_path):
    from zkcensus_amd import setup
    f = [str(tmp_path / ('f%d.ptau' % i)) for i in range(4)]
    setup.new_ptau(f[0], 3)
    for i, s in enumerate((S1, S2, S3)):
        setup.contribute_ptau(f[i], f[i + 1], ctx=gpu, secrets=s, name='c%d' % i)
    for prev, n_new in ((None, 3), (f[1], 2), (f[3], 0)):
        assert setup.verify_ptau_contributions(prev, f[3], ctx=gpu, seed=SEED) == (True, n_new, '') == setup.verify_ptau_contributions(prev, f[3], seed=SEED)
    rej = pc.rejects()
    for case in ('swap', 'tauG1', 'last_points'):
        change, words = rej[case]
        secs, order = read_sections(f[3])
        change(secs)
        bad = write_sections(tmp_path / 'bad.ptau', secs, order)
        got = setup.verify_ptau_contributions(None, bad, ctx=gpu, seed=SEED)
        assert got == setup.verify_ptau_contributions(None, bad, seed=SEED) and not got[0] and all(w in got[2] for w in words), got
