"""GPU: a contribution to a powers-of-tau file on the device (include/zkcensus_ptau_contribute.h, csrc/zkc_scale_each.hip).  contribute_ptau(ctx) writes the bytes of
contribute_ptau(ctx = None) and sections 2 .. 6 are tests/ptau_lib.py's at the product of the wastes: at power 5, where section 2 is 63 points, with chunks of 5, 16 and
64 points and the default (chunk edges inside a section, a chunk that is no multiple of the wave, a section in one chunk) and both kernel forms; at power 1, the smallest
file; with tau' = 1, r - 1 and on the domain; and verify_ptau_contributions(ctx) gives the host's verdicts on the chain and on three of the ways it is rejected.
Past one wave: power 9, where section 2 is 1023 points (four workgroups of the scalar kernel, exponent bits 0 .. 9), in one chunk and in chunks of 300; power 2 in chunks
of 1 and 2 points, where the record's own points come from a later chunk or from a chunk's last lane; a chain of two device contributions at power 9 and files changed
far from the front; and every forgery of tests/ptau_contrib_lib.py: forgeries() with the host's verdict and reason."""
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


# ---- one forgery per check: the device's verdicts are the host's ----
def test_forged_chains_get_the_hosts_verdicts(gpu, tmp_path):
    from zkcensus_amd import setup
    secs, _ = pc.make_chain(3, [S1, S2, S3])
    first_secs, _ = pc.make_chain(3, [S1])
    last, first = write_sections(tmp_path / 'py3.ptau', secs), write_sections(tmp_path / 'py1.ptau', first_secs)
    assert setup.verify_ptau_contributions(None, last, ctx=gpu, seed=SEED) == (True, 3, '')
    assert setup.verify_ptau_contributions(first, last, ctx=gpu, seed=SEED) == (True, 2, '')
    table = pc.forgeries(3, [S1, S2, S3])
    assert len(table) == 18
    for case in sorted(table):
        change_next, change_prev, words = table[case]
        nsecs = {i: bytearray(b) for i, b in secs.items()}
        change_next(nsecs)
        bad, prev = write_sections(tmp_path / 'bad.ptau', nsecs), None
        if change_prev:
            psecs = {i: bytearray(b) for i, b in first_secs.items()}
            change_prev(psecs)
            prev = write_sections(tmp_path / 'prev.ptau', psecs)
        got = setup.verify_ptau_contributions(prev, bad, ctx=gpu, seed=SEED)
        assert got == setup.verify_ptau_contributions(prev, bad, seed=SEED) and not got[0] and all(w in got[2] for w in words), (case, got)


# ---- past one wave ----
@pytest.fixture(scope='module')
def power9(gpu, tmp_path_factory):
    """the source file, the fixed-base expectation of sections 2 .. 6 at the product of the wastes, and the host path's output and hash, once"""
    from zkcensus_amd import setup
    d = tmp_path_factory.mktemp('p9')
    src = pl.write(str(d / 's.ptau'), 9, *W0, ctx=gpu)
    sc = pl.section_scalars(9, *pc.product([W0, S1]))
    want = {i: pl.to_mont(pl._points_gpu(gpu, pl.PT_BYTES[i], sc[i])) for i in range(2, 7)}
    assert [len(want[i]) for i in range(2, 7)] == [1023 * 64, 512 * 128, 512 * 64, 512 * 64, 128]
    host = str(d / 'host.ptau')
    h = setup.contribute_ptau(src, host, secrets=S1, name='p9')
    return src, want, open(host, 'rb').read(), h


@pytest.mark.parametrize('chunk', [0, 300])
def test_power_9_by_value(gpu, power9, tmp_path, chunk):
    """chunk 300: first = 300, 600, 900 and a last chunk of 123 points in section 2 (212 in the others), none a multiple of the wave or of the workgroup"""
    from zkcensus_amd import setup
    src, want, host_bytes, host_hash = power9
    dst = str(tmp_path / 'd.ptau')
    h = setup.debug_contribute_ptau(src, dst, ctx=gpu, secrets=S1, name='p9', chunk_points=chunk) if chunk else setup.contribute_ptau(src, dst, ctx=gpu, secrets=S1, name='p9')
    got, order = read_sections(dst)
    assert order == [1, 2, 3, 4, 5, 6, 7]
    for i in range(2, 7):
        if got[i] != want[i]:
            w = pl.PT_BYTES[i]
            assert False, 'section %d: first differing point %d' % (i, next(j for j in range(len(want[i]) // w) if got[i][w * j:w * j + w] != want[i][w * j:w * j + w]))
    assert open(dst, 'rb').read() == host_bytes and h == host_hash
    raw = setup.ptau_contributions(dst)[0]['raw']
    assert raw[pc.OFF_TRANSCRIPT:pc.OFF_TRANSCRIPT + 64] == pc.transcript(9, [], pc.poks_of(raw)) and h == pc.contribution_hash(9, [raw])
    assert pc.five_of(raw) == (want[2][64:128], want[3][128:256], want[4][:64], want[5][:64], want[6])


def test_record_points_from_a_later_chunk(gpu, tmp_path):
    """power 2 in chunks of one point: T_1 and U_1, which the record names, are a chunk of their own that starts at 1; in chunks of two they are a chunk's last lane"""
    from zkcensus_amd import setup
    src = pl.write(str(tmp_path / 's.ptau'), 2, *W0)
    files = {}
    for key, kw in (('host', dict()), ('default', dict(ctx=gpu)), (1, dict(ctx=gpu, chunk_points=1)), (2, dict(ctx=gpu, chunk_points=2)), ('host 1', dict(chunk_points=1))):
        dst = str(tmp_path / 'd.ptau')
        h = setup.debug_contribute_ptau(src, dst, secrets=S2, name='p2', **kw)
        files[key] = (open(dst, 'rb').read(), h)
        secs, _ = read_sections(dst)
        assert pc.five_of(setup.ptau_contributions(dst)[0]['raw']) == (bytes(secs[2][64:128]), bytes(secs[3][128:256]), bytes(secs[4][:64]), bytes(secs[5][:64]), bytes(secs[6])), key
    want = pl.sections(2, *pc.product([W0, S2]))
    for i in range(2, 7):
        assert secs[i] == want[i], i
    assert all(v == files['host'] for v in files.values()), [k for k, v in files.items() if v != files['host']]
    assert files['host'][1] == setup.contribute_ptau(src, str(tmp_path / 'e.ptau'), ctx=gpu, secrets=S2, name='p2')


def test_chain_of_two_at_power_9(gpu, tmp_path):
    from zkcensus_amd import setup
    f = [str(tmp_path / ('f%d.ptau' % i)) for i in range(3)]
    setup.new_ptau(f[0], 9)
    hashes = [setup.contribute_ptau(f[i], f[i + 1], ctx=gpu, secrets=s, name='c%d' % i) for i, s in enumerate((S1, S2))]
    assert setup.verify_ptau_contributions(None, f[2], ctx=gpu, seed=SEED) == (True, 2, '') == setup.verify_ptau_contributions(None, f[2], seed=SEED)
    raws = [r['raw'] for r in setup.ptau_contributions(f[2])]
    assert hashes[1] == pc.contribution_hash(9, raws) and hashes[0] == pc.contribution_hash(9, raws[:1])

    def swap(secs):
        a, b = bytes(secs[2][700 * 64:701 * 64]), bytes(secs[2][701 * 64:702 * 64])
        assert a != b
        secs[2][700 * 64:701 * 64], secs[2][701 * 64:702 * 64] = b, a

    def g2_300(secs):
        secs[3][300 * 128:301 * 128] = pl.g2_mont(7)

    def g1_511(secs):
        assert len(secs[5]) == 512 * 64
        secs[5][511 * 64:] = pl.g1_mont(7)
    for change, text in ((swap, 'section 2 is not the powers of one tau'), (g2_300, 'section 3 is not the powers of one tau'), (g1_511, 'section 5 is not beta times the powers of one tau')):
        secs, order = read_sections(f[2])
        change(secs)
        bad = write_sections(tmp_path / 'bad.ptau', secs, order)
        got = setup.verify_ptau_contributions(None, bad, ctx=gpu, seed=SEED)
        assert got == setup.verify_ptau_contributions(None, bad, seed=SEED) and not got[0] and 'check 5' in got[2] and text in got[2], got
