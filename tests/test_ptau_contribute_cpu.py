"""CPU: phase 1 on host threads (ctx = None; include/zkcensus_ptau_contribute.h): powersoftau new, contribute and the chain of contributions checked.  BY VALUE: the
sections 2 .. 6 of a contributed file against tests/ptau_lib.py's independent writer (Python integers and the oracle's scalar multiplications) at the product of the
wastes; then the secrets at their edges, a chain of three and every way it must be rejected, the section-7 parser, the inputs' handling and the way downstream to a key."""
import os, struct, subprocess
import pytest
import oracle_lib as ol
import ptau_lib as pl
import ptau_verify_lib as pv
import ptau_contrib_lib as pc
from ptau_contrib_lib import S1, S2, S3, read_sections, write_sections, records
from zkcensus_amd import _native, setup

ROOT, R = ol.ROOT, ol.R
SEED = bytes(range(11, 43))
NEW_ENTRY_POINTS = sorted(['zkc_g1_scale_each_dev', 'zkc_g2_scale_each_dev', 'zkc_ptau_new', 'zkc_ptau_contribute', 'zkc_ptau_contributions', 'zkc_ptau_verify_contributions',
                           'zkc_ptau_contribute_stats', 'zkc_debug_ptau_contribute', 'zkc_debug_scale_each_dev', 'zkc_debug_scale_each_stats', 'zkc_debug_scale_each_work_bytes',
                           'zkc_debug_tau_scalars_dev'])
BAD_ARG, FORMAT = 4, 5


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_ptau_contribute.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert '#include "zkcensus_ptau_contribute.h"' in open(os.path.join(ROOT, 'include', 'zkcensus.h')).read()


def expect(power, waste):
    return pl.sections(power, *waste)


@pytest.fixture(scope='module')
def chain(tmp_path_factory):
    """new -> S1 -> S2 -> S3 at power 3: the four files and the three hashes"""
    d = tmp_path_factory.mktemp('chain')
    f = [str(d / ('f%d.ptau' % i)) for i in range(4)]
    setup.new_ptau(f[0], 3)
    hashes = [setup.contribute_ptau(f[i], f[i + 1], secrets=s, name='c%d' % i) for i, s in enumerate((S1, S2, S3))]
    return f, hashes


# ---- by value ----
@pytest.mark.parametrize('power', [1, 2, 5])
def test_new_file_is_the_generators(tmp_path, power):
    p = setup.new_ptau(str(tmp_path / 'n.ptau'), power)
    secs, order = read_sections(p)
    want = expect(power, (1, 1, 1))
    assert order == [1, 2, 3, 4, 5, 6, 7]
    for i in range(1, 7):
        assert secs[i] == want[i], i
    assert secs[7] == struct.pack('<I', 0) and setup.ptau_contributions(p) == []
    assert setup.verify_ptau(p, seed=SEED)[0]
    assert setup.verify_ptau_contributions(None, p, seed=SEED) == (True, 0, '')


@pytest.mark.parametrize('power', [1, 2, 5])
def test_contribution_by_value_against_known_waste(tmp_path, power):
    w0 = (pv.TAU, pv.ALPHA, pv.BETA)
    src = pl.write(str(tmp_path / 's.ptau'), power, *w0)                      # a prepared file: 12 .. 15 are there
    dst = str(tmp_path / 'd.ptau')
    h = setup.contribute_ptau(src, dst, secrets=S1, name='by value')
    secs, order = read_sections(dst)
    want = expect(power, pc.product([w0, S1]))
    assert order == [1, 2, 3, 4, 5, 6, 7]                                     # the Lagrange sections are dropped
    for i in range(1, 7):
        assert secs[i] == want[i], i
    recs = setup.ptau_contributions(dst)
    assert len(recs) == 1 and recs[0]['name'] == 'by value' and recs[0]['type'] == 0 and len(h) == 64
    assert recs[0]['tauG1'] == want[2][64:128] and recs[0]['tauG2'] == want[3][128:256] and recs[0]['alphaG1'] == want[4][:64] and recs[0]['betaG1'] == want[5][:64]
    assert recs[0]['betaG2'] == want[6]
    assert setup.verify_ptau_contributions(src, dst, seed=SEED) == (True, 1, '')


ROOT4 = pl.root_of_unity(2)
EDGES = {'tau_one': (1, 5, 7), 'tau_minus_one': (R - 1, 5, 7), 'tau_on_domain': (ROOT4, 5, 7), 'alpha_is_beta': (S2[0], 99, 99), 'all_minus_one': (R - 1, R - 1, R - 1)}


@pytest.mark.parametrize('edge', sorted(EDGES))
def test_accepted_edge_secrets(tmp_path, edge):
    power, w0, s = 2, (pv.TAU, pv.ALPHA, pv.BETA), EDGES[edge]
    src = pl.write(str(tmp_path / 's.ptau'), power, *w0); dst = str(tmp_path / 'd.ptau')
    setup.contribute_ptau(src, dst, secrets=s)
    secs, _ = read_sections(dst)
    want = expect(power, pc.product([w0, s]))
    for i in range(2, 7):
        assert secs[i] == want[i], i
    assert setup.verify_ptau_contributions(src, dst, seed=SEED) == (True, 1, '')


@pytest.mark.parametrize('which', [0, 1, 2])
@pytest.mark.parametrize('value', [0, R])
def test_refused_secrets(tmp_path, which, value):
    src = setup.new_ptau(str(tmp_path / 'n.ptau'), 1); dst = tmp_path / 'd.ptau'
    s = [3, 5, 7]; s[which] = value
    with pytest.raises(_native.ZkcError) as ei:
        setup.contribute_ptau(src, str(dst), secrets=[x.to_bytes(32, 'little') for x in s])
    assert ei.value.code == BAD_ARG and 'must be in [1, r)' in str(ei.value) and not dst.exists()
    assert os.listdir(tmp_path) == ['n.ptau']                                # no temporary file either


def test_random_secrets_and_verify_flag(tmp_path):
    src = setup.new_ptau(str(tmp_path / 'n.ptau'), 2)
    a, b = str(tmp_path / 'a.ptau'), str(tmp_path / 'b.ptau')
    ha = setup.contribute_ptau(src, a, verify=True); hb = setup.contribute_ptau(src, b)
    assert ha != hb and read_sections(a)[0][2] != read_sections(b)[0][2]
    assert setup.verify_ptau_contributions(src, a, seed=SEED) == (True, 1, '')
    # verify=True refuses a source that is not the powers of one tau, with verify_ptau's reason
    secs, order = read_sections(a)
    secs[2][2 * 64:3 * 64], secs[2][3 * 64:4 * 64] = bytes(secs[2][3 * 64:4 * 64]), bytes(secs[2][2 * 64:3 * 64])
    bad = write_sections(tmp_path / 'bad.ptau', secs, order)
    with pytest.raises(_native.ZkcError) as ei:
        setup.contribute_ptau(bad, str(tmp_path / 'never.ptau'), verify=True)
    assert ei.value.code == FORMAT and 'section 2 is not the powers of one tau' in str(ei.value) and not (tmp_path / 'never.ptau').exists()


# ---- a chain of three ----
def test_chain_of_three(chain, tmp_path):
    f, hashes = chain
    assert setup.verify_ptau_contributions(None, f[3], seed=SEED) == (True, 3, '')
    assert setup.verify_ptau_contributions(f[0], f[3], seed=SEED) == (True, 3, '')
    assert setup.verify_ptau_contributions(f[1], f[3], seed=SEED) == (True, 2, '')
    assert setup.verify_ptau_contributions(f[3], f[3], seed=SEED) == (True, 0, '')
    want = expect(3, pc.product([S1, S2, S3]))
    secs, _ = read_sections(f[3])
    for i in range(2, 7):
        assert secs[i] == want[i], i
    raws = [[r['raw'] for r in setup.ptau_contributions(p)] for p in f]
    assert [len(x) for x in raws] == [0, 1, 2, 3]
    for i in range(3):
        assert raws[i + 1][:i + 1] == raws[i] + [raws[i + 1][i]] and raws[3][:i] == raws[i]       # earlier records are byte-equal prefixes
    assert [r['name'] for r in setup.ptau_contributions(f[3])] == ['c0', 'c1', 'c2']
    # the hash is a function of the file and the secrets
    again = str(tmp_path / 'again.ptau')
    assert setup.contribute_ptau(f[0], again, secrets=S1, name='c0') == hashes[0] and open(again, 'rb').read() == open(f[1], 'rb').read()
    assert len(set(hashes)) == 3
    assert setup.contribute_ptau(f[0], again, secrets=S2, name='c0') != hashes[0]


@pytest.mark.parametrize('case', sorted(pc.rejects()))
def test_changed_chain_is_rejected_with_its_reason(chain, tmp_path, case):
    f, _ = chain
    change, words = pc.rejects()[case]
    secs, order = read_sections(f[3])
    change(secs)
    bad = write_sections(tmp_path / 'bad.ptau', secs, order)
    ok, _, why = setup.verify_ptau_contributions(None, bad, seed=SEED)
    assert not ok and all(w in why for w in words), why


# ---- the record against its restatement in Python (tests/ptau_contrib_lib.py: hashlib, tests/g2_challenge.py, the oracle's products), in both directions ----
def test_library_records_against_the_restatement(chain):
    """what the library wrote, recomputed from the header's description alone: every stored transcript, every returned hash, g2_spx = x g2_sp with g2_sp hashed from
    the transcript, g1_sx = x g1_s"""
    f, hashes = chain
    raws = [r['raw'] for r in setup.ptau_contributions(f[3])]
    assert len(raws) == 3
    for k, (raw, s) in enumerate(zip(raws, (S1, S2, S3))):
        poks = pc.poks_of(raw)
        tr = pc.transcript(3, raws[:k], poks)
        assert raw[pc.OFF_TRANSCRIPT:pc.OFF_TRANSCRIPT + 64] == tr, k
        assert hashes[k] == pc.contribution_hash(3, raws[:k + 1]), k
        for i in range(3):
            g1_s, g1_sx, g2_spx = (pc.from_mont(p) for p in poks[i])
            assert g2_spx == ol.msm_g2(pc.challenge(tr, i), ol.le32(s[i])), (k, i)
            assert g1_sx == ol.g1_mul(g1_s, s[i]), (k, i)
        # the five points are the file's after that contribution
        secs, _ = read_sections(f[k + 1])
        assert pc.five_of(raw) == (bytes(secs[2][64:128]), bytes(secs[3][128:256]), bytes(secs[4][:64]), bytes(secs[5][:64]), bytes(secs[6]))


@pytest.fixture(scope='module')
def py_chain(tmp_path_factory):
    """a chain of three written by tests/ptau_contrib_lib.py alone: the sections of its last file, the file, and the file after the first contribution"""
    d = tmp_path_factory.mktemp('py_chain')
    secs, recs = pc.make_chain(3, [S1, S2, S3])
    first, recs1 = pc.make_chain(3, [S1])
    assert recs1 == recs[:1]
    return secs, recs, write_sections(d / 'py3.ptau', secs), write_sections(d / 'py1.ptau', first), first


def test_restatement_records_against_the_library(py_chain, tmp_path):
    secs, recs, last, first, _ = py_chain
    assert setup.verify_ptau_contributions(None, last, seed=SEED) == (True, 3, '')
    assert setup.verify_ptau_contributions(first, last, seed=SEED) == (True, 2, '')
    got = setup.ptau_contributions(last)
    assert [r['raw'] for r in got] == recs and [r['name'] for r in got] == ['py0', 'py1', 'py2']
    # the library goes on from a file it did not write, and hashes the Python-made records as the restatement does
    more = str(tmp_path / 'more.ptau')
    h = setup.contribute_ptau(last, more, secrets=pc.S4, name='c3')
    assert setup.verify_ptau_contributions(None, more, seed=SEED) == (True, 4, '')
    assert setup.verify_ptau_contributions(last, more, seed=SEED) == (True, 1, '')
    raws = [r['raw'] for r in setup.ptau_contributions(more)]
    assert raws[:3] == recs and h == pc.contribution_hash(3, raws)


# ---- one forgery per check ----
FORGERIES = pc.forgeries(3, [S1, S2, S3])


def test_forgery_table_names_every_check():
    assert sorted(n.split()[0] for n in FORGERIES) == sorted(['3.1'] * 3 + ['3.3'] * 4 + ['3.4'] * 2 + ['3.5'] * 2 + ['4'] * 5 + ['3.2', '3'])


@pytest.mark.parametrize('case', sorted(FORGERIES))
def test_forged_chain_is_refused_by_its_own_check(py_chain, tmp_path, case):
    """each forgery is applied to a chain that is accepted first, and the reason must be that of the check the forgery is for (its number is the case's first word),
    which shows the forgery valid under the checks before it"""
    secs, _, last, first, first_secs = py_chain
    change_next, change_prev, words = FORGERIES[case]
    prev = None
    if change_prev:
        assert setup.verify_ptau_contributions(first, last, seed=SEED) == (True, 2, '')
        psecs = {i: bytearray(b) for i, b in first_secs.items()}
        change_prev(psecs)
        assert psecs != first_secs
        prev = write_sections(tmp_path / 'prev.ptau', psecs)
    else:
        assert setup.verify_ptau_contributions(None, last, seed=SEED) == (True, 3, '')
    nsecs = {i: bytearray(b) for i, b in secs.items()}
    change_next(nsecs)
    assert change_prev or nsecs != secs
    bad = write_sections(tmp_path / 'bad.ptau', nsecs)
    ok, _, why = setup.verify_ptau_contributions(prev, bad, seed=SEED)
    assert not ok and all(w in why for w in words), (case, why)


def test_prev_must_be_a_prefix_and_of_the_same_power(chain, tmp_path):
    f, _ = chain
    other = str(tmp_path / 'other.ptau')
    setup.contribute_ptau(f[0], other, secrets=S2)
    ok, _, why = setup.verify_ptau_contributions(other, f[3], seed=SEED)
    assert not ok and "check 2: the previous file's contributions are not a prefix of the next file's" in why
    ok, _, why = setup.verify_ptau_contributions(f[3], f[1], seed=SEED)
    assert not ok and 'check 2: the next file has fewer contributions' in why
    p4 = setup.new_ptau(str(tmp_path / 'p4.ptau'), 4)
    ok, _, why = setup.verify_ptau_contributions(p4, f[3], seed=SEED)
    assert not ok and 'check 1: the files have different powers (4 and 3)' in why
    # the records of f[1] under the points of f[0]: nothing new, but the sections differ from the chain's start
    ok, _, why = setup.verify_ptau_contributions(f[1], f[2], seed=SEED)
    assert ok
    secs, order = read_sections(f[2]); secs[7] = read_sections(f[1])[0][7]
    stale = write_sections(tmp_path / 'stale.ptau', secs, order)
    ok, n_new, why = setup.verify_ptau_contributions(f[1], stale, seed=SEED)
    assert not ok and n_new == 0 and 'check 4: no new contribution' in why


# ---- the parser ----
def test_section_7_format_errors(chain, tmp_path):
    f, _ = chain
    secs, order = read_sections(f[3])
    good = bytes(secs[7])
    cases = {'truncated': (good[:-3], 'truncated contribution record'), 'count': (struct.pack('<I', 4) + good[4:], 'the contribution count does not fit section 7'),
             'huge_count': (struct.pack('<I', 0xffffffff) + good[4:], 'the contribution count does not fit section 7'), 'trailing': (good + b'\0', 'bytes after the last contribution record'),
             'short': (b'\x01\0', 'section 7 is shorter than its count')}
    at, ln = records(good)[1]
    t = bytearray(good); t[at + pc.REC - 8] = 1; cases['type'] = (bytes(t), 'unknown contribution type 1 (record 1)')
    t = bytearray(good); t[at + pc.REC] = 2; cases['tag'] = (bytes(t), 'unknown parameter tag 2 (record 1)')
    t = bytearray(good); t[at + pc.REC + 1] = 200; cases['param'] = (bytes(t), 'truncated parameter (record 1)')
    for name, (body, text) in cases.items():
        secs[7] = bytearray(body)
        bad = write_sections(tmp_path / (name + '.ptau'), secs, order)
        with pytest.raises(_native.ZkcError) as ei:
            setup.ptau_contributions(bad)
        assert ei.value.code == FORMAT and text in str(ei.value), name
        ok, _, why = setup.verify_ptau_contributions(None, bad, seed=SEED)
        assert not ok and 'check 1: the next file does not parse' in why and text in why
        with pytest.raises(_native.ZkcError) as ei:
            setup.contribute_ptau(bad, str(tmp_path / 'never.ptau'), secrets=S1)
        assert ei.value.code == FORMAT and not (tmp_path / 'never.ptau').exists()


def test_section_7_parser_under_asan_ubsan(tmp_path):
    """tests/host/ptau_contrib_parse_asan.cc: the parser alone, as a program of its own, over truncations and mutations of records it builds"""
    exe = str(tmp_path / 'ptau_contrib_parse_asan')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'ptau_contrib_parse_asan.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'ptau contribution parser: ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- input handling ----
def test_sections_in_another_order_and_no_section_7(tmp_path):
    power, w0 = 2, (pv.TAU, pv.ALPHA, pv.BETA)
    secs = pl.sections(power, *w0)
    shuffled = write_sections(tmp_path / 'sh.ptau', secs, [6, 13, 5, 7, 4, 1, 3, 12, 2, 15, 14])
    del secs[7]
    bare = write_sections(tmp_path / 'bare.ptau', secs)
    want = expect(power, pc.product([w0, S3]))
    for src in (shuffled, bare):
        dst = str(tmp_path / 'd.ptau')
        setup.contribute_ptau(src, dst, secrets=S3)
        got, order = read_sections(dst)
        assert order == [1, 2, 3, 4, 5, 6, 7]
        for i in range(1, 7):
            assert got[i] == want[i], i
        assert len(setup.ptau_contributions(dst)) == 1


@pytest.mark.parametrize('kind', ['off_curve', 'coordinate', 'infinity'])
def test_bad_point_is_refused_with_section_and_index(tmp_path, kind):
    power = 3
    secs = pl.sections(power, pv.TAU, pv.ALPHA, pv.BETA)
    at = 5 * 64
    if kind == 'off_curve':
        secs[4][at + 32] ^= 1
    elif kind == 'coordinate':
        secs[4][at:at + 32] = ol.Q.to_bytes(32, 'little')
    else:
        secs[4][at:at + 64] = bytes(64)
    secs[4][7 * 64 + 32] ^= 1                                                  # a later one as well: the smallest index is named
    src = write_sections(tmp_path / 's.ptau', secs); dst = tmp_path / 'd.ptau'
    with pytest.raises(_native.ZkcError) as ei:
        setup.contribute_ptau(src, str(dst), secrets=S1)
    assert ei.value.code == FORMAT and 'section 4 point 5 has a coordinate >= q, is not on the curve or is at infinity' in str(ei.value)
    assert sorted(os.listdir(tmp_path)) == ['s.ptau']


# ---- downstream ----
def test_contributed_file_prepares_and_gives_a_key(chain, tmp_path):
    f, _ = chain
    prepared = setup.prepare_ptau(f[3], str(tmp_path / 'p.ptau'))
    assert read_sections(prepared)[0][7] == read_sections(f[3])[0][7]        # section 7 survives prepare byte for byte
    assert setup.verify_ptau_contributions(f[2], prepared, seed=SEED) == (True, 1, '')
    r = pl.write_r1cs(tmp_path / 'tiny.r1cs', *pv.TINY_CIRCUIT)
    setup.from_ptau(r, prepared, tmp_path / 'k.zkey', tmp_path / 'k.json', verify=True)
    assert os.path.getsize(tmp_path / 'k.zkey') > 0 and os.path.getsize(tmp_path / 'k.json') > 0
    # a contribution to the prepared file drops the stale Lagrange sections
    again = str(tmp_path / 'again.ptau')
    setup.contribute_ptau(prepared, again, secrets=S1)
    assert read_sections(again)[1] == [1, 2, 3, 4, 5, 6, 7] and len(setup.ptau_contributions(again)) == 4
