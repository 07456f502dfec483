"""GPU: a folded pass without the transform pair of C (ZKC_C_ROWS; csrc/zkc_pass_plan.h: c_rows, h_vmap; csrc/zkc_fold.hip: c_rows_prepare; csrc/zkc_ntt.hip:
zkc_c_rows_delta, zkc_join_abc_ct).  The switch is read at key load and the rule keeps the nLevels-10 test key on the old path, so every configuration runs
tests/host/c_rows_child.py as a child process with the path forced (ZKC_C_ROWS=2) or off (=0): the public prove calls, every proof and public-signal block compared with
the CPU oracle's in the child.  Here: that the calls were byte-equal on both paths, that the forced calls really left C's pair out (two vectors per proof through the
transform kernels instead of three), that the G1 additions the device counted rose by exactly the non-zero window digits of C_dom - C_T (and the few digits by which the evaluations themselves change), that two calls in flight on the
two call slots give the bytes they give alone, and that the second half of the H table holds -H' by value."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
FORCED, OFF = {'ZKC_C_ROWS': '2'}, {'ZKC_C_ROWS': '0'}


@pytest.fixture(scope='module')
def child(tmp_path_factory):
    cache = str(tmp_path_factory.mktemp('c_rows') / 'oracle.pickle')

    def go(scenario, cfg, *more):
        env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
        env.update(cfg)
        r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'c_rows_child.py'), scenario, cache, *more], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (scenario, cfg, r.returncode, r.stderr[-2000:])
        out = json.loads(r.stdout.strip().splitlines()[-1])
        if 'calls' in out:
            out['by'] = {c['name']: c for c in out['calls']}
        return out
    return go


@pytest.fixture(scope='module')
def calls(child):
    """the same calls on fresh keys: path forced, path off, both without the top-of-tree table (whose hits in a two-pass call depend on timing), and forced with it"""
    nt = {'ZKC_TOP_FOLD': '0'}
    return child('calls', dict(FORCED, **nt), 'digits'), child('calls', dict(OFF, **nt)), child('calls', FORCED)


PROOFS = {'three': 3, 'thirtythree': 33, 'sixtyfive': 65, 'uneven': 5, 'foreign': 4}
PASSES = {'three': 1, 'thirtythree': 1, 'sixtyfive': 2, 'uneven': 1}


def test_every_proof_is_the_oracles_on_both_paths(calls):
    for run in calls:
        assert {k: c['proofs'] for k, c in run['by'].items()} == PROOFS
        assert all(c['equal'] for c in run['calls']), [(c['name'], c['equal']) for c in run['calls']]
    on, off, on_top = calls
    for name in PROOFS:
        assert on['by'][name]['sha'] == off['by'][name]['sha'] == on_top['by'][name]['sha'], name          # ZKC_C_ROWS=0 gives the same bytes


def test_forced_calls_leave_out_the_pair_of_c_and_others_keep_it(calls):
    on, off, on_top = calls
    for run in (on, on_top):
        for name, passes in PASSES.items():
            c = run['by'][name]
            assert (c['new'], c['old'], c['vectors']) == (passes, 0, 2 * PROOFS[name]), (name, c)
        f = run['by']['foreign']                                                       # one foreign witness unfolds its pass: three vectors per proof
        assert (f['new'], f['vectors']) == (0, 3 * PROOFS['foreign'])
    for name in PROOFS:
        c = off['by'][name]
        assert (c['new'], c['vectors']) == (0, 3 * PROOFS[name]), (name, c)
    assert on['depths5'] == [[5, 5], [2, 2], [5, 5], [2, 2], [2, 2]]                       # the uneven call: rows listed for the pass' depths hold the template's C for the shallow voters


def test_additions_rise_by_the_digits_of_the_c_differences(calls):
    """Category 7 counts every non-zero digit of every job.  The path adds the digits of the listed differences C_dom - C_T, and it replaces each proof's n evaluations
    h = A'B' - pair(C_dom) by h' = A'B' - pair(C_T): both are n full-width scalars whose 15 n digits are zero with probability 2^-17 each, a handful per proof and not the
    same handful (measured: 3 more non-zero digits over the 33-voter call).  The child counts both from the domain vectors, so the balance is exact."""
    on, off, _ = calls
    for name in PASSES:
        a, b = on['by'][name], off['by'][name]
        assert a['rows'] > 0 and a['digits'] > 0, (name, a)
        print(name, 'additions', a['adds'], b['adds'], 'rows', a['rows'], 'digits of the differences', a['digits'], 'change in the digits of the evaluations', a['h_digits'])
        assert a['adds'] - b['adds'] == a['digits'] + a['h_digits'], (name, a['adds'], b['adds'], a['digits'], a['h_digits'], a['rows'])
    assert on['by']['foreign']['adds'] == off['by']['foreign']['adds'] > 0


def test_two_call_slots_in_flight(child):
    out = child('slots', FORCED)
    assert out['equal'] and out['same'] == [True, True, True]
    assert out['new_alone'] == 1 and out['new_together'] == 3                           # the 33-voter call takes the new path every time, the pair of voters (a tree-shaped pass) never


def test_second_half_of_the_h_table_by_value(child):
    out = child('bases', FORCED)
    assert out['rows'] == [0, 1, out['last_row'], out['n'] - 1] and 1 < out['last_row'] < out['n'] - 1
    assert out['same'] == [True] * 4 and out['ready'] == 1
