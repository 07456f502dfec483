"""GPU: the census tree's top levels summed once per subtree and key (ZKC_TOP_FOLD, csrc/zkc_fold.hip: zkc_top_check, top_seed, fold_vmap; csrc/zkc_pass_plan.h: top_fold; csrc/zkc_finalize.hip: fold_const).
The switch is read at key load and every other test keeps its default, so each configuration runs tests/host/top_fold_child.py as a child process: nLevels = 10, the public
prove calls, every proof and public-signal block compared with the CPU oracle's in the child.  Here: that every call was byte-equal, and that the G1 additions the device counted
(zkc_profile_read, category 7) fell by exactly the non-zero window digits of the wires that slots stood for -- which says which proofs folded which tree, and which did not."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
BIG = {'ZKC_TEST_TOP_SLOTS': '4096'}          # a table in which the handful of subtrees of a test census do not share a slot (the default, 8 x 2^K slots, is run by test_two_censuses)


def _child(scenario, cfg):
    env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    env.update(cfg)
    r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'top_fold_child.py'), scenario], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (scenario, cfg, r.returncode, r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out['by'] = {c['name']: c for c in out['calls']}
    assert all(c['equal'] for c in out['calls']), [(c['name'], c['equal']) for c in out['calls']]          # every proof of every call: the oracle's bytes
    return out


@pytest.fixture(scope='module')
def census64():
    return _child('census64', dict(BIG, ZKC_TOP_FOLD='2')), _child('census64', {'ZKC_TOP_FOLD': '0'})


def test_misses_seed_and_hits_fold_exactly_the_slot_wires(census64):
    on, off = census64
    assert on['K'] == 2 and [len(set(s)) for s in on['subtree']] == [4, 4]              # four subtrees per tree
    adds, base = {k: c['adds'] for k, c in on['by'].items()}, {k: c['adds'] for k, c in off['by'].items()}
    assert base['second'] == base['first'] == adds['first']                             # all misses (they seed): proved as without the feature
    saved = sum(a + b for a, b in on['top'][:64])
    assert saved > 0 and adds['second'] == adds['first'] - saved                        # all hits: the slot wires of both trees left every proof's MSMs, and nothing else did


def test_small_and_early_passes_keep_their_lists(census64):
    on, off = census64
    for name in ('one', 'two', 'early'):                                               # a lone proof, a pair, a one-pass call laid out from its inputs: seeded subtrees, nothing folded
        assert on['by'][name]['adds'] == off['by'][name]['adds'] > 0, name


def test_one_changed_word_inside_a_top_group_misses(census64):
    on, _ = census64
    # voters 0 .. 3 with voter 0's witness altered in one word of the census tree's first group: the slot is the same (the index is hashed from other wires), the full
    # comparison says no, and that tree's wires stay in the proof's MSMs -- as the altered witness has them
    assert on['by']['altered']['adds'] == on['by']['unaltered']['adds'] + on['top'][64][0]


def test_passes_that_mix_hits_and_misses():
    out = _child('mixed65', dict(BIG, ZKC_TOP_FOLD='2'))
    adds = {k: c['adds'] for k, c in out['by'].items()}
    top, half = out['top'], set(out['half'])
    total = sum(a + b for a, b in top)
    unfolded = adds['again'] + total                                                   # 'again': 65 hits
    # 'all': 33 + 32 proofs.  The voters of the seeded half hit; the others of pass 0 miss (and seed); the others of pass 1 hit if their check ran after pass 0 was laid out
    upper = unfolded - sum(sum(top[i]) for i in half)
    lower = upper - sum(sum(top[i]) for i in range(33, 65) if i not in half)
    assert lower <= adds['all'] <= upper and adds['again'] < adds['all']
    assert adds['half'] > 0 and out['by']['half']['proofs'] == len(half) and 0 < len(half) < 65


def test_a_voter_at_depth_k_or_less_in_one_tree_folds_the_other():
    out = _child('shallow3', dict(BIG, ZKC_TOP_FOLD='3'))
    assert out['K'] == 3 and [tuple(d) for d in out['depths']] == [(5, 5), (1, 5), (5, 5)]
    adds = {k: c['adds'] for k, c in out['by'].items()}
    saved = sum(out['top'][i][t] for i in range(3) for t in range(2) if out['depths'][i][t] > 3)          # voter 1: the sik tree alone
    assert out['top'][1][0] > 0 and adds['second'] == adds['first'] - saved


def test_two_censuses_alternate_on_one_key():
    out = _child('two_roots', {'ZKC_TOP_FOLD': '2'})                                   # the default table: 8 x 2^K slots per tree, two subtrees may share one
    adds = {k: c['adds'] for k, c in out['by'].items()}
    for c, top in (('a', out['top_a']), ('b', out['top_b'])):
        full = sum(x + y for x, y in top)
        assert adds[c + '0'] - full <= adds[c + '1'] < adds[c + '0']                    # the second round folds, at most every slot wire
        assert adds[c + '2'] == adds[c + '1']                                           # and the other census' calls took nothing away


def test_one_slot_folds_one_subtree():
    out = _child('census64', {'ZKC_TOP_FOLD': '2', 'ZKC_TEST_TOP_SLOTS': '1'})
    adds = {k: c['adds'] for k, c in out['by'].items()}
    # the first miss of the first call fills the one slot of each tree (voter 0's subtrees); every other subtree finds it taken and is never folded
    saved = sum(out['top'][i][t] for t in range(2) for i in range(64) if out['subtree'][t][i] == 0)
    assert 0 < saved < sum(a + b for a, b in out['top'][:64]) and adds['second'] == adds['first'] - saved
