"""GPU: the stream plan of a batch call (csrc/zkc_pass_plan.h: plan::lane_roles; csrc/zkc_prove.hip: prove_batch_begin).  A census key's call of several passes rotates them
over the key's lanes and runs every stage of a pass on the lane's one stream; ZKC_LANE_STREAMS=2 / 3 give the G2 side, and the blinding too, streams of their own again.
Whatever the plan, the proofs are the same bytes: the plans differ only in which events order the same kernels.  The switches are read at key load, so each leg is one fresh
child process (tests/host/lane_streams_child.py, nLevels = 10) with its own time limit; this process never loads the library.

The plan a call took is read back as the number of distinct streams its witness chunks and passes were enqueued on (zkc_zkey_call_streams): the context's stream for the
witness chunks plus, per lane the call used, one, two or three of the lane's streams -- 1 + 4 x {1, 2, 3} = 5 / 9 / 13 for a call that uses all four lanes, 1 + 3 for a call
that stays on one lane without the caller naming it, 1 for a key loaded with ZKC_SERIAL_STREAMS."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu

_failed = []                                             # a child that failed or ran out of time (a fault, a hang): no test of this file starts a further one


def _child(scenario, cfg, oracle=False):
    if _failed:
        pytest.fail('no child started: an earlier one failed under %r' % (_failed[0],))
    env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    env.update(cfg)
    cmd = [sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'lane_streams_child.py'), scenario] + (['oracle'] if oracle else [])
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append((scenario, cfg))
        raise
    if r.returncode != 0:
        _failed.append((scenario, cfg))
    assert r.returncode == 0, (scenario, cfg, r.returncode, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


SERIAL = {'ZKC_LANES': '1', 'ZKC_SERIAL_STREAMS': '1'}


@pytest.fixture(scope='module')
def plan_default():
    """the default plan's leg: computed once, with the oracle's verdict on its sample, and shared"""
    return _child('plan', {'ZKC_INFLIGHT': '32'}, oracle=True)


def test_default_plan_is_one_stream_per_lane_and_the_oracles_bytes(plan_default):
    d = plan_default
    assert (d['pass_size'], d['lanes'], d['per']) == (32, 4, 28)             # 163 voters: six passes of 28, 28, 28, 28, 28, 23 -- the rotation wraps past lane 3
    assert d['sample'] == [0, 27, 28, 55, 56, 83, 84, 111, 112, 139, 140, 162]      # first, last, both sides of every pass boundary
    assert d['oracle_equal'] == [True] * len(d['sample'])
    assert d['streams'] == [5]                                             # four lanes' st + the context's stream (witness chunks, fold check)


@pytest.mark.parametrize('cfg, streams', [({'ZKC_LANE_STREAMS': '1'}, 5), ({'ZKC_LANE_STREAMS': '2'}, 9), ({'ZKC_LANE_STREAMS': '3'}, 13), (SERIAL, 1)],
                         ids=['streams=1', 'streams=2', 'streams=3', 'one lane, serial'])
def test_every_plan_gives_the_same_bytes(plan_default, cfg, streams):
    d = _child('plan', dict(cfg, ZKC_INFLIGHT='32'))
    assert d['streams'] == [streams]
    assert d['calls'] == plan_default['calls'], 'proofs or public signals differ from the default plan under %r' % (cfg,)


def test_pipelined_steps_repeat_their_bytes():
    """begin(0), begin(1), finish(0), finish(1), eight times over: the second call's passes land on lanes whose result slots the first call's blindings still read"""
    d = _child('pipelined', {'ZKC_INFLIGHT': '64'}, oracle=True)
    assert (d['pass_size'], d['lanes']) == (64, 4) and len(d['calls']) == 16
    assert d['streams'] == [3] * 8                                         # 65 voters: two passes on lanes 0 and 1 + the context's stream
    assert all(d['calls'][2 * r] == d['calls'][0] and d['calls'][2 * r + 1] == d['calls'][1] for r in range(8)) and d['calls'][0] != d['calls'][1]
    assert d['oracle_equal'] == [True] * 8


def test_small_calls_between_rotating_calls():
    """a lone proof and a pair (the tree shape of a pass, on lane 0 with the plan of a one-lane call) between calls of three passes over three lanes"""
    d = _child('tree', {'ZKC_INFLIGHT': '32'}, oracle=True)
    ref = _child('tree', dict(SERIAL, ZKC_INFLIGHT='32'))
    assert d['streams'] == [4, 3, 4, 3, 4] and ref['streams'] == [1] * 5     # rotating: 3 lanes + 1; a small one-pass call: st, st2 (blinding on st) + 1
    assert d['calls'] == ref['calls']
    assert d['calls'][0] == d['calls'][2] == d['calls'][4] and d['oracle_equal'] == [True] * 3


def test_a_one_pass_call_beside_a_rotating_call_on_one_lane(plan_default):
    """The two halves of a batch call on both call slots of one key, the plans differing: a rotating call runs its G2 MSM on the lane's st, a call of one pass on st2, and
    lane 0 has one G2 work space for both (zkc_lane::g2_on / g2_done order them).  begin(0), begin(1), finish(0), finish(1) with (rotating, one pass) and (one pass,
    rotating), the one-pass call of 20 voters and of 2 (the tree shape), three times each: every call repeats the bytes of its synchronous call, which are the default
    plan's of test_every_plan_gives_the_same_bytes for the 163 voters (the same voters and scalars)."""
    d = _child('mixed', {'ZKC_INFLIGHT': '32'})
    sync = dict(zip((163, 20, 2), d['calls']))
    assert d['streams'][0] == 5 and len(d['pipelined']) == 12 and sync[163] == plan_default['calls'][0]
    assert sorted({tuple(p['sizes']) for p in d['pipelined']}) == [(2, 163), (20, 163), (163, 2), (163, 20)]
    for p in d['pipelined']:
        assert p['calls'] == [sync[b] for b in p['sizes']], ('pipelined calls differ from their synchronous bytes', p['sizes'])
        assert [s for b, s in zip(p['sizes'], p['streams']) if b == 163] == [5]          # the rotating call keeps one stream per lane beside the other call


def test_tree_shaped_passes_inside_a_rotating_call(plan_default):
    """plan::call_split cuts a call into equal passes (163 voters at 32 per pass: 28, 28, 28, 28, 28, 23 -- not five of 32 and a stub of three), so only a tiny pass size puts a
    one- or two-proof pass into a call that rotates: three voters at ZKC_INFLIGHT=2 are a pass of two on lane 0 and a tree-shaped pass of one on lane 1, each on its lane's st."""
    assert plan_default['per'] == 28
    d = _child('tiny', {'ZKC_INFLIGHT': '2'})
    assert (d['pass_size'], d['lanes']) == (2, 4) and d['streams'] == [3, 3]
    assert d['calls'][0] == d['calls'][1] and d['oracle_equal'] == [True] * 3
