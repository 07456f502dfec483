"""GPU: every scheduling / kernel-form switch of the library gives the SAME proof bytes as the default configuration.  Most of them are read once per process
(`static const ... = getenv(...)`), so each configuration runs tests/host/prove_digest.py as a child process (started before this process needs the GPU for anything else) and the
digests are compared.  What is covered: the two LDS-DMA forms of the G2 accumulation, the G2 accumulation held behind the transforms (round 2-3's order), the bucket reduction
on its own stream, two pipeline lanes, round 1's reduction windows and odd ones, buildABC with products for the unit coefficients, unfolded passes with their infinity bases left
in, the buildABC prefetch placements, the two-transform NTT, the one-stage head kernel, the second section tables of a deep pass, folding off.  This file sorts first on purpose (like the Node test): the children are started BEFORE this pytest
process has initialised the GPU -- the GPU boxes refuse to start a program from a process that has."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CONFIGS = [
    {}, {'ZKC_G2_ACC': '1', 'ZKC_C_SECTIONS': '13'}, {'ZKC_G2_ACC': '2'}, {'ZKC_G2_ACC_HOLD': '1'}, {'ZKC_REDUCE_STREAM': '1', 'ZKC_INFLIGHT': '40'}, {'ZKC_LANES': '2', 'ZKC_INFLIGHT': '40'},
    {'ZKC_VW_BIG': '1024', 'ZKC_VW_SMALL': '256', 'ZKC_INFLIGHT': '40'}, {'ZKC_VW_BIG': '8192', 'ZKC_VW_SMALL': '512', 'ZKC_VW_G2': '256', 'ZKC_INFLIGHT': '40'},
    {'ZKC_MATVEC_UNITS': '0', 'ZKC_NTT_RADIX': '1'}, {'ZKC_NOFOLD_LISTS': '0', 'ZKC_NO_FOLD': '1'}, {'ZKC_NO_FOLD': '1'}, {'ZKC_MV_PREFETCH_AT_NTT': '1', 'ZKC_INFLIGHT': '8'}, {'ZKC_MATVEC_INLINE': '1', 'ZKC_INFLIGHT': '8'},
    {'ZKC_NTT_SEPARATE': '1'}, {'ZKC_INFLIGHT': '40'}, {'ZKC_DEEP_TABLES': '2', 'ZKC_DEEP_WIRES': '1', 'ZKC_INFLIGHT': '40'},
]


_failed = []                                             # the configuration of a child that failed or ran out of time (a fault, a hang): no test of this file starts a further child


def _child(script, cfg):
    """one configuration in a child process: its own time limit, and its exit status looked at before anything it printed"""
    if _failed:
        pytest.fail('no child started: an earlier one failed under %r' % (_failed[0],))
    env = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    env.update(cfg)
    try:                                                 # (a box that refuses to start a child program from this process raises OSError: a failure, not a skip)
        r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', script)], env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(cfg)
        raise
    if r.returncode != 0:
        _failed.append(cfg)
    assert r.returncode == 0, (cfg, r.returncode, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_switches_do_not_change_a_byte():
    digests = [_child('prove_digest.py', cfg)['sha256'] for cfg in CONFIGS]
    assert len(set(digests)) == 1, [(c, d[:12]) for c, d in zip(CONFIGS, digests)]


# Switches that no configuration above runs: the one-wave-per-task blinding for every pass, the lane-per-segment G2 accumulation of small passes, a key without the
# lone-proof G2 table, the G2 MSM behind the G1 sort, the G2 accumulation never held, unchained G1 accumulations over two lanes, fold flags awaited instead of the early
# layout, other window bits for the H section and for the second section tables (taken by every pass: ZKC_DEEP_WIRES=1), every stage on one stream.
UNVISITED = [
    {'ZKC_FINALIZE_WAVES': '1'}, {'ZKC_G2_BUCKET_WAVE': '0'}, {'ZKC_G2_LONE_TABLE': '0'}, {'ZKC_G2_LATE': '1'}, {'ZKC_G2_ACC_EARLY': '1'},
    {'ZKC_ACC_CHAIN': '0', 'ZKC_LANES': '2', 'ZKC_INFLIGHT': '40'}, {'ZKC_EARLY_LAYOUT': '0'}, {'ZKC_C_H': '13'},
    {'ZKC_C_DEEP': '13', 'ZKC_DEEP_TABLES': '2', 'ZKC_DEEP_WIRES': '1', 'ZKC_INFLIGHT': '40'}, {'ZKC_SERIAL_STREAMS': '1'},
]


@pytest.fixture(scope='module')
def default_digest():
    return _child('prove_digest.py', {})['sha256']


@pytest.mark.parametrize('cfg', UNVISITED, ids=lambda c: ','.join('%s=%s' % kv for kv in c.items()))
def test_unvisited_switches_do_not_change_a_byte(default_digest, cfg):
    assert _child('prove_digest.py', cfg)['sha256'] == default_digest, cfg          # (a digest that differs is a finding, not a reason to stop: the child ended well)


def test_blinding_forms_agree_at_scalar_edges():
    """Passes of 5 and of 65 proofs (one pass each: ZKC_INFLIGHT=128 in tests/host/blind_digest.py) with the edge (r, s) pairs of tests/blinding_cases.py, each unfolded
    (with the foreign witness) and folded (voters only), through the lane-per-product kernels (default) and through zkc_finalize (ZKC_FINALIZE_WAVES, 65 workgroups):
    the same bytes, and the CPU oracle's, computed here in the parent."""
    import blinding_cases as bc
    from zkcensus_amd import setup
    outs = [_child('blind_digest.py', cfg) for cfg in ({}, {'ZKC_FINALIZE_WAVES': '1'})]
    zk = open(setup.artifact_paths(bc.NL)[1], 'rb').read()                # the children made sure of the key; this process reads the file and never loads the library
    want, cache = {}, {}
    for n, foreign in ((5, True), (65, True), (5, False), (65, False)):
        jobs = list(zip(*bc.batch(n, with_foreign=foreign)[:2]))
        todo = [j for j in dict.fromkeys(jobs) if j not in cache]
        for j, (rc, proof, _) in zip(todo, ol.pmap(lambda j: ol.prove(zk, j[0], *j[1]), todo)):
            assert rc == 0
            cache[j] = proof
        want[str(n) + ('' if foreign else 'f')] = b''.join(cache[j] for j in jobs).hex()
    assert all(set(o) == set(want) for o in outs)
    for n in want:
        bad = [[q for q in range(len(want[n]) // 512) if o[n][512 * q:512 * q + 512] != want[n][512 * q:512 * q + 512]] for o in outs]
        assert bad == [[], []], (n, 'proofs that differ from the oracle (lane per product, wave per task)', bad)
    assert outs[0] == outs[1]
