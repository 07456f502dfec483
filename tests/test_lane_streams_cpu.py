"""CPU: which of a lane's roles share a stream in a pass (csrc/zkc_pass_plan.h: plan::lane_roles) through a stand-alone host program (tests/host/lane_streams_host.cc) under
AddressSanitizer + UBSan.  A call that stays on one lane keeps the plan of plan::stream_order field for field, whatever ZKC_LANE_STREAMS says; a call whose passes rotate over
several lanes runs every role on the lane's st by default, the G2 side on st2 with ZKC_LANE_STREAMS=2, and the old three streams with 3.  The expected values are a model
written here from those rules, and literals; prove_batch_begin (csrc/zkc_prove.hip) keeps no copy of the logic."""
import itertools
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, ST2, FIN, RED = 0, 1, 2, 3


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('lane_streams') / 'lane_streams_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'lane_streams_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the program's answers are still checked
    assert b.returncode == 0, b.stderr[-3000:]

    def go(cases):
        text = ''.join('roles ' + ' '.join(str(int(x)) for x in c) + '\n' for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
        assert r.returncode == 0 and 'lane streams: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-2] == 'lane streams: %d cases' % len(cases)
        return [[int(x) for x in ln.split()] for ln in lines[:len(cases)]]
    return go


def call(key_lanes, lane0, npasses):
    """(one_lane, lanes) as prove_batch_begin derives them: the caller named the lane or the key has one; else the call rotates over as many lanes as it has passes"""
    return int(lane0 >= 0 or key_lanes == 1), 1 if lane0 >= 0 else min(key_lanes, npasses)


def grid():
    for nb, key_lanes, lane0, npasses, sw, tree, red, serial in itertools.product((1, 2, 4, 31, 32, 64), (1, 2, 4), (-1, 0, 3), (1, 2, 5), (0, 1, 2, 3), (0, 1), (0, 1), (0, 1)):
        one_lane, lanes = call(key_lanes, lane0, npasses)
        for pas in sorted({0, npasses - 1}):
            yield (nb, one_lane, pas, npasses, lane0, tree, lanes, sw, red, serial)


def today(nb, npasses, lane0, tree, red, serial):
    """the plan of rounds 2-5, as plan::stream_order's comments state it: G2 on st2; blinding on fin unless the call is one pass that is small or stays on its lane; the
    bucket reduction on st unless ZKC_REDUCE_STREAM moves a full pass' to its own stream"""
    blind_on_st = npasses == 1 and (bool(tree) or lane0 >= 0)
    red_split = bool(red) and not serial and nb >= 32
    return [ST, ST2, ST if blind_on_st else FIN, RED if red_split else ST], blind_on_st, red_split


def test_roles_over_the_grid(run):
    cases = list(grid())
    got = run(cases)
    seen_rot = set()
    for (nb, one_lane, pas, npasses, lane0, tree, lanes, sw, red, serial), g in zip(cases, got):
        plan3, blind_on_st, red_split = today(nb, npasses, lane0, tree, red, serial)
        assert g[5:] == [int(blind_on_st), int(red_split)]                      # the model of stream_order agrees with the header
        rotates = not one_lane and lanes > 1
        if not rotates:
            want = plan3                                                       # a one-lane call: today's plan, field for field, under every switch value
        else:
            n = sw or 1
            want = [ST, ST2 if n >= 2 else ST, FIN if n == 3 else ST, plan3[3]]
            seen_rot.add((n, tuple(want[:3])))
        assert g[:4] == want and g[4] == len(set(want)), (nb, one_lane, pas, npasses, lane0, tree, lanes, sw, red, serial, g)
    assert seen_rot == {(1, (ST, ST, ST)), (2, (ST, ST2, ST)), (3, (ST, ST2, FIN))}


def test_literals(run):
    def case(nb, key_lanes, lane0, npasses, pas=0, tree=0, sw=0, red=0, serial=0):
        one_lane, lanes = call(key_lanes, lane0, npasses)
        return (nb, one_lane, pas, npasses, lane0, tree, lanes, sw, red, serial)
    got = run([
        case(64, 4, -1, 16, pas=7),                    # the benchmark's call: 1 024 voters, sixteen passes over four lanes -> every role on st
        case(64, 4, -1, 16, sw=2), case(64, 4, -1, 16, sw=3),
        case(3, 4, -1, 6, pas=5), case(2, 4, -1, 3, pas=2, tree=1),      # the short and the tree-shaped last pass of a rotating call rotate too
        case(1, 4, -1, 1, tree=1), case(64, 4, -1, 1),                   # a census key's call of ONE pass stays on lane 0: today's plan
        case(64, 1, -1, 11, pas=3), case(64, 1, -1, 11, sw=1),           # a key with one lane (ZKC_LANES=1, or not a census key)
        case(16, 4, 3, 1), case(64, 4, 0, 2, pas=1, sw=1),               # the proving service names the lane
        case(64, 4, -1, 16, red=1), case(64, 4, -1, 16, red=1, serial=1), case(31, 4, -1, 16, red=1),      # the reduction stream is a switch of its own
    ])
    assert [g[:5] for g in got] == [
        [ST, ST, ST, ST, 1],
        [ST, ST2, ST, ST, 2], [ST, ST2, FIN, ST, 3],
        [ST, ST, ST, ST, 1], [ST, ST, ST, ST, 1],
        [ST, ST2, ST, ST, 2], [ST, ST2, FIN, ST, 3],
        [ST, ST2, FIN, ST, 3], [ST, ST2, FIN, ST, 3],
        [ST, ST2, ST, ST, 2], [ST, ST2, FIN, ST, 3],
        [ST, ST, ST, RED, 2], [ST, ST, ST, ST, 1], [ST, ST, ST, ST, 1],
    ]
