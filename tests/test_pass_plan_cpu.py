"""CPU: the host decisions of a batch call and its passes (csrc/zkc_pass_plan.h) through a stand-alone host program (tests/host/pass_plan_host.cc) under AddressSanitizer +
UBSan: how a call splits into passes, a proof's depth from its row of fold flags and the early layout's agreement rule, which slot of the top-of-tree table a proof takes or
seeds, the windows / tables / job counts of a pass, and the stream-order booleans.  prove_batch_begin and prove_batch_finish (csrc/zkc_prove.hip) keep no copy of this logic.
The expected values are stated here -- as literals, or by a model written from the rules as the prover's comments give them -- and never through the header."""
import itertools
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SLOT = 0xffff
HIT = 1 << 31
BIG = 10 ** 12
# the nLevels = 160 census key
KEY = dict(c_sec=12, c_h=17, c_deep=15, nv=82754, np=8, n=131072)
NC = KEY['nv'] - KEY['np'] - 1


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('pass_plan')
    exe = str(tmp / 'pass_plan_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'pass_plan_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the program's answers are still checked
    assert b.returncode == 0, b.stderr[-3000:]

    def go(cases):
        """cases: lists of (word, integers ...) -> one list of integers per case"""
        text = ''.join(' '.join(str(int(x)) if not isinstance(x, str) else x for x in c) + '\n' for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
        assert r.returncode == 0 and 'pass plan: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-2] == 'pass plan: %d cases' % len(cases)
        return [[int(x) for x in ln.split()] for ln in lines[:len(cases)]]
    return go


def test_call_split(run):
    assert run([('split', 1024, 96), ('split', 65, 64), ('split', 64, 64), ('split', 1, 64)]) == [[11, 94], [2, 33], [1, 64], [1, 1]]
    assert 10 * 94 + 84 == 1024 and 33 + 32 == 65
    grid = [(B, mi) for mi in (1, 2, 4, 64, 96) for B in range(1, 201)]
    for (B, mi), (npasses, per) in zip(grid, run([('split', B, mi) for B, mi in grid])):
        sizes = [min(per, B - p0) for p0 in range(0, B, per)]                  # the passes as the loop of prove_batch_begin walks them
        assert sum(sizes) == B and len(sizes) == npasses and max(sizes) <= mi and min(sizes) >= 1, (B, mi)
        assert npasses == -(-B // mi)                                          # no more passes than the limit forces
        assert all(s == per for s in sizes[:-1]) and max(sizes) - min(sizes) == per - sizes[-1] < npasses, (B, mi)      # equal passes: the last is short by less than one proof per pass


@pytest.mark.parametrize('n', [11, 4])
def test_flag_rows(run, n):
    row = lambda *on: [1 if g in on else 0 for g in range(n)]
    cases = [row()] + [row(g) for g in range(n - 1)] + [row(n - 1), row(0, n - 1), row(*range(n))] + [row(0, g) for g in range(1, n - 1)] + [row(g, n - 2) for g in range(n - 2)]
    want = [0] + [g + 1 for g in range(n - 1)] + [-1, -1, -1] + [g + 1 for g in range(1, n - 1)] + [n - 1] * (n - 2)
    assert [r[0] for r in run([('depth', n, *c) for c in cases])] == want


def test_early_layout_rule(run):
    n, ok, stride = 4, 0, 2 * 4 + 2
    def voter(census, sik):                                                    # [2][n] flags and the two top-fold words, which the rule does not read
        return census + sik + [0xdead, 0xbeef]
    at = lambda D: [0] * n if D == 0 else [0] * (D - 1) + [1] + [0] * (n - D)          # last set flag below n - 1 at D - 1
    foreign = [0, 0, 0, 1]
    def case(status, early, voters):
        return ('early', n, stride, len(voters), ok, *status, *early, *[x for v in voters for x in v])
    cases = [
        case([0], [2, 1], [voter(at(2), at(1))]),                              # D = early in both trees: agrees
        case([0], [2, 1], [voter(at(3), at(1))]),                              # census D = early + 1
        case([0], [2, 1], [voter(at(2), at(2))]),                              # sik D = early + 1
        case([0], [2, 1], [voter(at(1), at(0))]),                              # shallower than laid out: agrees
        case([0], [3, 3], [voter(foreign, at(0))]),                            # an accepted voter with a foreign row
        case([0], [3, 3], [voter(at(0), foreign)]),
        case([5], [0, 0], [voter(foreign, foreign)]),                          # a rejected voter is skipped whatever its rows say
        case([5, 0, 0, 0], [0, 0, 2, 2, 1, 1, 0, 0], [voter(foreign, at(3)), voter(at(2), at(2)), voter(at(1), at(2)), voter(foreign, foreign)]),      # the first that disagrees
        case([0, 7], [1, 1, 0, 0], [voter(at(1), at(1)), voter(at(3), foreign)]),
    ]
    assert [r[0] for r in run(cases)] == [-1, 0, 0, -1, 0, 0, -1, 2, -1]


def test_top_fold_decisions(run):
    K, S = 2, 4
    def case(dc, ds, words, valid, early=0, nb=None, K=K):
        nb = len(dc) if nb is None else nb
        return ('top', K, S, early, nb, *dc, *ds, *[w for pair in words for w in pair], *valid)
    def want(tc, ts, seeds=()):
        return list(tc) + list(ts) + [len(seeds)] + [x for s in seeds for x in s]
    none3, empty, full = [NO_SLOT] * 3, [0] * (2 * S), [1] * (2 * S)
    cases, expect = [], []
    def add(c, w): cases.append(c); expect.append(w)
    # depth K: no fold, and no seed either; depth K + 1: folds on a hit
    add(case([2, 3, 2], [3, 2, 2], [(HIT | 1, HIT | 2)] * 3, full), want([NO_SLOT, 1, NO_SLOT], [S + 2, NO_SLOT, NO_SLOT]))
    # a hit word against a miss word on a valid slot: the miss neither folds nor seeds
    add(case([5, 5, 5], [5, 5, 5], [(HIT | 3, 3), (3, HIT | 3), (0, 0)], full), want([3, NO_SLOT, NO_SLOT], [NO_SLOT, S + 3, NO_SLOT]))
    # a miss on an empty slot seeds it; two proofs missing on one empty slot give one seed, from the first of them
    add(case([5, 5, 5], [0, 0, 0], [(1, 0), (2, 0), (1, 0)], empty), want(none3, none3, [(0, 0, 1), (1, 0, 2)]))
    # the same slot number in both trees: two seeds
    add(case([5, 0, 0], [5, 0, 0], [(3, 3), (0, 0), (0, 0)], empty), want(none3, none3, [(0, 0, 3), (0, 1, 3)]))
    # valid in the census tree only
    add(case([5, 0, 0], [5, 0, 0], [(3, 3), (0, 0), (0, 0)], [0, 0, 0, 1, 0, 0, 0, 0]), want(none3, none3, [(0, 1, 3)]))
    # slot index nslots: ignored, hit bit or not
    add(case([5, 5, 5], [5, 5, 5], [(S, HIT | S), (HIT | (S + 1), 0x7fffffff), (HIT | 0, 0)], empty), want([NO_SLOT, NO_SLOT, 0], none3, [(2, 1, 0)]))
    # early: nothing
    add(case([5, 5, 5], [5, 5, 5], [(HIT | 1, 1)] * 3, empty, early=1), want(none3, none3))
    # nb = 2: nothing; nb = 3: active
    add(case([5, 5], [5, 5], [(HIT | 1, 1)] * 2, empty), want([NO_SLOT] * 2, [NO_SLOT] * 2))
    add(case([5, 5, 5], [5, 5, 5], [(HIT | 1, 1)] * 3, empty), want([1, 1, 1], none3, [(0, 1, 1)]))
    # K = 0 (the key folds no top, or the pass does not fold): nothing
    add(case([5, 5, 5], [5, 5, 5], [(HIT | 1, 1)] * 3, empty, K=0), want(none3, none3))
    assert run(cases) == expect


def nw(c): return (254 + c) // c
def half(c): return 1 << (c - 1)


def shape_model(k, cap, sw, nb, lists):
    """the rules as the comments of zkc_pass_plan.h and the prover's history state them"""
    nv, nc = k['nv'], k['nv'] - k['np'] - 1
    sizes = lists if lists is not None else [(nv, nv, nc)] * nb
    vws = 64 if nb <= 4 else sw['vw_small'] or (256 if nb < 32 else 2048)
    vwb = 256 if nb <= 4 else sw['vw_big'] or (1024 if nb < 32 else 4096)
    live = sum(a + b + c for a, b, c in sizes)
    deep = k['c_deep'] != 0 and nb > 2 and live >= 3 * sw['deep_wires'] * nb
    cw = k['c_deep'] if deep else k['c_sec']
    tables = (4000, 5000, 6000) if deep else (1000, 2000, 3000)
    lone = nb <= 2 and k['lone_table'] and 32 * sum(b for _, b, _ in sizes) <= cap['w2_entries']
    c2 = 8 if lone else cw
    vwg2 = 128 if lone else (sw['vw_g2'] if sw['vw_g2'] and nb >= 32 else vws)
    entries = sum(nw(k['c_h']) * k['n'] + nw(k['c_sec']) * (2 * a + 2 * b + c) for a, b, c in sizes)
    tree = k['fb4'] and nb <= 2 and 6 * nb <= cap['w1_jobs'] and entries <= cap['w1_entries'] and nb * (5 * half(k['c_sec']) + half(k['c_h'])) <= cap['w1_buckets']
    return [vws, vwb, vwg2, int(deep), cw, *tables, c2, int(tree), 5 if tree else 3]


def shape_case(k, cap, sw, nb, lists):
    return ('shape', k['c_sec'], k['c_h'], k['c_deep'], k['nv'], k['np'], k['n'], k['lone_table'], k['fb4'], cap['w1_entries'], cap['w1_buckets'], cap['w1_jobs'], cap['w2_entries'],
            sw['vw_big'], sw['vw_small'], sw['vw_g2'], sw['deep_wires'], nb, lists is not None, *[x for l in (lists or []) for x in l])


def test_pass_shape(run):
    key = dict(KEY, lone_table=1, fb4=1)
    roomy = dict(w1_entries=BIG, w1_buckets=BIG, w1_jobs=512, w2_entries=BIG)
    dflt = dict(vw_big=0, vw_small=0, vw_g2=0, deep_wires=16000)
    over = dict(vw_big=8192, vw_small=512, vw_g2=1024, deep_wires=16000)
    voter = (9000, 6000, 9000)                                                 # a folded voter's lists
    cases = []
    for nb, sw, lists in itertools.product((1, 2, 3, 4, 5, 31, 32, 64), (dflt, over), (None, voter)):
        cases.append((key, roomy, sw, nb, None if lists is None else [lists] * nb))
    # deep exactly at live_wires = 3 * deep_wires * nb and one below; never at nb <= 2 or without second tables
    for dw in (16000, 1):
        sw = dict(dflt, deep_wires=dw)
        cases += [(key, roomy, sw, 3, [(dw, dw, dw)] * 3), (key, roomy, sw, 3, [(dw, dw, dw)] * 2 + [(dw, dw, dw - 1)]), (key, roomy, sw, 2, [(80000, 80000, 80000)] * 2), (key, roomy, sw, 2, None),
                  (dict(key, c_deep=0), roomy, sw, 3, [(80000, 80000, 80000)] * 3), (dict(key, c_deep=0), roomy, sw, 64, None)]
    # the lone G2 table: nb <= 2, the table exists, 32 entries per listed B scalar fit the G2 work space -- at equality and one entry short
    for nb in (1, 2, 3):
        fit = 32 * 6000 * nb
        cases += [(key, dict(roomy, w2_entries=fit), dflt, nb, [voter] * nb), (key, dict(roomy, w2_entries=fit - 1), dflt, nb, [voter] * nb), (dict(key, lone_table=0), roomy, dflt, nb, [voter] * nb)]
    cases += [(key, dict(roomy, w2_entries=32 * KEY['nv']), dflt, 1, None), (key, dict(roomy, w2_entries=32 * KEY['nv'] - 1), dflt, 1, None)]
    # the tree form: nb <= 2, six jobs per proof, the entries of 5 sections + H, the buckets of 5 sections + H -- each at equality and one past it
    for nb, lists in ((1, [voter]), (2, [voter, (9001, 6001, 9001)]), (1, None), (2, None), (3, [voter] * 3)):
        sizes = lists if lists is not None else [(KEY['nv'], KEY['nv'], NC)] * nb
        entries = sum(15 * 131072 + 22 * (2 * a + 2 * b + c) for a, b, c in sizes)
        buckets = nb * (5 * 2048 + 65536)
        exact = dict(roomy, w1_jobs=6 * nb, w1_entries=entries, w1_buckets=buckets)
        cases += [(key, exact, dflt, nb, lists), (key, dict(exact, w1_jobs=6 * nb - 1), dflt, nb, lists), (key, dict(exact, w1_entries=entries - 1), dflt, nb, lists),
                  (key, dict(exact, w1_buckets=buckets - 1), dflt, nb, lists), (dict(key, fb4=0), exact, dflt, nb, lists)]
    got = run([shape_case(*c) for c in cases])
    assert got == [shape_model(*c) for c in cases]
    by = {(c[3], id(c[2]), c[4] is None): g for c, g in zip(cases[:32], got[:32])}
    # the literal table of windows: (sections, H, G2) per pass size, the overrides honoured only above four proofs (G2: from 32)
    for nb, want_d, want_o in ((1, (64, 256, 128), (64, 256, 128)), (2, (64, 256, 128), (64, 256, 128)), (3, (64, 256, 64), (64, 256, 64)), (4, (64, 256, 64), (64, 256, 64)),
                               (5, (256, 1024, 256), (512, 8192, 512)), (31, (256, 1024, 256), (512, 8192, 512)), (32, (2048, 4096, 2048), (512, 8192, 1024)), (64, (2048, 4096, 2048), (512, 8192, 1024))):
        assert tuple(by[(nb, id(dflt), False)][:3]) == want_d and tuple(by[(nb, id(over), False)][:3]) == want_o, nb
    # per is 5 exactly when the pass takes the tree form; c2 = 8 only in passes of one or two; a folded voter's pass is never deep, an unlisted pass of three is
    assert all(g[10] == (5 if g[9] else 3) for g in got) and any(g[9] for g in got) and not all(g[9] for g in got)
    assert all(c[3] <= 2 for c, g in zip(cases, got) if g[8] == 8) and all(g[9] == 0 for c, g in zip(cases, got) if c[3] > 2)
    assert by[(3, id(dflt), False)][3:8] == [0, 12, 1000, 2000, 3000] and by[(3, id(dflt), True)][3:8] == [1, 15, 4000, 5000, 6000] and by[(2, id(dflt), True)][3] == 0
    deep_at = [g[3] for g in got[32:44]]
    assert deep_at == [1, 0, 0, 0, 0, 0] * 2


def test_proof_views(run):
    nv, np_ = 100, 8
    nc = nv - np_ - 1
    got = run([('views', nv, np_, 1, 0, 40, 40, 30, 70, 25), ('views', nv, np_, 0, 0, 0, 0, 0, 0, 0)])
    # per section: scalars - w, vmap - d, count, table offset, table count, pt_shift
    assert got[0] == [0, 0, 40, 1000, nv, 0] + [0, 40, 30, 2000, nv, 0] + [0, 70, 25, 3000, nc, np_ + 1]
    assert got[1] == [0, -1, nv, 1000, nv, 0] + [0, -1, nv, 2000, nv, 0] + [8 * (np_ + 1), -1, nc, 3000, nc, 0]


def test_stream_booleans(run):
    grid = list(itertools.product((31, 32), (0, 1), (0, 1), (1, 2), (-1, 0), (0, 1), *[(0, 1)] * 5))
    got = run([('order', *g) for g in grid])
    for (nb, one_lane, pas, npasses, lane0, tree, mv_inline, hold, early, red, serial), g in zip(grid, got):
        prefetch = bool(one_lane) and not mv_inline
        want = [prefetch, prefetch and pas > 0,
                bool(hold) or ((nb < 32 or not one_lane) and not early),
                bool(red) and not serial and nb >= 32,
                npasses == 1 and (bool(tree) or lane0 >= 0)]
        assert g == [int(x) for x in want], (nb, one_lane, pas, npasses, lane0, tree, mv_inline, hold, early, red, serial)
    # each output takes both values, and each switch changes what it should
    assert all({g[i] for g in got} == {0, 1} for i in range(5))
