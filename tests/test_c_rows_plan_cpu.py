"""CPU: when a pass leaves out the transform pair of C (csrc/zkc_pass_plan.h: c_rows_rule, c_rows) and the list its H job then runs over (h_vmap), through a stand-alone
host program (tests/host/c_rows_plan_host.cc) under AddressSanitizer + UBSan.  The rule is k nw_H <= beta n log2 n; the expected values are literals or the rule as this
file writes it, never the header."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 10 ** 12


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('c_rows_plan')
    exe = str(tmp / 'c_rows_plan_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'c_rows_plan_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the program's answers are still checked
    assert b.returncode == 0, b.stderr[-3000:]

    def go(cases):
        text = ''.join(' '.join(str(int(x)) if not isinstance(x, str) else x for x in c) + '\n' for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
        assert r.returncode == 0 and 'c rows plan: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-2] == 'c rows plan: %d cases' % len(cases)
        return [[int(x) for x in ln.split()] for ln in lines[:len(cases)]]
    return go


def test_rule_at_its_edges(run):
    # 16-bit windows: nw_H = (254 + 16) // 16 = 16.  beta = 0.125: 0.125 x 4096 x 12 / 16 = 384 rows at n = 2^12, 0.125 x 131072 x 17 / 16 = 17408 at n = 2^17, both exact
    cases, want = [], []
    for n, logn, bound in ((1 << 12, 12, 384), (1 << 17, 17, 17408)):
        assert 125 * n * logn == bound * 16 * 1000
        for k, ok in ((bound - 1, 1), (bound, 1), (bound + 1, 0), (0, 1)):
            cases.append(('rule', k, 16, n, logn, 125)); want.append([ok])
    # the census key: 17-bit windows, nw_H = 15, the default beta = 0.120 -> 17825.79 rows at n = 2^17, 393.2 at n = 2^12
    cases += [('rule', 17825, 15, 1 << 17, 17, 120), ('rule', 17826, 15, 1 << 17, 17, 120), ('rule', 393, 15, 1 << 12, 12, 120), ('rule', 394, 15, 1 << 12, 12, 120)]
    want += [[1], [0], [1], [0]]
    cases += [('rule', 1, 15, 1 << 12, 12, 0), ('rule', 0, 15, 1 << 12, 12, 0), ('rule', 1 << 17, 15, 1 << 17, 17, 100000)]      # beta 0: only an empty list; a huge beta: every list
    want += [[0], [1], [1]]
    assert run(cases) == want


def take(c_h=16, n=1 << 12, nb=3, tree=0, mode=1, beta=125, wide=1, abc=1, early=0, k=384, logn=12, sec=0, cap_p=BIG, w1=BIG):
    return ('take', c_h, n, nb, tree, mode, beta, wide, abc, early, k, logn, sec, cap_p, w1)


def test_which_passes_take_the_path(run):
    n, nw = 1 << 12, 16
    cases = [take(), take(k=385), take(k=385, mode=2), take(mode=0), take(mode=2, k=n)]
    want = [[1, 1], [0, 0], [1, 1], [0, 0], [1, 1]]
    # everything that keeps the pair of three vectors, rule satisfied or path forced: a tree-shaped pass, one or two proofs, a pass laid out early, buildABC not folded
    # (an unfolded pass, the prefetched buildABC, ZKC_ABC_FOLD=0), a key with the narrow H table
    for kw in (dict(tree=1), dict(nb=2), dict(nb=1), dict(early=1), dict(abc=0), dict(wide=0)):
        cases += [take(**kw), take(mode=2, **kw)]; want += [[0, 0], [0, 0]]                 # ... and none of them is a candidate: no list is counted for it
    # the lane's caps: sections + nb x nw x (n + k) entries must fit w1, nb x 16 n words the H-scalar buffer
    nb, k, sec = 5, 100, 7777
    need = sec + nb * nw * (n + k)
    cases += [take(nb=nb, k=k, sec=sec, w1=need), take(nb=nb, k=k, sec=sec, w1=need - 1), take(nb=nb, k=k, sec=sec, w1=need - 1, mode=2),
              take(nb=nb, k=k, cap_p=nb * 16 * n), take(nb=nb, k=k, cap_p=nb * 16 * n - 1), take(nb=nb, k=k, cap_p=nb * 8 * n, mode=2)]
    want += [[1, 1], [0, 1], [0, 1], [1, 1], [0, 1], [0, 1]]                               # (candidates all: the caps are asked last)
    assert run(cases) == want


def test_h_job_list(run):
    n = 16
    got = run([('vmap', n, 0), ('vmap', n, 1, 5), ('vmap', n, 3, 0, 7, n - 1), ('vmap', 1 << 12, 2, 1, (1 << 12) - 1)])
    ident = list(range(n))
    assert got[0] == ident and got[1] == ident + [n + 5] and got[2] == ident + [n, n + 7, 2 * n - 1]
    assert got[3] == list(range(1 << 12)) + [(1 << 12) + 1, (1 << 13) - 1]
    for v in got:
        assert v == sorted(v) and len(set(v)) == len(v)                       # ascending, no entry twice
