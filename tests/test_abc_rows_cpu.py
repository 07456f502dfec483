"""CPU: the row classes behind buildABC's template copy (csrc/zkc_abc_rows.h) as a stand-alone host program (tests/host/abc_rows_host.cc) under AddressSanitizer + UBSan, over
the nLevels = 10 test key, against a brute-force classification in Python from the key's coefficient section: a row is constant at depths (Dc, Ds) when each of its wires is
wire 0 or a non-control wire of a level >= Dc of the census tree or >= Ds of the sik tree -- what zkc_fold_check compares with the template for a proof of those depths.
The lists are compared entry for entry, order included (jagged-diagonal order: rows by decreasing length, equal lengths in input order), for every pair of depths in
{0, 1, 9, 10}; (10, 10) lists every row that holds a wire other than wire 0, (0, 0) is non-empty and shorter."""
import os
import struct
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 10
DEPTHS = (0, 1, 9, 10)
MATVEC_LONG = 16                    # zkc_prove.hip: rows with more coefficients are summed by a whole wave


def sections(zkey):
    assert zkey[:4] == b'zkey'
    nsec = struct.unpack_from('<I', zkey, 8)[0]
    at, out = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from('<IQ', zkey, at)
        out[typ] = zkey[at + 12:at + 12 + size]
        at += 12 + size
    return out


@pytest.fixture(scope='module')
def key():
    from zkcensus_amd import setup
    from zkcensus_amd.r1cs import Layout
    _, zp, _ = setup.ensure_test_artifacts(NL)
    sec = sections(open(zp, 'rb').read())
    h = sec[2]
    n8q = struct.unpack_from('<I', h, 0)[0]; n8r = struct.unpack_from('<I', h, 4 + n8q)[0]
    nvars, npub, ncons = struct.unpack_from('<III', h, 8 + n8q + n8r)
    ncoef = struct.unpack_from('<I', sec[4], 0)[0]
    co = np.frombuffer(sec[4], dtype=np.uint8, count=44 * ncoef, offset=4).reshape(ncoef, 44)[:, :12].copy().view('<u4').reshape(ncoef, 3)
    L = Layout(NL)
    assert L.nWires == nvars and npub == 8
    return L, nvars, ncons, co


def brute_force(L, nvars, ncons, co):
    """per row: its wires; per wire: None (a voter's), 'one', or (tree, level) with level n - 1 for the old-key block"""
    n = L.n
    group = [None] * nvars
    group[0] = 'one'
    for tree, blk in enumerate((L.off_census, L.off_sikver)):
        for g in range(n - 1):
            nctrl = (g == n - 3) + (0 < g < n - 2) + 1
            for w in range(blk + L.lvl_off(g) + nctrl, blk + (L.lvl_off(g + 1) if g + 1 < n - 1 else L.lvl_off(n - 1))):
                group[w] = (tree, g)
        for w in range(blk + L.off_n2bold, blk + L.off_n2bold + 253 + 127 + 133):
            group[w] = (tree, n - 1)
    rows = [[] for _ in range(2 * ncons)]
    for m, c, s in co.tolist():
        rows[m * ncons + c].append(s)
    return rows, group


def constant(wires, group, n, Dc, Ds):
    for w in wires:
        g = group[w]
        if g == 'one':
            continue
        if g is None or g[1] == n - 1 or g[1] < (Dc, Ds)[g[0]]:
            return False
    return True


def test_voter_row_lists_equal_a_brute_force_classification(key, tmp_path):
    L, nvars, ncons, co = key
    exe = str(tmp_path / 'abc_rows_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'abc_rows_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the checks of the program itself still run
    assert b.returncode == 0, b.stderr[-3000:]
    pairs = [(dc, ds) for dc in DEPTHS for ds in DEPTHS]
    head = [L.n, L.off_census, L.off_sikver, L.off_n2bold] + [L.lvl_off(i) for i in range(L.n)] + [nvars, ncons, MATVEC_LONG, len(co)]
    inp, outp = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(np.array(head, dtype='<u4').tobytes() + co.astype('<u4').tobytes() + np.array([len(pairs)] + [x for p in pairs for x in p], dtype='<u4').tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'abc rows: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
    got = np.fromfile(outp, dtype='<u4').tolist()

    rows, group = brute_force(L, nvars, ncons, co)
    order = sorted(range(2 * ncons), key=lambda i: -len(rows[i]))               # stable: equal lengths keep their input order
    never = sum(1 for w in rows if any(group[x] is None or (group[x] != 'one' and group[x][1] == L.n - 1) for x in w))
    assert got[0] == never and got[1] == 2 * ncons - never
    at, lists = 2, {}
    for p in pairs:
        nrows, nlong, nC, nW = got[at:at + 4]; at += 4
        want = [i for i in order if not constant(rows[i], group, L.n, *p)]
        assert got[at:at + nrows] == want, p
        assert nlong == sum(1 for i in want if len(rows[i]) > MATVEC_LONG), p
        at += nrows
        assert got[at:at + nC] == sorted({i % ncons for i in want}), p          # C_i is formed when A row i or B row i is a voter's
        at += nC
        assert got[at:at + nW] == sorted({w for i in want for w in rows[i]}), p
        at += nW
        lists[p] = want
    assert at == len(got)
    assert lists[(10, 10)] == [i for i in order if any(w != 0 for w in rows[i])]
    assert 0 < len(lists[(0, 0)]) < len(lists[(10, 10)])
    # deeper voters can only add rows
    for dc, ds in pairs:
        assert set(lists[(0, 0)]) <= set(lists[(dc, ds)]) <= set(lists[(10, 10)])
