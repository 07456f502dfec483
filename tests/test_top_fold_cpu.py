"""CPU: the list builder of the top-of-tree folding (csrc/zkc_top_fold.h) as a stand-alone host program (tests/host/top_fold_host.cc) under AddressSanitizer + UBSan, over the
nLevels = 10 test key.  For every (Tc, Dc, Ts, Ds) -- D = a proof's depth per tree, T = 0 or K where D > K, K in (2, 3, 8, 9) -- the program checks that the wires of
fold_vmap's lists, the wires summed into a slot and the wires behind the suffix sums hold every wire of a section whose base is not at infinity exactly once; the sizes of the
lists are compared here with a brute-force count from the key's own sections."""
import os
import struct
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 10
KS = (2, 3, 8, 9)


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
    nvars, npub, _ = struct.unpack_from('<III', h, 8 + n8q + n8r)
    L = Layout(NL)
    assert L.nWires == nvars and npub == 8
    zero = lambda s, cnt: ~np.frombuffer(s, dtype=np.uint8, count=64 * cnt).reshape(cnt, 64).any(axis=1)
    inf = np.zeros((nvars, 3), dtype=bool)
    inf[:, 0] = zero(sec[5], nvars); inf[:, 1] = zero(sec[6], nvars); inf[npub + 1:, 2] = zero(sec[8], nvars - npub - 1)
    return L, nvars, npub, inf


def test_lists_slots_and_suffix_sums_partition_every_section(key, tmp_path):
    L, nvars, npub, inf = key
    n = L.n
    exe = str(tmp_path / 'top_fold_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'top_fold_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the checks of the program itself still run
    assert b.returncode == 0, b.stderr[-3000:]
    head = [n, L.off_census, L.off_sikver, L.off_n2bold] + [L.lvl_off(i) for i in range(n)] + [nvars, npub]
    inp, outp = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(np.array(head, dtype='<u4').tobytes() + inf.astype('<u4').tobytes() + np.array([len(KS)] + list(KS), dtype='<u4').tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'top fold: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
    got = np.fromfile(outp, dtype='<u4').reshape(-1, 3)

    # brute force: per tree, the non-infinity wires of every level group per section; a list holds the section's live wires minus the groups below T, from D on, and the old-key blocks
    grp = np.zeros((2, n, 3), dtype=np.int64)
    for tree, blk in enumerate((L.off_census, L.off_sikver)):
        for g in range(n - 1):
            nctrl = (g == n - 3) + (0 < g < n - 2) + 1
            a, e = blk + L.lvl_off(g) + nctrl, blk + (L.lvl_off(g + 1) if g + 1 < n - 1 else L.lvl_off(n - 1))
            grp[tree, g] = (~inf[a:e]).sum(axis=0)
        a = blk + L.off_n2bold
        grp[tree, n - 1] = (~inf[a:a + 253 + 127 + 133]).sum(axis=0)
    live = (~inf).sum(axis=0); live[2] = (~inf[npub + 1:, 2]).sum()
    want = []
    for K in KS:
        for Tc in (0, K):
            for Dc in range(n):
                for Ts in (0, K):
                    for Ds in range(n):
                        if (Tc and Dc <= K) or (Ts and Ds <= K):
                            continue
                        want.append(live - grp[0, :Tc].sum(axis=0) - grp[0, Dc:].sum(axis=0) - grp[1, :Ts].sum(axis=0) - grp[1, Ds:].sum(axis=0))
    assert got.shape == (len(want), 3) and (got == np.array(want)).all()
    # folding the top takes wires out of every section
    assert (grp[:, :2].sum(axis=1) > 0).all()
