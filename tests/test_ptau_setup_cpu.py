"""CPU: Groth16 keys from a prepared powers-of-tau file (include/zkcensus_ptau.h) on host threads (ctx = None).  The .ptau is WRITTEN by tests/ptau_lib.py from known
(tau, alpha, beta) in Python integers and read by csrc/zkc_ptau_parse.h: no shared code.  Held against three things that do not read a .ptau: the seeded generator with the
same waste (zkc_debug_setup_from_waste at gamma = delta = 1, itself held against zkc_setup_from_r1cs), every exponent of the key recomputed in Python, and
hashlib for the circuit hash.  Each refusal of the reader fires on a file changed to provoke it, the reader runs under ASan + UBSan as its own program, and the sanity
checks refuse a file with two blocks swapped or one point replaced."""
import ctypes, hashlib, os, random, struct, subprocess
import pytest
import oracle_lib as ol
import closed_form as cf
import big_circuit
import ptau_lib as pl
from zkcensus_amd import _native, setup

ROOT, R, Q = ol.ROOT, ol.R, ol.Q
FMT = 5                                                        # ZKC_ERR_FORMAT
NEW_ENTRY_POINTS = sorted(['zkc_setup_from_ptau', 'zkc_zkey_verify_circuit', 'zkc_setup_ptau_stats', 'zkc_debug_setup_from_waste'])
TAU, ALPHA, BETA = 0x1f3a5c7e9b2d4f6081a3c5e7092b4d6f8fa1c3e5072 % R, 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da5 % R, 0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251 % R


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_ptau.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert '#include "zkcensus_ptau.h"' in open(os.path.join(ROOT, 'include', 'zkcensus.h')).read()


def from_waste(r1cs_path, waste, zkey, vkey):
    err = ctypes.create_string_buffer(512)
    rc = _native.load().zkc_debug_setup_from_waste(os.fsencode(r1cs_path), *[ol.le32(x) for x in waste], os.fsencode(zkey), os.fsencode(vkey), err, 512)
    assert rc == 0, err.value


def test_waste_hook_reproduces_the_seeded_generator(tmp_path):
    r, z, v = setup.ensure_test_artifacts(10, directory=str(tmp_path))
    from_waste(r, cf.toxic_waste(setup.DEFAULT_SEED), tmp_path / 'w.zkey', tmp_path / 'w.json')
    assert open(tmp_path / 'w.zkey', 'rb').read() == open(z, 'rb').read()
    assert open(tmp_path / 'w.json', 'rb').read() == open(v, 'rb').read()
    err = ctypes.create_string_buffer(512)
    bad = [1, 2, 3, 4, R]
    assert _native.load().zkc_debug_setup_from_waste(os.fsencode(r), *[x.to_bytes(32, 'little') for x in bad], os.fsencode(tmp_path / 'x'), None, err, 512) == 4 and b'outside [1, r)' in err.value


# ---- the files: one set of section bodies per (power, waste), shared and never changed ----
_secs = {}


def secs(power, tau=TAU, alpha=ALPHA, beta=BETA):
    key = (power, tau, alpha, beta)
    if key not in _secs:
        _secs[key] = pl.sections(power, tau, alpha, beta)
    return {i: bytearray(b) for i, b in _secs[key].items()}


def ptau_file(path, power, change=None, order=None, **kw):
    s = secs(power, **kw)
    if change:
        change(s)
    open(path, 'wb').write(pl.assemble(s, order))
    return str(path)


def instance(tmp_path, power, seed=1):
    n_pub = 2 + power % 2
    n_cons = (1 << power) - n_pub - 1 - (power == 6)          # power 6: one row of the domain stays empty
    p = str(tmp_path / ('c%d.r1cs' % power))
    big_circuit.big_instance(p, n_cons, n_cons + 5, n_pub, seed)
    return p


def refused(r1cs_path, ptau_path, tmp_path):
    out = tmp_path / 'never.zkey'
    with pytest.raises(_native.ZkcError) as ei:
        setup.from_ptau(r1cs_path, ptau_path, out, tmp_path / 'never.json')
    assert ei.value.code == FMT and not out.exists() and not (tmp_path / 'never.json').exists()
    return str(ei.value)


@pytest.mark.parametrize('power,file_power', [(4, 4), (5, 5), (6, 6), (4, 6)])
def test_key_equals_the_seeded_generator_with_the_same_waste(tmp_path, power, file_power):
    """sections 2 - 9 and the verification key; file_power > power: the blocks are found at their offsets inside larger sections, in a file whose sections are out of order"""
    r = instance(tmp_path, power)
    p = ptau_file(tmp_path / 'a.ptau', file_power, order=[1, 7, 15, 14, 13, 12, 6, 5, 4, 3, 2] if file_power != power else None)
    setup.from_ptau(r, p, tmp_path / 'p.zkey', tmp_path / 'p.json')
    from_waste(r, [TAU, ALPHA, BETA, 1, 1], tmp_path / 'w.zkey', tmp_path / 'w.json')
    a, b = pl.zkey_sections(open(tmp_path / 'p.zkey', 'rb').read()), pl.zkey_sections(open(tmp_path / 'w.zkey', 'rb').read())
    for s in range(1, 10):
        assert a[s] == b[s], 'section %d' % s
    assert open(tmp_path / 'p.json', 'rb').read() == open(tmp_path / 'w.json', 'rb').read()
    assert a[10][64:] == bytes(4) and a[10][:64] != bytes(64)
    assert struct.unpack_from('<I', a[2], 80)[0] == 1 << power
    ms = setup.ptau_stats()
    assert ms['upload'] == 0 and ms['accumulate_reduce'] > 0


CRAFT = [([(0, 1), (1, R - 1), (2, 2)], [(1, 1), (3, R - 2)], [(4, 1)]),                  # unit, minus one, small, small negative
         ([(2, 1)], [(2, 1)], [(5, 1)]),                                                  # a squaring: K adds alpha L and beta L of one row with coefficient 1
         ([(3, 1 << 253)], [(3, 1 << 253), (1, 7)], []),                                  # 2^253; C empty
         ([(4, 0x123456789abcdef0fedcba9876543210aabbccddeeff00112233445566778899 % R), (5, 0)], [(0, 5)], [(6, 3), (6, R - 3)]),      # a zero coefficient; a wire twice in one side
         ([(6, (R - 1) // 2), (1, (R + 1) // 2)], [(6, 1)], [(0, 1)])] + \
        [([(1 + k % 5, 3 + k)], [(2, 1)], [(1 + (k + 1) % 6, R - 1)]) for k in range(6)] + \
        [([(7, 1)], [(7, 1)], []), ([(7, 12345)], [(7, 12345)], [])]                       # wire 7: squared, C empty.  13 constraints, 1 public: domain 16


@pytest.mark.parametrize('waste', ['plain', 'alpha=beta', 'alpha=-beta', 'tau=root'])
def test_every_point_is_its_exponent_times_the_generator(tmp_path, waste):
    """power 4, every A, B1, B2, K and H point, the header points and the circuit hash.  alpha = beta: K takes P + P; alpha = -beta: P - P, K is infinity where C is empty;
    tau on the domain: every Lagrange point but one is infinity, and so is all of H"""
    tau, alpha, beta = {'plain': (TAU, ALPHA, BETA), 'alpha=beta': (TAU, ALPHA, ALPHA), 'alpha=-beta': (TAU, R - BETA, BETA), 'tau=root': (pow(pl.root_of_unity(4), 5, R), ALPHA, BETA)}[waste]
    n_wires, n_pub = 8, 1
    r = pl.write_r1cs(tmp_path / 'c.r1cs', n_wires, n_pub, CRAFT)
    p = ptau_file(tmp_path / 'a.ptau', 4, tau=tau, alpha=alpha, beta=beta)
    setup.from_ptau(r, p, tmp_path / 'p.zkey', tmp_path / 'p.json')
    s = pl.zkey_sections(open(tmp_path / 'p.zkey', 'rb').read())
    logn, A, B, K, H = pl.key_exponents(n_wires, n_pub, CRAFT, tau, alpha, beta)
    assert logn == 4
    assert s[5] == b''.join(pl.g1_mont(x) for x in A) and s[6] == b''.join(pl.g1_mont(x) for x in B) and s[7] == b''.join(pl.g2_mont(x) for x in B)
    assert s[3] == b''.join(pl.g1_mont(x) for x in K[:n_pub + 1]) and s[8] == b''.join(pl.g1_mont(x) for x in K[n_pub + 1:])
    assert s[9] == b''.join(pl.g1_mont(x) for x in H)
    hdr = pl.g1_mont(alpha) + pl.g1_mont(beta) + pl.g2_mont(beta) + pl.g2_mont(1) + pl.g1_mont(1) + pl.g2_mont(1)
    assert s[2][84:] == hdr
    if waste == 'alpha=-beta':
        assert K[7] == 0 and A[7] != 0 and s[8][64 * (7 - n_pub - 1):64 * (7 - n_pub)] == bytes(64)          # wire 7: the same coefficients in A and B of its rows, C empty
    if waste == 'tau=root':
        assert s[9] == bytes(64 * 16)
    # the circuit hash, restated: uncompressed big-endian standard form, G2 components c1 before c0, infinity = 0x40 then zeros; counts as u32 big endian
    inv = pow(1 << 256, -1, Q)

    def unc(m):
        if not any(m): return bytes([0x40]) + bytes(len(m) - 1)
        c = [(int.from_bytes(m[i:i + 32], 'little') * inv % Q).to_bytes(32, 'big') for i in range(0, len(m), 32)]
        return b''.join(c if len(c) == 2 else [c[1], c[0], c[3], c[2]])
    pts = lambda sec, w: [sec[i:i + w] for i in range(0, len(sec), w)]
    h = hashlib.blake2b(digest_size=64)
    h.update(unc(hdr[:64]) + unc(hdr[64:128]) + unc(hdr[128:256]) + unc(hdr[256:384]) + unc(hdr[384:448]) + unc(hdr[448:576]))
    for sec, w in ((s[3], 64), (s[9], 64), (s[8], 64), (s[5], 64), (s[6], 64), (s[7], 128)):
        h.update(struct.pack('>I', len(sec) // w)); [h.update(unc(x)) for x in pts(sec, w)]
    assert s[10][:64] == h.digest()


def test_each_refusal_of_the_reader(tmp_path):
    r4, r5 = instance(tmp_path, 4), instance(tmp_path, 5)
    good = ptau_file(tmp_path / 'good.ptau', 4)
    setup.from_ptau(r4, good, tmp_path / 'ok.zkey')                                          # a good file parses, and the JSON is optional
    assert (tmp_path / 'ok.zkey').exists()
    raw = open(good, 'rb').read()
    mut = lambda name, b: (open(tmp_path / name, 'wb').write(b), str(tmp_path / name))[1]
    assert 'bad magic' in refused(r4, mut('m.ptau', b'ptaX' + raw[4:]), tmp_path)
    assert 'unsupported version 2' in refused(r4, mut('v.ptau', raw[:4] + struct.pack('<I', 2) + raw[8:]), tmp_path)
    assert 'runs past the file' in refused(r4, mut('t.ptau', raw[:-1]), tmp_path)
    assert 'runs past the file' in refused(r4, mut('t2.ptau', raw[:8] + struct.pack('<I', 12) + raw[12:]), tmp_path)
    assert 'shorter than a file header' in refused(r4, mut('s.ptau', raw[:11]), tmp_path)

    def other_q(s): s[1][4:36] = R.to_bytes(32, 'little')
    assert "q is not BN254's" in refused(r4, ptau_file(tmp_path / 'q.ptau', 4, other_q), tmp_path)

    def short14(s): del s[14][-64:]
    assert 'length of section 14 does not match power 4' in refused(r4, ptau_file(tmp_path / 'l.ptau', 4, short14), tmp_path)

    def long2(s): s[2] += bytes(64)
    assert 'length of section 2 does not match power 4' in refused(r4, ptau_file(tmp_path / 'l2.ptau', 4, long2), tmp_path)

    def power5(s): s[1][36:40] = struct.pack('<I', 5)
    assert 'does not match power 5' in refused(r4, ptau_file(tmp_path / 'p5.ptau', 4, power5), tmp_path)

    def unprepared(s):
        for i in (12, 13, 14, 15): del s[i]
    assert 'no section 12: run `powersoftau prepare phase2`' in refused(r4, ptau_file(tmp_path / 'u.ptau', 4, unprepared), tmp_path)

    def partly(s): del s[15]
    assert 'no section 15' in refused(r4, ptau_file(tmp_path / 'pp.ptau', 4, partly), tmp_path)
    assert "power 4 is below the circuit's 5" in refused(r5, good, tmp_path)
    assert 'cannot open' in refused(r4, str(tmp_path / 'missing.ptau'), tmp_path)
    assert 'not an r1cs file' in refused(good, good, tmp_path)


def test_bad_points_and_failed_sanity_checks_are_refused(tmp_path):
    r4 = instance(tmp_path, 4)
    b12, b13 = pl.block(4), pl.block(4, 128)

    def swap(s): s[14][b12], s[15][b12] = s[15][b12], s[14][b12]
    assert 'section 14) does not sum to alphaTauG1[0]' in refused(r4, ptau_file(tmp_path / 'sw.ptau', 4, swap), tmp_path)

    def replace12(s): s[12][b12.start + 64 * 3:b12.start + 64 * 4] = pl.g1_mont(5)
    assert 'section 12) does not sum to the G1 generator' in refused(r4, ptau_file(tmp_path / 'r12.ptau', 4, replace12), tmp_path)

    def replace13(s): s[13][b13.start:b13.start + 128] = pl.g2_mont(5)
    assert 'section 13) does not sum to the G2 generator' in refused(r4, ptau_file(tmp_path / 'r13.ptau', 4, replace13), tmp_path)

    def beta2(s): s[6][:] = pl.g2_mont(BETA + 1)
    assert 'sameRatio(G1, betaTauG1[0]; G2, betaG2) fails' in refused(r4, ptau_file(tmp_path / 'b2.ptau', 4, beta2), tmp_path)

    def off_curve(s): s[12][b12.start + 64 * 9] ^= 1
    assert 'section 12 point 24 has a coordinate >= q or is not on the curve' in refused(r4, ptau_file(tmp_path / 'oc.ptau', 4, off_curve), tmp_path)

    def big_coord(s): s[15][b12.start + 64 * 2 + 32:b12.start + 64 * 2 + 64] = (Q + 1).to_bytes(32, 'little')
    assert 'section 15 point 17 has a coordinate' in refused(r4, ptau_file(tmp_path / 'bc.ptau', 4, big_coord), tmp_path)

    def h_point(s): s[12][64 * 31 + 64 * 7 + 5] ^= 0x10                                         # the size-32 block, an odd index: an H point
    assert 'section 12 point 38 has a coordinate' in refused(r4, ptau_file(tmp_path / 'h.ptau', 4, h_point), tmp_path)

    def off_twist(s): s[13][b13.start + 128 * 4 + 40] ^= 1
    assert 'section 13 point 19 has a coordinate >= q or is not on the twist' in refused(r4, ptau_file(tmp_path / 'ot.ptau', 4, off_twist), tmp_path)


def test_ptau_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'ptau_parse_asan')
    cmd = ['g++', '-std=c++17', '-O2', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'ptau_parse_asan.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]
    work = tmp_path / 'files'; work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'ptau reader: ok' in r.stdout, (r.stdout + r.stderr)[-3000:]
