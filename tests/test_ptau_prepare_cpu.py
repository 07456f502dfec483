"""CPU: a powers-of-tau file prepared for phase 2 (include/zkcensus_ptau_prepare.h) on host threads (ctx = None).  The unprepared file and the image a preparer must write
come from tests/ptau_prep_lib.py: Python integers and the oracle's scalar multiplications, no transform over points.  The prepared file is then used as a key source
(setup.from_ptau, against ptau_lib's own prepared file and against the exponents), checked by check_prepared -- which must also catch what from_ptau's own checks accept --
and every refusal fires on a file changed to provoke it.  The open-unprepared path and the writer run under ASan + UBSan as their own program."""
import os, random, struct, subprocess
import pytest
import oracle_lib as ol
import closed_form as cf
import big_circuit
import ptau_lib as pl
import ptau_prep_lib as pp
from zkcensus_amd import _native, setup

ROOT, R, Q = ol.ROOT, ol.R, ol.Q
FMT = 5                                                        # ZKC_ERR_FORMAT
NEW_ENTRY_POINTS = sorted(['zkc_g1_lagrange_dev', 'zkc_g2_lagrange_dev', 'zkc_ptau_prepare', 'zkc_ptau_check_prepared', 'zkc_ptau_prepare_stats'])
WASTE_NAMES = ['plain', 'one', 'minus-one', 'on-domain', 'on-double-domain']


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_ptau_prepare.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert '#include "zkcensus_ptau_prepare.h"' in open(os.path.join(ROOT, 'include', 'zkcensus.h')).read()


def test_the_integer_transform_is_the_definition():
    rng = random.Random(5)
    for logn in (0, 1, 2, 3, 5):
        ks = [rng.randrange(R) for _ in range(1 << logn)]
        assert pp.intt(ks, logn) == pp.direct_intt(ks, logn)
    # and the top block in the exponent is the transform of the padded monomial vector
    for power, tau in ((1, 7), (3, pp.PLAIN[0]), (2, pl.root_of_unity(3))):
        n2 = 2 << power
        assert pp.top_block_exponents(power, tau) == pp.intt([pow(tau, i, R) for i in range(n2 - 1)] + [0], power + 1)
        if pow(tau, n2, R) != 1:
            assert pl.lagrange_at(tau, power + 1) == pp.intt([pow(tau, i, R) for i in range(n2)], power + 1)


def write(path, img):
    open(path, 'wb').write(img)
    return str(path)


@pytest.mark.parametrize('waste', WASTE_NAMES)
@pytest.mark.parametrize('power', [1, 2, 3, 4])
def test_prepared_file_is_the_expected_image(tmp_path, power, waste):
    unprepared, expected, _ = pp.images(power, pp.wastes(power)[waste])
    src, dst = write(tmp_path / 'in.ptau', unprepared), str(tmp_path / 'out.ptau')
    assert setup.prepare_ptau(src, dst) == dst
    got = open(dst, 'rb').read()
    order, body = pp.parse(got)
    assert order == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    _, inb = pp.parse(unprepared)
    for i in range(1, 8):
        assert body[i] == inb[i], 'section %d is not the input\'s' % i
    _, exp = pp.parse(expected)
    for i in (12, 13, 14, 15):
        w = pl.PT_BYTES[i]
        diff = [k for k in range(len(exp[i]) // w) if body[i][w * k:w * k + w] != exp[i][w * k:w * k + w]]
        assert len(body[i]) == len(exp[i]) and diff == [], 'section %d points %r' % (i, diff[:8])
    assert got == expected
    assert sorted(os.listdir(tmp_path)) == ['in.ptau', 'out.ptau']      # no temporary file left
    if waste == 'on-domain' and power >= 2:
        blk = body[13][pl.block(power, 128)]
        assert sum(any(blk[128 * k:128 * k + 128]) for k in range(1 << power)) == 1       # the indicator: one point, the rest infinity
    ms = setup.ptau_prepare_stats()
    assert ms['transforms_g1'] > 0 and ms['transforms_g2'] > 0 and ms['affine_download'] == 0


def test_sections_are_copied_in_the_inputs_order_with_unknown_ones(tmp_path):
    _, _, secs = pp.images(2, pp.PLAIN)
    s = {i: secs[i] for i in range(1, 8)}
    s[7] = struct.pack('<I', 1) + bytes(range(200))             # never parsed
    s[9] = b'left alone'
    order = [7, 5, 1, 9, 3, 2, 6, 4]
    src, dst = write(tmp_path / 'in.ptau', pl.assemble(s, order)), str(tmp_path / 'out.ptau')
    setup.prepare_ptau(src, dst)
    got_order, body = pp.parse(open(dst, 'rb').read())
    assert got_order == order + [12, 13, 14, 15] and body[7] == s[7] and body[9] == s[9]
    _, exp = pp.parse(pp.images(2, pp.PLAIN)[1])
    assert all(body[i] == exp[i] for i in (12, 13, 14, 15))
    assert setup.check_prepared(dst) == (True, 0, 0, '')


# ---- use as a key source ----
TAU, ALPHA, BETA = pp.PLAIN


def prepared_here(tmp_path, power, waste=pp.PLAIN, name='here.ptau'):
    src = write(tmp_path / ('un_' + name), pp.images(power, waste)[0])
    return setup.prepare_ptau(src, str(tmp_path / name))


def instance(tmp_path, power, seed=1):
    n_pub = 2 + power % 2
    raw = str(tmp_path / ('raw%d.r1cs' % power))
    wtns = big_circuit.big_instance(raw, (1 << power) - n_pub - 1, (1 << power) + 5, n_pub, seed)       # a satisfiable instance and its witness ...
    return pl.write_r1cs(str(tmp_path / ('c%d.r1cs' % power)), *cf.read_r1cs(raw)), wtns                   # ... written by ptau_lib.write_r1cs, as every circuit of these tests is


def test_key_from_the_prepared_file_below_the_files_power(tmp_path):
    """cirPower < power: no block that differs is read, the key is ptau_lib's file's key byte for byte"""
    r, _ = instance(tmp_path, 3)
    here = prepared_here(tmp_path, 4)
    theirs = write(tmp_path / 'lib.ptau', pl.assemble(pp.images(4, pp.PLAIN)[2]))
    setup.from_ptau(r, here, tmp_path / 'a.zkey', tmp_path / 'a.json')
    setup.from_ptau(r, theirs, tmp_path / 'b.zkey', tmp_path / 'b.json')
    assert open(tmp_path / 'a.zkey', 'rb').read() == open(tmp_path / 'b.zkey', 'rb').read()
    assert open(tmp_path / 'a.json', 'rb').read() == open(tmp_path / 'b.json', 'rb').read()


def test_key_at_the_files_power_has_the_padded_h_points_and_proves(tmp_path, monkeypatch):
    """cirPower == power: H (section 9) is the odd half of the padded top block and sections 1 - 8 are ptau_lib's file's.  Section 10 opens with the circuit hash, which is
    taken over the H points among others (include/zkcensus_ptau.h), so it differs with them and cannot be equal: that it does differ is asserted, and the rest of section 10
    (no contributions) is equal.  A proof under the key is the closed form and verifies"""
    import json
    power = 4
    r, wtns = instance(tmp_path, power)
    here = prepared_here(tmp_path, power)
    theirs = write(tmp_path / 'lib.ptau', pl.assemble(pp.images(power, pp.PLAIN)[2]))
    setup.from_ptau(r, here, tmp_path / 'a.zkey', tmp_path / 'a.json')
    setup.from_ptau(r, theirs, tmp_path / 'b.zkey', tmp_path / 'b.json')
    za = open(tmp_path / 'a.zkey', 'rb').read()
    a, b = pl.zkey_sections(za), pl.zkey_sections(open(tmp_path / 'b.zkey', 'rb').read())
    for s in (1, 2, 3, 4, 5, 6, 7, 8):
        assert a[s] == b[s], 'section %d' % s
    assert open(tmp_path / 'a.json', 'rb').read() == open(tmp_path / 'b.json', 'rb').read()
    top = pp.top_block_exponents(power, TAU)
    assert a[9] == b''.join(pl.g1_mont(top[2 * i + 1]) for i in range(1 << power))
    assert a[9] != b[9] and a[10][:64] != b[10][:64] and a[10][64:] == b[10][64:]      # the H points differ, and the circuit hash with them; nothing else of section 10 does
    rc, proof, pub = ol.prove(za, wtns, 12345, R - 6, npub=2 + power % 2)
    assert rc == 0 and pub == wtns[32:32 * (3 + power % 2)]
    assert ol.verify(json.load(open(tmp_path / 'a.json')), pub, proof)
    monkeypatch.setattr(cf, 'toxic_waste', lambda seed: [TAU, ALPHA, BETA, 1, 1])
    assert proof == cf.proof_from_scalars(ol, *cf.proof_scalars(r, 0, wtns, 12345, R - 6))


# ---- check_prepared ----
def changed(tmp_path, img, edits, name):
    m = bytearray(img); off = pp.offsets(img)
    for sec, at, val in edits:
        m[off[sec] + at:off[sec] + at + len(val)] = val
    return write(tmp_path / name, bytes(m))


def test_check_prepared_names_the_first_point_that_differs(tmp_path):
    power = 3
    here = prepared_here(tmp_path, power)
    assert setup.check_prepared(here) == (True, 0, 0, '')
    img = open(here, 'rb').read()
    flip = lambda sec, pt, byte=5: (sec, pl.PT_BYTES[sec] * pt + byte, bytes([pp.parse(img)[1][sec][pl.PT_BYTES[sec] * pt + byte] ^ 1]))
    for sec, pt in ((12, 9), (12, 30), (13, 0), (13, 14), (14, 7), (15, 2)):
        ok, s, i, why = setup.check_prepared(changed(tmp_path, img, [flip(sec, pt, 40)], 'one.ptau'))
        assert (ok, s, i) == (False, sec, pt) and why == 'ptau: section %d point %d is not the transform of section %d' % (sec, pt, sec - 10)
    # two changes: the earlier one is named -- by section first, then by index
    assert setup.check_prepared(changed(tmp_path, img, [flip(14, 1), flip(13, 12)], 'two.ptau'))[:3] == (False, 13, 12)
    assert setup.check_prepared(changed(tmp_path, img, [flip(15, 11), flip(15, 4)], 'two.ptau'))[:3] == (False, 15, 4)
    assert setup.ptau_prepare_stats()['write_or_compare'] > 0


def test_check_prepared_catches_a_shift_that_the_key_generator_accepts(tmp_path):
    """D added to L_3 and -D to L_5 of the size-2^power block of section 12: every point is on the curve and the basis still sums to the generator, so from_ptau takes the
    file for a circuit whose rows do not touch those points -- and check_prepared names L_3"""
    power = 3
    here = prepared_here(tmp_path, power)
    img = open(here, 'rb').read()
    lag = pl.lagrange_at(TAU, power)
    D = 0x1234567
    b = pl.block(power)
    edits = [(12, b.start + 64 * 3, pl.g1_mont(lag[3] + D)), (12, b.start + 64 * 5, pl.g1_mont(lag[5] - D))]
    shifted = changed(tmp_path, img, edits, 'shift.ptau')
    # four constraints, the fourth empty, no public wire: rows 0, 1, 2 and wire 0's extra row 4 of the domain of 8 are in use, rows 3 and 5 are not
    r = pl.write_r1cs(tmp_path / 'tiny.r1cs', 5, 0, [([(1, 1)], [(2, 1)], [(3, 1)]), ([(3, 2)], [(1, 5)], [(4, 1)]), ([(4, 1)], [(4, R - 1)], []), ([], [], [])])
    setup.from_ptau(r, shifted, tmp_path / 's.zkey', tmp_path / 's.json')                      # the hole: accepted
    setup.from_ptau(r, here, tmp_path / 'h.zkey', tmp_path / 'h.json')
    assert open(tmp_path / 's.zkey', 'rb').read() == open(tmp_path / 'h.zkey', 'rb').read()
    ok, s, i, why = setup.check_prepared(shifted)
    assert (ok, s, i) == (False, 12, (1 << power) - 1 + 3) and 'section 12 point %d is not the transform of section 2' % ((1 << power) - 1 + 3) in why


@pytest.mark.parametrize('power', [1, 3])
def test_check_prepared_refuses_the_true_top_block(tmp_path, power):
    theirs = write(tmp_path / 'lib.ptau', pl.assemble(pp.images(power, pp.PLAIN)[2]))
    assert setup.check_prepared(theirs)[:3] == (False, 12, (2 << power) - 1)


# ---- refusals ----
def refused(src, tmp_path, dst=None):
    out = tmp_path / 'never.ptau' if dst is None else dst
    with pytest.raises(_native.ZkcError) as ei:
        setup.prepare_ptau(src, out)
    assert ei.value.code == FMT
    assert not os.path.exists(out) and not [f for f in os.listdir(tmp_path) if '.tmp' in f]
    return str(ei.value)


def test_each_refusal_of_prepare(tmp_path):
    power = 2
    unprepared, expected, secs = pp.images(power, pp.PLAIN)
    base = {i: bytearray(secs[i]) for i in range(1, 8)}
    assert 'already prepared (it has section 12)' in refused(write(tmp_path / 'p.ptau', expected), tmp_path)
    only14 = dict(base); only14[14] = secs[14]
    assert 'already prepared (it has section 14)' in refused(write(tmp_path / 'p14.ptau', pl.assemble(only14)), tmp_path)
    no3 = {i: b for i, b in base.items() if i != 3}
    assert 'ptau: no section 3' in refused(write(tmp_path / 'n3.ptau', pl.assemble(no3)), tmp_path)
    off = {i: bytearray(b) for i, b in base.items()}; off[2][64 * 5 + 3] ^= 1; off[2][64 * 6] ^= 1          # two bad points: the smaller index is named
    assert 'ptau: section 2 point 5 has a coordinate >= q or is not on the curve' in refused(write(tmp_path / 'oc.ptau', pl.assemble(off)), tmp_path)
    big = {i: bytearray(b) for i, b in base.items()}; big[3][128 * 2 + 32:128 * 2 + 64] = Q.to_bytes(32, 'little')
    assert 'ptau: section 3 point 2 has a coordinate >= q or is not on the twist' in refused(write(tmp_path / 'bc.ptau', pl.assemble(big)), tmp_path)
    top = {i: bytearray(b) for i, b in base.items()}; top[5][64 * 3 + 40] ^= 2
    assert 'ptau: section 5 point 3 has' in refused(write(tmp_path / 't5.ptau', pl.assemble(top)), tmp_path)
    good = write(tmp_path / 'good.ptau', unprepared)
    assert 'cannot write' in refused(good, tmp_path, str(tmp_path / 'no_such_dir' / 'out.ptau'))
    assert 'cannot open' in refused(str(tmp_path / 'missing.ptau'), tmp_path)
    assert sorted(f for f in os.listdir(tmp_path) if 'never' in f or '.tmp' in f) == []
    # a bad monomial point under check_prepared: refused, not a verdict
    _, eb = pp.parse(expected)
    bad = {i: bytearray(b) for i, b in eb.items()}; bad[4][64 * 1 + 7] ^= 1
    with pytest.raises(_native.ZkcError) as ei:
        setup.check_prepared(write(tmp_path / 'bm.ptau', pl.assemble(bad)))
    assert ei.value.code == FMT and 'section 4 point 1 has a coordinate' in str(ei.value)
    with pytest.raises(_native.ZkcError) as ei:
        setup.check_prepared(good)
    assert ei.value.code == FMT and 'no section 12: run `powersoftau prepare phase2`' in str(ei.value)


def test_power_28_is_refused_before_anything_is_computed(tmp_path):
    """Fr has no 2^29-th root of unity, and section 12's last block at power 28 is a transform of that size: prepare and check_prepared refuse such a file by its header
    (a header doctored to say 28: the text comes before the section lengths are looked at), the key generator's reader still takes power 28 and only finds the lengths wrong"""
    unprepared, expected, secs = pp.images(2, pp.PLAIN)

    def power28(img):
        order, body = pp.parse(img)
        body = dict(body); body[1] = body[1][:36] + struct.pack('<II', 28, 28)
        return pl.assemble(body, order)
    text = "power 28 cannot be prepared or checked here: section 12's last block is a transform of size 2^29, and Fr has no root of unity of order above 2^28 (the largest power is 27)"
    assert text in refused(write(tmp_path / 'u28.ptau', power28(unprepared)), tmp_path)
    with pytest.raises(_native.ZkcError) as ei:
        setup.check_prepared(write(tmp_path / 'p28.ptau', power28(expected)))
    assert ei.value.code == FMT and text in str(ei.value)
    r = pl.write_r1cs(tmp_path / 'tiny.r1cs', 4, 1, [([(1, 1)], [(2, 1)], [(3, 1)])])
    with pytest.raises(_native.ZkcError) as ei:
        setup.from_ptau(r, str(tmp_path / 'p28.ptau'), tmp_path / 'never.zkey')
    assert 'the length of section 2 does not match power 28' in str(ei.value) and not (tmp_path / 'never.zkey').exists()
    # power 27 passes that gate (and then fails on the lengths, as any wrong power does)
    order, body = pp.parse(unprepared); body = dict(body); body[1] = body[1][:36] + struct.pack('<II', 27, 27)
    assert 'the length of section 2 does not match power 27' in refused(write(tmp_path / 'u27.ptau', pl.assemble(body, order)), tmp_path)


def test_open_unprepared_and_writer_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'ptau_prepare_asan')
    cmd = ['g++', '-std=c++17', '-O2', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'ptau_prepare_asan.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]
    work = tmp_path / 'files'; work.mkdir()
    unprepared, expected, _ = pp.images(3, pp.PLAIN)
    src = write(work / 'in.ptau', unprepared)
    _, exp = pp.parse(expected)
    for i in (12, 13, 14, 15):                                  # the bodies the program hands to the writer, so that its output can be compared here
        write(work / ('sec%d.bin' % i), exp[i])
    r = subprocess.run([exe, src, str(work)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'ptau prepare io: ok' in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert open(work / 'out.ptau', 'rb').read() == expected     # header, copied sections, block offsets: the writer alone reproduces the expected image
