"""CPU: is a powers-of-tau file the powers of one tau?  (include/zkcensus_ptau_verify.h) on host threads (ctx = None), at powers 2 and 3.  Files come from tests/ptau_lib.py
and tests/ptau_prep_lib.py: Python integers and the oracle's scalar multiplications.  First the hole this check closes -- a file whose section 2 is (G, tau G, any points
..), prepared from that, is accepted by check_prepared and by from_ptau --, then every waste of ptau_prep_lib.wastes as a valid file, one changed file per check with the
check's id and the point it names, and the eight sums by value through the hook: (sum r_i tau^i) G from Python integers and the oracle, at chunk sizes that do not divide
the 14 terms of section 2."""
import os, random
import pytest
import oracle_lib as ol
import g2_py
import edge_points as ep
import ptau_lib as pl
import ptau_prep_lib as pp
import ptau_verify_lib as pv
from ptau_verify_lib import (POINT, G2_SUBGROUP, GENERATORS, TAU_G1_G2, TAU_G1, TAU_G2, ALPHA_TAU_G1, BETA_TAU_G1, BETA_G1_G2, WASTE_NAMES, TAU, ALPHA, BETA, monomial, mutations,
                             expected_sums, weight_sets, w16, get_pt, g2_from_mont, with_cofactor_part, off_curve)
from zkcensus_amd import _native, setup

ROOT, R, Q = ol.ROOT, ol.R, ol.Q
SEED = bytes(range(7, 39))
NEW_ENTRY_POINTS = sorted(['zkc_g1_wsum_pair_dev', 'zkc_g2_wsum_pair_dev', 'zkc_ptau_verify', 'zkc_ptau_verify_stats', 'zkc_debug_ptau_verify'])


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_ptau_verify.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert '#include "zkcensus_ptau_verify.h"' in open(os.path.join(ROOT, 'include', 'zkcensus.h')).read()
    hdr = open(os.path.join(ROOT, 'include', 'zkcensus_ptau_verify.h')).read()
    for i, name in enumerate(setup.PTAU_CHECKS):
        if i:
            assert 'ZKC_PTAU_CHECK_%s = %d' % (name, i) in hdr


def write(path, img):
    open(path, 'wb').write(img)
    return str(path)


# ---- the hole ----
@pytest.mark.parametrize('power', [2, 3])
def test_a_file_of_arbitrary_points_passes_the_other_checks_and_fails_this_one(tmp_path, power):
    """ptau_verify_lib.hole_sections: section 2 = (G, tau G, arbitrary points ..), sections 3 .. 6 honest"""
    secs = pv.hole_sections(power)
    src = write(tmp_path / 'hole_u.ptau', pl.assemble(secs)); hole = str(tmp_path / 'hole.ptau')
    setup.prepare_ptau(src, hole)
    assert setup.check_prepared(hole) == (True, 0, 0, '')
    r = pl.write_r1cs(tmp_path / 'tiny.r1cs', *pv.TINY_CIRCUIT)
    setup.from_ptau(r, hole, tmp_path / 'hole.zkey', tmp_path / 'hole.json')                                                   # the hole: accepted, a key is written
    assert os.path.getsize(tmp_path / 'hole.zkey') > 0
    for path in (src, hole):                                    # unprepared and prepared alike
        ok, check, section, index, why = setup.verify_ptau(path, seed=SEED)
        assert (ok, check, section) == (False, TAU_G1, 2) and why == 'ptau: section 2 is not the powers of one tau: sameRatio(R1, R2; G2, tauG2[1]) fails'
    with pytest.raises(_native.ZkcError) as ei:
        setup.from_ptau(r, hole, tmp_path / 'never.zkey', tmp_path / 'never.json', verify=True)
    assert ei.value.code == 5 and 'section 2 is not the powers of one tau' in str(ei.value)
    assert not (tmp_path / 'never.zkey').exists() and not (tmp_path / 'never.json').exists()


def test_from_ptau_with_verify_writes_the_same_key(tmp_path):
    power = 3
    src = write(tmp_path / 'u.ptau', pp.images(power, pp.PLAIN)[0]); good = setup.prepare_ptau(src, str(tmp_path / 'p.ptau'))
    r = pl.write_r1cs(tmp_path / 'tiny.r1cs', *pv.TINY_CIRCUIT)
    setup.from_ptau(r, good, tmp_path / 'a.zkey', tmp_path / 'a.json')
    setup.from_ptau(r, good, tmp_path / 'b.zkey', tmp_path / 'b.json', verify=True)
    assert open(tmp_path / 'a.zkey', 'rb').read() == open(tmp_path / 'b.zkey', 'rb').read()
    assert open(tmp_path / 'a.json', 'rb').read() == open(tmp_path / 'b.json', 'rb').read()
    # ptau_lib's own prepared file holds the true top block of section 12, which no preparer can write: verify_ptau takes it (sections 2 .. 6 are right), check_prepared
    # does not, and from_ptau(verify=True) gives that reason
    theirs = write(tmp_path / 'lib.ptau', pl.assemble(pp.images(power, pp.PLAIN)[2]))
    assert setup.verify_ptau(theirs, seed=SEED)[0]
    with pytest.raises(_native.ZkcError) as ei:
        setup.from_ptau(r, theirs, tmp_path / 'never.zkey', verify=True)
    assert ei.value.code == 5 and 'is not the transform of section 2' in str(ei.value) and not (tmp_path / 'never.zkey').exists()


# ---- valid files ----
@pytest.mark.parametrize('waste', WASTE_NAMES)
@pytest.mark.parametrize('power', [2, 3])
def test_every_waste_is_a_valid_file(tmp_path, power, waste):
    """tau = 1, tau = r - 1 and tau on the domain make the sums meet equal points, opposite points and (partial sums at) infinity"""
    unprepared, expected, _ = pp.images(power, pp.wastes(power)[waste])
    for img in (unprepared, expected):
        path = write(tmp_path / 'f.ptau', img)
        assert setup.verify_ptau(path, seed=SEED) == (True, 0, 0, 0, '')
        assert setup.verify_ptau(path) == (True, 0, 0, 0, '')               # weights from the OS
    ms = setup.ptau_verify_stats()
    assert list(ms) == ['read', 'upload_check', 'g2_membership', 'sums_g1', 'sums_g2', 'pairings'] and all(v > 0 for v in ms.values()), ms


# ---- one changed file per check (ptau_verify_lib.mutations) ----
MUTATION_NAMES = sorted(mutations(2))


@pytest.mark.parametrize('name', MUTATION_NAMES)
@pytest.mark.parametrize('power', [2, 3])
def test_each_check_fires_on_a_file_changed_to_provoke_it(tmp_path, power, name):
    change, check, section, index = mutations(power)[name]
    secs = monomial(power)
    change(secs)
    ok, c, s, i, why = setup.verify_ptau(write(tmp_path / 'm.ptau', pl.assemble(secs)), seed=SEED)
    assert (ok, c) == (False, check), (setup.PTAU_CHECKS[c], why)
    assert why.startswith('ptau: ')
    if section is not None:
        assert s == section
    if index is not None:
        assert i == index
        assert check == BETA_G1_G2 or 'section %d point %d ' % (section, index) in why


def test_the_ratio_checks_alone_would_pass_a_cofactor_part():
    """The model of what a pairing sees: only the order-r component of a twist point.  c = 1 mod r, c = 0 mod 10069 projects U_2 + T back onto U_2, so S1, S2 of the changed
    section -- summed in Python with the cofactor part in them -- are, to the pairing, the honest sums, which are in the ratio tau: nothing but the membership check
    stands between this file and a key whose B2 points the verifiers refuse."""
    power = 3; N = 1 << power
    secs = monomial(power)
    honest = [g2_from_mont(get_pt(secs, 3, i)) for i in range(N)]
    with_cofactor_part(secs)
    changed = [g2_from_mont(get_pt(secs, 3, i)) for i in range(N)]
    assert changed[2] != honest[2] and not g2_py.in_g2(changed[2]) and all(g2_py.in_g2(p) for p in honest)
    rng = random.Random(3); ws = [rng.getrandbits(128) for _ in range(N - 1)]
    c = g2_py.SMALL_ORDER * pow(g2_py.SMALL_ORDER, -1, R)
    seen = lambda p: g2_py.g2_mul(p, c)
    s1, s2 = ep.g2_msm(changed[:-1], ws), ep.g2_msm(changed[1:], ws)
    assert s1 != ep.g2_msm(honest[:-1], ws)                                                 # the sums do carry the cofactor part ...
    assert seen(s1) == ep.g2_msm(honest[:-1], ws) and seen(s2) == ep.g2_msm(honest[1:], ws)  # ... which the pairing does not see
    assert seen(s2) == g2_py.g2_mul(seen(s1), TAU)


def test_refusals_that_are_not_verdicts(tmp_path):
    power = 2
    secs = monomial(power)
    no3 = {i: b for i, b in secs.items() if i != 3}
    for img, text in ((pl.assemble(no3), 'ptau: no section 3'), (b'nope' + bytes(40), 'bad magic'), (pl.assemble(secs)[:-10], 'runs past the file')):
        with pytest.raises(_native.ZkcError) as ei:
            setup.verify_ptau(write(tmp_path / 'r.ptau', img), seed=SEED)
        assert ei.value.code == 5 and text in str(ei.value)
    with pytest.raises(_native.ZkcError) as ei:
        setup.verify_ptau(str(tmp_path / 'missing.ptau'))
    assert ei.value.code == 5 and 'cannot open' in str(ei.value)
    good = write(tmp_path / 'g.ptau', pl.assemble(secs))
    with pytest.raises(_native.ZkcError) as ei:                 # the hook wants exactly 2N - 2 weights
        setup.debug_verify_ptau(good, bytes(16 * 5))
    assert ei.value.code == 4 and 'takes 6 weights' in str(ei.value)
    err = __import__('ctypes').create_string_buffer(256)
    assert _native.load().zkc_debug_ptau_verify(None, os.fsencode(good), None, 6, 0, None, None, None, None, err, 256) == -4
    assert _native.load().zkc_ptau_verify(None, None, None, None, None, None, err, 256) == -4
    assert _native.load().zkc_ptau_verify(None, os.fsencode(good), SEED, None, None, None, None, 0) == 1      # every output may be absent


# ---- the sums by value (ptau_verify_lib.expected_sums) ----
@pytest.mark.parametrize('chunk', [0, 1, 2, 3, 5])
def test_the_eight_sums_by_value(tmp_path, chunk):
    """power 3: 14 terms in section 2 and 7 in the others, so none of the chunk sizes divides them and chunks of one term, chunks that end one term short and the default
    (one chunk) all occur"""
    power = 3
    path = write(tmp_path / 'f.ptau', pp.images(power, pp.PLAIN)[0])
    for name, ws in weight_sets(power).items():
        verdict, sums = setup.debug_verify_ptau(path, w16(ws), chunk_terms=chunk)
        exp = expected_sums(power, pp.PLAIN, ws)
        assert [k for k in range(0, 640, 64) if sums[k:k + 64] != exp[k:k + 64]] == [], name
        # 'one-term' weighs only T_13 and T_14: the sums over the seven terms of sections 3 .. 5 are infinity, and a sum at infinity fails its check
        assert verdict[:3] == ((False, TAU_G2, 3) if name == 'one-term' else (True, 0, 0)), (name, verdict)


@pytest.mark.parametrize('chunk', [0, 3])
def test_sums_at_infinity_fail_their_check(tmp_path, chunk):
    power = 3; n = (2 << power) - 2
    path = write(tmp_path / 'f.ptau', pp.images(power, pp.PLAIN)[0])
    verdict, sums = setup.debug_verify_ptau(path, bytes(16 * n), chunk_terms=chunk)       # all-zero weights
    assert verdict[:3] == (False, TAU_G1, 2) and sums == bytes(640)
    # tau = r - 1 with weights (1, 1, ..): section 2 is G, -G, G, .. and its 14 terms cancel in pairs -- R1 and R2 are infinity -- while the 7 terms of the other sections
    # leave one point
    minus = pp.wastes(power)['minus-one']
    path = write(tmp_path / 'm.ptau', pp.images(power, minus)[0])
    verdict, sums = setup.debug_verify_ptau(path, w16([1] * n), chunk_terms=chunk)
    exp = expected_sums(power, minus, [1] * n)
    assert sums == exp and sums[:128] == bytes(128) and sums[128:256] == pl.G2_GEN and any(sums[384:448])
    assert verdict[:3] == (False, TAU_G1, 2)
    # and with weights that do not cancel the same file is valid
    ws = weight_sets(power)['random']
    verdict, sums = setup.debug_verify_ptau(path, w16(ws), chunk_terms=chunk)
    assert verdict[0] and sums == expected_sums(power, minus, ws)


def test_a_failed_point_check_leaves_no_sums(tmp_path):
    power = 2
    secs = monomial(power); off_curve(secs)
    verdict, sums = setup.debug_verify_ptau(write(tmp_path / 'b.ptau', pl.assemble(secs)), w16(weight_sets(power)['random']))
    assert verdict[:4] == (False, POINT, 2, 4) and sums == bytes(640)
