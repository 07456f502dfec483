"""TEST INFRASTRUCTURE for the check that a powers-of-tau file holds the powers of one tau (include/zkcensus_ptau_verify.h), shared by tests/test_ptau_verify_cpu.py and
tests/test_gpu_ptau_verify.py: honest section bodies to change, one change per check with what it must be answered with, the file of arbitrary points that the other
checks accept, weights chosen by a test, and the eight sums such weights give, from Python integers and the oracle -- never from the sums under test."""
import random
import oracle_lib as ol
import g2_py
import edge_points as ep
import ptau_lib as pl
import ptau_prep_lib as pp

R, Q = ol.R, ol.Q
POINT, G2_SUBGROUP, GENERATORS, TAU_G1_G2, TAU_G1, TAU_G2, ALPHA_TAU_G1, BETA_TAU_G1, BETA_G1_G2 = range(1, 10)      # ZKC_PTAU_CHECK_*
WASTE_NAMES = ['plain', 'one', 'minus-one', 'on-domain', 'on-double-domain']
TAU, ALPHA, BETA = pp.PLAIN


def monomial(power, waste=pp.PLAIN, ctx=None):
    """the bodies of sections 1 .. 7 of an honest file, for a test to change"""
    return {i: bytearray(b) for i, b in pp.images(power, waste, ctx)[2].items() if i < 8}


def hole_sections(power, ctx=None):
    """section 2 = k_i G with k_0 = 1, k_1 = tau (so that the first thing wrong is the chain of section 2 itself) and the rest arbitrary; sections 3 .. 6 honest"""
    N = 1 << power; rng = random.Random(40 + power)
    secs = monomial(power, pp.PLAIN, ctx)
    secs[2] = bytearray(pp.points([1, TAU] + [rng.randrange(1, R) for _ in range(2 * N - 3)], 64, ctx))
    assert len(secs[2]) == 64 * (2 * N - 1)
    return secs


TINY_CIRCUIT = (4, 0, [([(1, 1)], [(2, 1)], [(3, 1)]), ([(3, 2)], [(1, 5)], [(2, R - 1)])])      # 2 constraints + 1: a domain of 4


# ---- one changed file per check ----
def set_pt(secs, sec, i, pt):
    w = pl.PT_BYTES[sec]
    assert len(pt) == w
    secs[sec][w * i:w * i + w] = pt


def get_pt(secs, sec, i):
    w = pl.PT_BYTES[sec]
    return bytes(secs[sec][w * i:w * i + w])


def g2_from_mont(b):
    c = [int.from_bytes(b[32 * i:32 * i + 32], 'little') * ep.MONT_INV % Q for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def with_cofactor_part(secs):
    """U_2 + T, T of order 10069 on the twist: on the twist, outside G2"""
    p = g2_py.g2_add(g2_from_mont(get_pt(secs, 3, 2)), g2_py.small_order_point())
    assert g2_py.on_twist(p)
    set_pt(secs, 3, 2, ep.g2_mont(p))


def swap_3_4(secs):
    a, b = get_pt(secs, 2, 3), get_pt(secs, 2, 4)
    set_pt(secs, 2, 3, b); set_pt(secs, 2, 4, a)


def off_curve(secs):
    secs[2][64 * 6 + 3] ^= 1; secs[2][64 * 4 + 40] ^= 1        # two bad points: the smaller index is named


def coordinate_q(secs):
    secs[4][64 * 2 + 32:64 * 2 + 64] = Q.to_bytes(32, 'little')


def twist_coordinate_q(secs):
    secs[3][128 * 1 + 96:128 * 1 + 128] = Q.to_bytes(32, 'little')


def mutations(power):
    """name -> (change of the section bodies, check, section or None, index or None)"""
    N = 1 << power; K = 0x1d2c3b4a5968778695a4b3c2d1e0f
    other = 0x3f2e1d0c9b8a79685746352413021100ffeeddccbbaa % R
    g1, g2 = (lambda k: pl.g1_mont(k % R)), (lambda k: pl.g2_mont(k % R))
    return {
        't5-plus-one': (lambda s: set_pt(s, 2, 5, g1(pow(TAU, 5, R) + 1)), TAU_G1, 2, None),
        't3-t4-swapped': (swap_3_4, TAU_G1, 2, None),
        'last-t': (lambda s: set_pt(s, 2, 2 * N - 2, g1(pow(TAU, 2 * N - 2, R) + 1)), TAU_G1, 2, None),                  # the boundary term: only R2 holds it
        'section-2-scaled': (lambda s: s.__setitem__(2, bytearray(pp.points([K * pow(TAU, i, R) % R for i in range(2 * N - 1)], 64))), GENERATORS, 2, 0),
        'section-3-other-tau': (lambda s: s.__setitem__(3, bytearray(pp.points([pow(other, i, R) for i in range(N)], 128))), TAU_G1_G2, None, None),
        'u2': (lambda s: set_pt(s, 3, 2, g2(pow(TAU, 2, R) + 1)), TAU_G2, 3, None),
        'a0-alone': (lambda s: set_pt(s, 4, 0, g1(ALPHA + 1)), ALPHA_TAU_G1, 4, None),
        'b3': (lambda s: set_pt(s, 5, 3, g1(BETA * pow(TAU, 3, R) + 1)), BETA_TAU_G1, 5, None),
        'beta2': (lambda s: set_pt(s, 6, 0, g2(BETA + 1)), BETA_G1_G2, 6, 0),
        'off-curve': (off_curve, POINT, 2, 4),
        'coordinate-q': (coordinate_q, POINT, 4, 2),
        'twist-coordinate-q': (twist_coordinate_q, POINT, 3, 1),
        'beta2-off-twist': (lambda s: s[6].__setitem__(5, s[6][5] ^ 1), POINT, 6, 0),
        'u2-cofactor-part': (with_cofactor_part, G2_SUBGROUP, 3, 2),
        'beta2-cofactor-part': (lambda s: set_pt(s, 6, 0, ep.g2_mont(g2_py.g2_add(g2_from_mont(get_pt(s, 6, 0)), g2_py.small_order_point()))), G2_SUBGROUP, 6, 0),
        'infinity-at-t1': (lambda s: set_pt(s, 2, 1, bytes(64)), POINT, 2, 1),
        'infinity-at-last-b': (lambda s: set_pt(s, 5, N - 1, bytes(64)), POINT, 5, N - 1),
        # two things wrong: the earlier check in the order of the header is reported, whatever the order of the sections
        'u2-cofactor-part-and-bad-b': (lambda s: (with_cofactor_part(s), s[5].__setitem__(64 * 1 + 9, s[5][64 * 1 + 9] ^ 1)), POINT, 5, 1),
        'u2-cofactor-part-and-t5': (lambda s: (with_cofactor_part(s), set_pt(s, 2, 5, g1(77))), G2_SUBGROUP, 3, 2),
    }



# the changes whose points exist at power 1 (section 2: three points, the others two)
POWER_1_MUTATIONS = ['last-t', 'section-2-scaled', 'section-3-other-tau', 'a0-alone', 'beta2', 'beta2-off-twist', 'beta2-cofactor-part', 'infinity-at-t1', 'infinity-at-last-b']


# ---- the sums by value ----
def expected_sums(power, waste, ws):
    """R1 R2 | S1 S2 | A pair | B pair in standard form from Python integers: (sum r_i tau^i) G and tau times it"""
    tau, alpha, beta = waste; N = 1 << power
    s = lambda n: sum(w * pow(tau, i, R) for i, w in enumerate(ws[:n])) % R
    g1 = lambda k: ol.g1_mul(pl.G1_GEN, k % R) if k % R else bytes(64)
    g2 = lambda k: ol.msm_g2(pl.G2_GEN, ol.le32(k % R)) if k % R else bytes(128)
    t, u = s(2 * N - 2), s(N - 1)
    return g1(t) + g1(tau * t) + g2(u) + g2(tau * u) + g1(alpha * u) + g1(alpha * tau * u) + g1(beta * u) + g1(beta * tau * u)


def weight_sets(power):
    n = (2 << power) - 2; rng = random.Random(50 + power)
    edge = [0, 1, (1 << 128) - 1, 1 << 127, 2, (1 << 64) - 1, 1 << 64]
    return {'random': [rng.getrandbits(128) for _ in range(n)], 'edges': [edge[i % len(edge)] for i in range(n)], 'all-max': [(1 << 128) - 1] * n,
            'one-term': [0] * (n - 1) + [0x1234567], 'ones': [1] * n}


def w16(ws):
    return b''.join(w.to_bytes(16, 'little') for w in ws)
