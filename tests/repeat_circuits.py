"""TEST INFRASTRUCTURE: one crafted circuit whose wire rows hold the SAME point many times, for the keys-from-a-.ptau path (csrc/zkc_setup_ptau.hip over
csrc/zkc_point_ops.h).  A plain module beside ptau_lib.py: no fixtures; tests/test_ptau_setup_repeats_cpu.py and tests/test_gpu_ptau_setup_repeats.py import it.

The reader keeps a wire that is named twice in one linear combination as two terms (csrc/zkc_r1cs_parse.h) and Builder::add takes them one by one, so a row of a tiny
circuit can be P + P, P - P or 65 536 x P.  Domain 2^3 (seven constraints and the extra row of wire 0), a .ptau of power 3, no public wire.  No constraint names wire 0
and every C side names wires >= 1, so (1, 0, .., 0) is a witness.

Each case is one wire.  Its terms stand on the A side and on the B side alike, so the A, B1 and B2 rows of the wire have the shape written beside the case -- over
P = L_c(tau) G1 in the first two, over L_c(tau) G2 in B2 -- and the K row is that shape over beta P followed by the same over alpha P (and one C term for `pmp`).

What the comments on the cases rest on, all in make_plan (csrc/zkc_setup_ptau.hip):
  - the two loops that fill P.terms, `for (auto& u : B.unit)` before `for (j < nj)`: a row's +-1 terms come first, in the order they were added (by constraint, A side
    before B side), then its scaled terms in the order of the stable sort of B.gen by scalar; every scaled term is a scale job of its own, so equal (scalar, point) pairs
    are equal products at different indices;
  - `ns = (l + SEG - 1) / SEG` and `seg_start.push_back(at + s * SEG)`: a row of l terms is cut into segments of SEG = 32 consecutive terms, the last one shorter;
  - reduction_steps: every step sums RED = 32 consecutive partial sums of a row, and ALL rows of a group take as many steps as its longest row needs; a row that is down
    to 0 or 1 partial sums passes through the remaining steps by the `a == b` and `b - a == 1` exits of zkc_ptau_red.
The verdicts of the tests do not depend on that layout: they are exponents (ptau_lib.key_exponents, which sums over terms).  The purpose of the cases does."""
import ptau_lib as pl

R = pl.R
SEG, RED = 32, 32
FULL = 0x2a9e3c1f7b5d08e64c3a1f9d7e5b2c0a8f6e4d2b1a0918273645546372819aaf % R            # above (r - 1) / 2: Builder::add makes it -(r - FULL)
HALF = (R - 1) // 2
N_CONS, POWER = 7, 3
LONG = 5                                                                                    # the constraint of the longest rows: tau = root^LONG makes L_LONG = 1
RED3_CONS = (3, 4, 5, 6)                                                                    # the four constraints of red3_lo / _at / _hi, in increasing order


def _cycle(n):
    """n terms whose coefficients cycle 1, r - 1, 2, FULL, the i-th kind in constraint RED3_CONS[i]: [(constraint, coefficient, count)]"""
    return [(RED3_CONS[i], k, (n - i + 3) // 4) for i, k in enumerate((1, R - 1, 2, FULL))]


# name -> [(constraint, coefficient, how many times)], in the order the terms are written.  Wire = 1 + position in this table.
CASES = [
    # [P, P]: one segment; set, then the mixed addition refuses with equal y: G::dbl
    ('pp', [(0, 1, 2)]),
    # [P, -P]: one segment; set, then the mixed addition refuses with opposite y: back to infinity.  The row is infinity
    ('pm', [(1, 1, 1), (1, R - 1, 1)]),
    # [P, -P, P]: infinity as above, then set again: P.  C of constraint 3 names this wire, so K has one term more
    ('pmp', [(2, 1, 1), (2, R - 1, 1), (2, 1, 1)]),
    # [P x 5]: set, doubling, then three lean additions onto what the doubling left (2P + P, 3P + P, 4P + P)
    ('p5', [(3, 1, 5)]),
    # two scaled terms, two scale jobs (r - FULL, P) with the subtract bit: [-P', -P'] with P' = (r - FULL) P at two indices: set, doubling
    ('kk', [(0, FULL, 2)]),
    # FULL -> -(r - FULL), r - FULL stays: two jobs with one scalar, [-P', P'] (the stable sort keeps the order written): infinity
    ('k-k', [(1, FULL, 1), (1, R - FULL, 1)]),
    # (r - 1) / 2 stays (the longest chain), (r + 1) / 2 becomes -(r - 1) / 2; 3 stays, r - 3 becomes -3 (the shortest chain that is a job).  Sorted by scalar the row is
    # [3Q, -3Q, hP, -hP]: its sum is (r - 1) / 2 + (r + 1) / 2 + 3 - 3 = 0 mod r, so this row checks the signs but not the products: half_lo and half_hi do
    ('half', [(0, HALF, 1), (0, HALF + 1, 1), (1, 3, 1), (1, R - 3, 1)]),
    # the two sides of the sign rule in rows that do not cancel: [3Q, hP] and [-3Q, -hP]
    ('half_lo', [(2, HALF, 1), (6, 3, 1)]),
    ('half_hi', [(6, HALF + 1, 1), (2, R - 3, 1)]),
    # 32 units then 16 jobs (2, P): segments [P x 32] = 32P and [2P x 16] = 32P (both begin set, doubling).  One reduction job of two equal partial sums: the complete
    # addition's doubling.  K: [bP x 32], [aP x 32], [2bP x 16, 2aP x 16]; with alpha = beta 32P + 32P, then 64P + 64P
    ('red_eq', [(LONG, 1, 32), (LONG, 2, 16)]),
    # r - 2 becomes -2: segments 32P and -32P; the complete addition of opposite operands: infinity
    ('red_op', [(4, 1, 32), (4, R - 2, 16)]),
    # 64 segments of 32P.  Step 1: two jobs of 32 equal partial sums (32P + 32P, then 64P + 32P ..) leave 1024P each; step 2: 1024P + 1024P; step 3: the copy
    ('red_eq2', [(LONG, 1, 2048)]),
    # 2048 segments -> 64 -> 2 -> 1: equal operands at the third step, 32768P + 32768P.  K has 131 072 terms, 4096 -> 128 -> 4 -> 1
    ('red3_eq', [(LONG, 1, 65536)]),
    # 32 767 and 32 768 terms are 1024 segments, two steps by themselves; 32 769 are 1025, three.  Row: [P3 x 8192 or 8193, -P4 x 8192, 2 P5 x 8192, -(r - FULL) P6 x 8191
    # or 8192].  Up to 32 768 every segment holds one point 32 times (31 in the last of 32 767); at 32 769 the cuts move by one and three segments hold two points
    ('red3_lo', _cycle(SEG * RED * RED - 1)),
    ('red3_at', _cycle(SEG * RED * RED)),
    ('red3_hi', _cycle(SEG * RED * RED + 1)),
    # no term: no segment, `a == b` at every step.  All four points are infinity
    ('empty', []),
    # one term: one segment, `b - a == 1` at every step (K: two terms, one addition in the accumulation)
    ('single', [(2, FULL, 1)]),
]
WIRE = {name: 1 + i for i, (name, _) in enumerate(CASES)}
N_WIRES = 1 + len(CASES)
ZERO_ROWS = ('pm', 'k-k', 'half', 'red_op', 'empty')                                        # infinity in A, B1, B2 and K under every waste


def circuit():
    """(n_wires, n_pub, cons) for ptau_lib.write_r1cs and ptau_lib.key_exponents"""
    sides = [[] for _ in range(N_CONS)]
    for name, terms in CASES:
        for c, coef, count in terms:
            sides[c] += [(WIRE[name], coef)] * count
    return N_WIRES, 0, [(s, s, [(WIRE['pmp'], 1)] if c == 3 else []) for c, s in enumerate(sides)]


def write(path):
    n_wires, n_pub, cons = circuit()
    assert 1 << (POWER - 1) < len(cons) + n_pub + 1 <= 1 << POWER
    return pl.write_r1cs(path, n_wires, n_pub, cons)


def exponents(tau, alpha, beta):
    """(A, B, K) of every wire under the waste, integers mod r"""
    logn, A, B, K, _ = pl.key_exponents(*circuit(), tau, alpha, beta)
    assert logn == POWER
    return A, B, K


def key_points(sections, w):
    """the A, B1, B2 and K points of wire w in a key's sections (ptau_lib.zkey_sections); no public wire: wire 0's K point is the one point of section 3"""
    s = sections
    return s[5][64 * w:64 * w + 64], s[6][64 * w:64 * w + 64], s[7][128 * w:128 * w + 128], s[3][:64] if w == 0 else s[8][64 * (w - 1):64 * w]


def oracle_points(A, B, K, w):
    """the same four points from the exponents, through the CPU oracle"""
    return pl.g1_mont(A[w]), pl.g1_mont(B[w]), pl.g2_mont(B[w]), pl.g1_mont(K[w])
