"""CPU: the references of tests/test_gpu_pairing_dev.py held against each other before a kernel is held against them (tests/g2_py.py).
The closed form of a pairing product rests on the bilinearity of the host pairing zkc_pairing_bin (pinned to snarkjs' vk_alphabeta_12 by tests/test_host_abi_cpu.py):
e(a G1, b G2) = e([ab] G1, G2), and it tells neighbouring exponents apart.  Membership in G2 is its definition [r]Q = infinity in Python integers: true on multiples of
the generator, false on EVERY point the GPU tests list as a non-member -- forty points of the twist with distinct x, a point T of order 10069, Q + T, and the negatives
of these -- none taken on trust."""
import random
import oracle_lib as ol
import g2_py
from g2_py import R, Q, g2_add, g2_mul, g2_neg, g2_bytes, g2_point, in_g2, on_twist


def _gens():
    from zkcensus_amd import engines
    return engines.G1_GENERATOR, engines.G2_GENERATOR


def test_host_pairing_is_bilinear_in_both_arguments():
    G1, G2b = _gens(); G2 = g2_point(G2b)
    rng = random.Random(31)
    pairs = [(1, 1), (1, R - 1), (R - 1, 1), (R - 1, R - 1), (2, 3)] + [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(3)]
    for a, b in pairs:
        lhs = g2_py.pairing_bin(ol.g1_mul(G1, a), g2_bytes(g2_mul(G2, b)))
        assert lhs == g2_py.pairing_of_exponent(a * b), (a, b)
        assert lhs == g2_py.expected_product([R - 1], [a], [b])                       # the closed form itself: weight -1 undoes its sign
        nxt = g2_py.pairing_bin(ol.g1_mul(G1, a + 1), g2_bytes(g2_mul(G2, b))) if a + 1 < R else g2_py.UNIT12       # (a + 1) G1 = infinity pairs to 1
        assert lhs != nxt and lhs != g2_py.UNIT12, (a, b)
    # e(P, Q) e(-P, Q) = 1 has no pairing to compute: s = 0 is the unit element, written directly
    assert g2_py.expected_product([1, 1], [5, R - 5], [7, 7]) == g2_py.UNIT12
    assert g2_py.expected_product([R], [5], [7]) == g2_py.UNIT12 and g2_py.expected_product([3], [0], [7]) == g2_py.UNIT12


def test_membership_reference_on_members():
    _, G2b = _gens(); G2 = g2_point(G2b)
    rng = random.Random(32)
    for b in (1, 2, R - 1, rng.randrange(1, R), rng.randrange(1, R)):
        p = g2_mul(G2, b)
        assert on_twist(p) and in_g2(p) and in_g2(g2_neg(p)), b
    assert in_g2(None)


def test_membership_reference_on_every_listed_non_member():
    _, G2b = _gens(); G2 = g2_point(G2b)
    pts = g2_py.outside_points(40)
    assert len({p[0][0] for p in pts}) == 40 and all(p[0][1] == 1 for p in pts)
    assert pts[0] == ol.twist_point_outside_g2()                                       # the one point the verifier tests have used so far is the first of them
    T = g2_py.small_order_point()
    assert T is not None and g2_mul(T, g2_py.SMALL_ORDER) is None and g2_py.TWIST_H % g2_py.SMALL_ORDER == 0
    assert all(g2_py.SMALL_ORDER % d for d in range(2, 101))                           # 10069 is prime: T has exactly that order
    rng = random.Random(33)
    shifted = [g2_add(g2_mul(G2, b), T) for b in (1, R - 1, rng.randrange(1, R))]
    listed = pts + [T] + shifted
    listed += [g2_neg(p) for p in listed]
    assert len(listed) == 88
    for p in listed:
        assert on_twist(p) and not in_g2(p)
