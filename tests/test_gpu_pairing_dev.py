"""GPU: the device side of the batch verifiers (csrc/zkc_pairing_dev.hip, fed by zkc_fold_mul / zkc_fold_gsum of csrc/zkc_msm.hip) BY VALUE, through the test hook
zkc_debug_pairing_dev, which drives what zkc_verify_batch / zkc_verify_batch_each drive.  No key, no prover: P_i = a_i G1, Q_i = b_i G2 and weights w_i, so that

    prod_i e(-w_i P_i, Q_i) = e([s]G1, G2),   s = -(sum_i w_i a_i b_i) mod r

is one G1 product of the oracle and one host pairing (tests/g2_py.py expected_product; s = 0 is the unit element), and every comparison is byte equality: the product of a
batch, every node of every kept level of its product tree over that node's own range, the folded points w_i P_i against the oracle, and the membership flags against
[r]Q = infinity in Python integers.  tests/test_pairing_refs_cpu.py holds these references against each other first.

One list of 131 members serves every size: the edge members sit at its END and a batch of N takes the last N, so they move over lanes 0 / 63 / 64 / N - 1."""
import contextlib
import json
import os
import random
import sys
import pytest
import oracle_lib as ol
import g2_py
from g2_py import R, Q, g2_add, g2_mul, g2_mul_many, g2_neg, g2_bytes, g2_point, in_g2, on_twist, expected_product, UNIT12

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
BAD_ARG = 4                                                         # ZKC_ERR_BAD_ARG
L = 131


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.fixture(scope='module')
def gpu():
    import zkcensus_amd
    from zkcensus_amd import groth16
    ctx = zkcensus_amd.Context(0)
    yield ctx, groth16
    ctx.close()


def neg(m):
    """the opposite pair: (-P, Q) under the same weight"""
    return ((R - m[0]) % R, m[1], m[2])


class Points:
    """a G1 = bytes, b G2 = bytes, each made once (0: the point at infinity)"""

    def __init__(self):
        from zkcensus_amd import engines
        self.G1, self.G2 = engines.G1_GENERATOR, g2_point(engines.G2_GENERATOR)
        self._g1, self._g2 = {0: bytes(64)}, {0: None}

    def g1(self, a):
        if a not in self._g1:
            self._g1[a] = ol.g1_mul(self.G1, a)
        return self._g1[a]

    def g2_many(self, bs):
        new = sorted({b for b in bs if b not in self._g2})
        if new:
            self._g2.update(zip(new, g2_mul_many(self.G2, new)))

    def g2(self, b):
        if b not in self._g2:
            self._g2[b] = g2_neg(self._g2[R - b]) if (R - b) in self._g2 else g2_mul(self.G2, b)
        return g2_bytes(self._g2[b])


@pytest.fixture(scope='module')
def master():
    """(members, points): 131 members (a, b, w), the edge members last"""
    rng = random.Random(2024)
    ra = lambda: rng.randrange(1, R)
    rw = lambda: rng.randrange(1, 1 << 128)                        # the production width
    x64, x1, x2, twin = (ra(), ra(), rw()), (ra(), ra(), rw()), (ra(), ra(), rw()), (ra(), ra(), rw())
    edge = [(ra(), ra(), 0), (ra(), ra(), 1), (ra(), ra(), (1 << 128) - 1), (ra(), ra(), 1 << 128), (ra(), ra(), R - 1), (ra(), ra(), (1 << 256) - 1),
            (ra(), 1, rw()), (ra(), R - 1, rw()),                  # Q = G2 itself, Q = -G2
            twin, twin,                                            # two identical pairs
            (0, 0, rw()),                                          # both at infinity
            neg(x64),                                              # its partner sits 64 places before it: they meet high in the tree
            x1, neg(x1), (ra(), ra(), rng.getrandbits(256)), x2, neg(x2),      # a pair and its opposite, adjacent, at both parities: one of the two meets in zkc_line_pairs
            (0, ra(), rw()),                                       # P at infinity, Q finite
            (ra(), 0, rw()),                                       # Q at infinity, P finite
            (ra(), ra(), R),                                       # weight r: folds to infinity through the kernel's own P + (-P)
            (ra(), ra(), rng.getrandbits(256) | (1 << 255))]       # a full-width weight, last: the batch of one
    members = [(ra(), ra(), rng.getrandbits(256) if i % 5 == 4 else rw()) for i in range(L - len(edge))] + edge
    at64 = L - len(edge) + edge.index(neg(x64))
    members[at64 - 64] = x64
    assert len(members) == L and members[at64] == neg(members[at64 - 64]) and at64 - 64 >= 0
    pts = Points()
    pts.g2_many([b for _, b, _ in members])
    return members, pts


def run(gpu, pts, members, weights=True, nodes=None, want_flags=False):
    ctx, groth16 = gpu
    g1 = b''.join(pts.g1(a) for a, _, _ in members); g2 = b''.join(pts.g2(b) for _, b, _ in members)
    w = b''.join(m[2].to_bytes(32, 'little') for m in members) if weights else None
    return groth16.debug_pairing_dev(ctx, g1, g2, w, folded=True, members=want_flags, nodes=nodes)


def closed_form(members, weights=True):
    return expected_product([m[2] if weights else 1 for m in members], [m[0] for m in members], [m[1] for m in members])


def folded_expected(pts, members, weights=True):
    """w_i P_i by the oracle, the weight reduced here; infinity is 64 zero bytes"""
    out = []
    for a, _, w in members:
        k = (w if weights else 1) % R
        out.append(bytes(64) if a == 0 or k == 0 else ol.g1_mul(pts.g1(a), k))
    return out


def check_batch(gpu, pts, members, weights=True):
    prod, bad, folded, _, _ = run(gpu, pts, members, weights)
    exp_f = folded_expected(pts, members, weights)
    for i in range(len(members)):
        assert folded[64 * i:64 * i + 64] == exp_f[i], ('folded', i, hex(members[i][2]))
    assert bad == 0
    assert prod == closed_form(members, weights), ('product', len(members))
    return prod


# ---- the product by value, and the folded points of the same batches ----
@pytest.mark.parametrize('N,chunk', [(1, None), (2, None), (3, None), (5, None), (64, None), (65, None), (129, None), (131, '2'), (100, '33'), (65, '64')])
def test_product_equals_closed_form(gpu, master, N, chunk):
    """At the default round size and with several rounds of pairs: odd levels at several depths, the lone dense line in the odd slot, a last round of one pair"""
    members, pts = master
    with env(ZKC_VERIFY_CHUNK=chunk):
        prod = check_batch(gpu, pts, members[-N:])
    assert prod != UNIT12


def test_weight_r_folds_to_infinity(gpu, master):
    members, pts = master
    i = next(k for k, m in enumerate(members) if m[2] == R)
    for N in (L - i, 65):
        _, _, folded, _, _ = run(gpu, pts, members[-N:])
        k = i - (L - N)
        a, _, w = members[-N:][k]
        assert w == R and a != 0 and folded[64 * k:64 * k + 64] == bytes(64)


def test_null_weights_are_all_ones(gpu, master):
    members, pts = master
    for N in (3, 65):
        ones = [(a, b, 1) for a, b, _ in members[-N:]]
        assert check_batch(gpu, pts, ones, weights=False) == check_batch(gpu, pts, ones, weights=True) != UNIT12


def test_batches_whose_product_is_one(gpu, master):
    """A batch that cancels completely -- opposite pairs adjacent (met in zkc_line_pairs) and 64 apart (met high in the tree), and
    (P, Q) with (P, -Q) -- and a batch with every member at infinity: the unit element, byte for byte"""
    members, pts = master
    plain = [m for m in members[:40] if m[2] % R and m[0] and m[1]]
    x, y, z = plain[0], plain[1], plain[2]
    batch = [None] * 66
    batch[0], batch[64] = x, neg(x)                                 # 64 apart, from lane 0 ...
    batch[1], batch[65] = y, neg(y)                                 # ... and from an odd lane
    for k in range(2, 64, 2):                                       # adjacent, in both orders
        m = plain[3 + (k // 2) % (len(plain) - 3)]
        batch[k], batch[k + 1] = (m, neg(m)) if k % 4 else (neg(m), m)
    batch += [z, (z[0], R - z[1], z[2])]                            # (P, Q) (P, -Q)
    assert len(batch) == 68 and closed_form(batch) == UNIT12
    assert check_batch(gpu, pts, batch) == UNIT12
    with env(ZKC_VERIFY_CHUNK='5'):
        assert check_batch(gpu, pts, batch) == UNIT12
    inf = [(0, x[1], x[2]), (x[0], 0, x[2]), (0, 0, x[2]), (0, y[1], y[2]), (y[0], 0, 0)]
    assert check_batch(gpu, pts, inf) == UNIT12
    assert check_batch(gpu, pts, inf[:1]) == UNIT12 and check_batch(gpu, pts, inf[1:2]) == UNIT12


def test_exchanging_two_q_changes_the_product(gpu, master):
    """Control: the closed form is no constant of the batch's multiset of points"""
    members, pts = master
    batch = [(a, b, 1) for a, b, _ in members[:5]]
    (a0, b0, _), (a1, b1, _) = batch[0], batch[1]
    assert (a0 * b1 + a1 * b0 - a0 * b0 - a1 * b1) % R != 0
    swapped = [(a0, b1, 1), (a1, b0, 1)] + batch[2:]
    before, after = check_batch(gpu, pts, batch, weights=False), check_batch(gpu, pts, swapped, weights=False)
    assert before != after


# ---- every node of every kept level ----
def tree_nodes(N, chunk):
    """TreeShape's rule: (round, level, t) -> the pairs [lo, hi) of the batch under that node"""
    out = {}
    chunk = chunk or N
    for c in range((N + chunk - 1) // chunk):
        base = c * chunk; n = min(chunk, N - base)
        m, k = (n + 1) // 2, 0
        while True:
            for t in range(m):
                out[(c, k, t)] = (base + min(n, t << (k + 1)), base + min(n, (t + 1) << (k + 1)))
            if m <= 1: break
            m, k = (m + 1) // 2, k + 1
    return out


@pytest.mark.parametrize('N,chunk', [(5, None), (13, None), (131, '32')])
def test_every_tree_node_equals_the_closed_form_of_its_range(gpu, master, N, chunk):
    members, pts = master
    batch = members[-N:]
    nodes = tree_nodes(N, int(chunk) if chunk else None)
    order = sorted(nodes)
    with env(ZKC_VERIFY_CHUNK=chunk):
        prod, bad, _, _, got = run(gpu, pts, batch, nodes=order)
    assert bad == 0 and prod == closed_form(batch)
    lone = 0
    for node, value in zip(order, got):
        lo, hi = nodes[node]
        assert hi > lo
        assert value == closed_form(batch[lo:hi]), (node, lo, hi)
        lone += hi - lo == 1
    assert lone >= 1                                                # a lone member handed up unchanged is among them
    if not chunk:
        top = max(order)
        assert nodes[top] == (0, N) and got[order.index(top)] == prod
    else:                                                           # (131, 32): rounds of 32, 32, 32, 32 and 3 pairs
        assert len({c for c, _, _ in order}) == 5 and nodes[(4, 1, 0)] == (128, 131) and nodes[(4, 0, 1)] == (130, 131)
    # the nodes in another order, a subset of them: the same values
    some = order[::-3]
    with env(ZKC_VERIFY_CHUNK=chunk):
        _, _, _, _, again = run(gpu, pts, batch, nodes=some)
    assert again == [got[order.index(x)] for x in some]


# ---- membership, flag by flag ----
@pytest.fixture(scope='module')
def g2_pool():
    """(members, non-members) of the twist as point tuples (None = infinity); every one classified by [r]Q = infinity here, none on trust"""
    from zkcensus_amd import engines
    G2 = g2_point(engines.G2_GENERATOR)
    rng = random.Random(77)
    bs = [1, 2, R - 1, R - 2, (1 << 128) - 1, 1 << 128, (1 << 253)] + [rng.randrange(1, R) for _ in range(9)]
    inside = g2_mul_many(G2, bs)
    T = g2_py.small_order_point()
    outside = g2_py.outside_points(40)
    outside += [T, g2_add(T, T)] + [g2_add(q, T) for q in inside[:6]] + [g2_add(outside[0], inside[3])]
    outside += [g2_neg(p) for p in outside]                         # (x, -y)
    assert all(on_twist(p) for p in inside + outside)
    assert all(in_g2(p) for p in inside) and not any(in_g2(p) for p in outside)
    assert len(inside) + 1 + len(outside) >= 64
    return inside + [None], outside


def membership_batch(pool, N, bad_lanes):
    inside, outside = pool
    batch = [inside[(5 * i + N) % len(inside)] for i in range(N)]
    for j, lane in enumerate(sorted(bad_lanes)):
        batch[lane] = outside[(11 * j + 3 * N + lane) % len(outside)]
    return batch


def run_membership(gpu, batch):
    ctx, groth16 = gpu
    from zkcensus_amd import engines
    g1 = b''.join(ol.g1_mul(engines.G1_GENERATOR, i + 2) for i in range(min(len(batch), 4)))
    g1 = (g1 * (len(batch) // 4 + 1))[:64 * len(batch)]              # arbitrary curve points
    _, bad, _, flags, _ = groth16.debug_pairing_dev(ctx, g1, b''.join(g2_bytes(p) for p in batch), None, members=True)
    return bad, flags


@pytest.mark.parametrize('N', [1, 63, 64, 65, 130])
def test_membership_flags(gpu, g2_pool, N):
    inside, outside = g2_pool
    edges = {l for l in (0, 63, 64, N - 1) if l < N}
    lanes = edges | {l for l in range(N) if l % 7 == 3 and not ({l - 1, l + 1} & edges)}      # the neighbours of an edge lane stay members
    batch = membership_batch(g2_pool, N, lanes)
    if N == 130:
        batch[0], batch[64], batch[129] = g2_py.small_order_point(), g2_add(inside[0], g2_py.small_order_point()), g2_neg(g2_py.small_order_point())
        batch[5] = None
    expected = [0 if (p is None or in_g2(p)) else 1 for p in batch]
    assert [i for i, f in enumerate(expected) if f] == sorted(lanes)
    bad, flags = run_membership(gpu, batch)
    assert flags == expected, [(i, f, e) for i, (f, e) in enumerate(zip(flags, expected)) if f != e]
    assert (bad != 0) == any(flags) and bad != 0


def test_membership_of_every_pool_point(gpu, g2_pool):
    """Every point of the pool once, members and non-members interleaved, and the all-member batches"""
    inside, outside = g2_pool
    batch = []
    for i in range(max(len(inside), len(outside))):
        batch += [outside[i % len(outside)], inside[i % len(inside)]]
    for lo in range(0, len(batch), 130):
        bad, flags = run_membership(gpu, batch[lo:lo + 130])
        assert flags == [1, 0] * (len(flags) // 2) and bad != 0
    for N in (1, 17, 65):
        bad, flags = run_membership(gpu, [inside[i % len(inside)] for i in range(N)])
        assert bad == 0 and flags == [0] * N
    bad, flags = run_membership(gpu, [None])
    assert bad == 0 and flags == [0]


def test_membership_covers_all_rounds(gpu, g2_pool):
    """Rounds of two pairs, seven points, the only non-member last: the membership kernels cover all N whatever the rounds"""
    inside, outside = g2_pool
    for rogue in (outside[0], g2_py.small_order_point()):
        batch = inside[:6] + [rogue]
        with env(ZKC_VERIFY_CHUNK='2'):
            bad, flags = run_membership(gpu, batch)
        assert bad != 0 and flags == [0] * 6 + [1]


# ---- the public surface on a B with a small-order component ----
def test_verifiers_refuse_b_plus_small_order_point(gpu):
    """B + T for T of order 10069: on the twist, outside G2, and e(A, B + T) is what a verifier without the membership test could take for e(A, B).  zkc_verify_bin, both
    paths of verify_batch and verify_each on the GPU refuse it, in the middle of twelve and as the last member of five."""
    import torch, numpy as np
    import zkcensus_amd
    from zkcensus_amd import setup, _native
    from census_gen import random_voter
    ctx, groth16 = gpu
    nl, base, k = 10, 12, 4
    _, zp, vp = setup.ensure_test_artifacts(nl)
    pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read()); vk = json.load(open(vp))
    rng = random.Random(12)
    voters = [random_voter(rng, ol.poseidon, nLevels=nl, depth_c=rng.randint(1, nl), depth_s=rng.randint(1, nl)) for _ in range(base)]
    ws, st = ctx.witness(voters, nLevels=nl); assert st == [0] * base
    d = torch.from_numpy(np.frombuffer(b''.join(ws), dtype=np.uint8).copy()).cuda()
    rs = b''.join(rng.randrange(ol.R).to_bytes(32, 'little') for _ in range(2 * base))
    proofs, pubs = pk.prove_batch_dev(d.data_ptr(), base, rs)
    pk.close()
    P = [proofs[256 * i:256 * (i + 1)] for i in range(base)]; U = [pubs[256 * i:256 * (i + 1)] for i in range(base)]
    assert all(ol.verify(vk, u, p) for p, u in zip(P, U))
    B = g2_point(P[k][64:192]); BT = g2_add(B, g2_py.small_order_point())
    assert in_g2(B) and on_twist(BT) and not in_g2(BT)
    Pb = list(P); Pb[k] = P[k][:64] + g2_bytes(BT) + P[k][192:]
    vkb = groth16.vk_to_bytes(vk); seed = bytes(range(32))
    assert _native.load().zkc_verify_bin(vkb, 8, U[k], P[k]) == 1 and _native.load().zkc_verify_bin(vkb, 8, U[k], Pb[k]) == 0
    for n in (12, 5):
        for path in ('0', '1'):
            with env(ZKC_VERIFY_BATCH_GPU=path):
                assert groth16.verify_batch(ctx, vk, b''.join(U[:n]), b''.join(Pb[:n]), seed) is False, (n, path)
                assert groth16.verify_batch(ctx, vk, b''.join(U[:n]), b''.join(P[:n]), seed) is True
        with env(ZKC_VERIFY_BATCH_GPU='1'):
            got = groth16.verify_each(ctx, vk, b''.join(U[:n]), b''.join(Pb[:n]), seed)
        assert got == [groth16.PROOF_MALFORMED if i == k else groth16.PROOF_VALID for i in range(n)]


# ---- what the hook refuses ----
def test_hook_refusals(gpu, master):
    import zkcensus_amd
    ctx, groth16 = gpu
    members, pts = master
    batch = members[:5]
    g1 = b''.join(pts.g1(a) for a, _, _ in batch); g2 = b''.join(pts.g2(b) for _, b, _ in batch)
    le = lambda v: v.to_bytes(32, 'little')
    y = int.from_bytes(g1[32:64], 'little'); y2 = int.from_bytes(g2[64:96], 'little')
    cases = [(g1[:32] + le((y + 1) % Q) + g1[64:], g2, None),                      # a G1 point off the curve
             (g1, g2[:64] + le((y2 + 1) % Q) + g2[96:], None),                     # a G2 point off the twist
             (b'\xff' * 32 + g1[32:], g2, None), (g1[:64 * 4] + g1[64 * 4:64 * 4 + 32] + le(Q), g2, None),      # a coordinate >= q
             (g1, g2[:128 * 4 + 96] + b'\xff' * 32, None),
             (b'', b'', None),                                                     # N = 0
             (g1, g2, [(1, 0, 0)]), (g1, g2, [(0, 3, 0)]), (g1, g2, [(0, 0, 3)]), (g1, g2, [(0, 0, 0), (0, 2, 1)])]      # no such round, level, node
    assert tree_nodes(5, None).keys() >= {(0, 2, 0), (0, 0, 2)} and (0, 3, 0) not in tree_nodes(5, None)
    for a, b, nodes in cases:
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            groth16.debug_pairing_dev(ctx, a, b, None, folded=True, members=True, nodes=nodes)
        assert ei.value.code == BAD_ARG
    with env(ZKC_VERIFY_CHUNK='2'):                                                # rounds of 2, 2, 1: round 2 has one level of one node
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            groth16.debug_pairing_dev(ctx, g1, g2, None, nodes=[(2, 0, 1)])
        assert ei.value.code == BAD_ARG
    check_batch(gpu, pts, batch)                                                   # the context goes on: an honest product afterwards
