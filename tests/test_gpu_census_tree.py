"""GPU: the census tree that grows in place (census.CensusTree, csrc/zkc_tree.hip) -- after every batch the same tree as the static builder zkc_smt_build over the current
(key, value) set, root and sibling lists byte for byte; its proofs climb to its root with the oracle's Poseidon; refused entries change nothing; and the circuit inputs it
builds for voters of two resident trees equal the static census builder's and pass the witness."""
import random
import pytest
import oracle_lib as ol
from census_lib import W, VALID, fresh_keys, oracle_verdict, sib_list, tree_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


def _check_against_static(ctx, tree, keys, vals, nl, proofs=False, chunk=16384):
    """keys, vals: bytearrays of 32-byte words, the tree's current (key, value) set"""
    from zkcensus_amd import census
    n = len(keys) // 32
    root, sib, dep = census.smt_build(ctx, bytes(keys), bytes(vals), nl, siblings=proofs)
    assert tree.root == root and len(tree) == n
    if not proofs:
        return
    blk = 32 * (nl + 1)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        r, s, d, ex = tree.gen_proof(bytes(keys[32 * lo:32 * hi]))
        assert r == root and all(ex)
        assert d == dep[lo:hi], lo
        assert s == sib[blk * lo:blk * hi], lo


@pytest.mark.parametrize('schedule', ['one_add', 'growing'])
def test_tree_equals_the_static_builder_at_160_levels(ctx, schedule):
    """Random 160-bit-path keys up to 2^15 (one add) / 2^17 (batches of 1, 7, then 1 024, updates interleaved): the root equals zkc_smt_build's after every batch,
    across the many doublings of the device value array; at the end every key's proof equals zkc_smt_build's."""
    from zkcensus_amd import census
    rng = random.Random(160 + len(schedule))
    nl = 160
    tree = census.CensusTree(ctx, nl)
    keys, vals = bytearray(), bytearray()
    if schedule == 'one_add':
        n = 1 << 15
        ks = list(dict.fromkeys(rng.getrandbits(250) for _ in range(n + 16)))[:n]; vs = [rng.randrange(ol.R) for _ in range(n)]
        keys += b''.join(map(W, ks)); vals += b''.join(map(W, vs))
        assert tree.add(bytes(keys), bytes(vals)) == [0] * n
        _check_against_static(ctx, tree, keys, vals, nl, proofs=True)
        tree.close()
        return
    seen = set()
    fresh = lambda m: fresh_keys(rng, seen, m, 253)
    sizes = [1] * 40 + [7] * 40 + [1024] * 127
    for b, m in enumerate(sizes):
        ks = fresh(m); vs = [rng.randrange(ol.R) for _ in range(m)]
        kb, vb = b''.join(map(W, ks)), b''.join(map(W, vs))
        assert tree.add(kb, vb) == [0] * m
        keys += kb; vals += vb
        if b % 5 == 4:                                   # interleaved updates, a key repeated within the batch included (the last value wins)
            n = len(keys) // 32
            idx = [rng.randrange(n) for _ in range(min(n, 50))] + [0, 0]
            nv = [rng.randrange(ol.R) for _ in idx]
            assert tree.update(b''.join(bytes(keys[32 * i:32 * i + 32]) for i in idx), b''.join(map(W, nv))) == [0] * len(idx)
            for i, v in zip(idx, nv):
                vals[32 * i:32 * i + 32] = W(v)
        if m < 1024 or b % 8 == 0 or b == len(sizes) - 1:
            _check_against_static(ctx, tree, keys, vals, nl)
    assert len(tree) == sum(sizes) > (1 << 17) - 1024
    _check_against_static(ctx, tree, keys, vals, nl, proofs=True)
    tree.close()


def test_tree_equals_the_static_builder_at_12_levels(ctx):
    """nLevels 12: 3 000 keys with distinct low 12 bits (a full-depth, densely branching tree), grown in batches of 7 and once in one add; proofs byte-equal."""
    from zkcensus_amd import census
    rng = random.Random(12)
    nl = 12
    ks = tree_keys(rng, nl, 3000); vs = [rng.randrange(ol.R) for _ in ks]
    kb, vb = b''.join(map(W, ks)), b''.join(map(W, vs))
    with census.CensusTree(ctx, nl) as whole:
        assert whole.add(kb, vb) == [0] * len(ks)
        _check_against_static(ctx, whole, kb, vb, nl, proofs=True)
        with census.CensusTree(ctx, nl) as grown:
            for lo in range(0, len(ks), 7):
                assert grown.add(kb[32 * lo:32 * (lo + 7)], vb[32 * lo:32 * (lo + 7)]) == [0] * len(ks[lo:lo + 7])
                if lo % 700 == 0:
                    _check_against_static(ctx, grown, kb[:32 * (lo + 7)], vb[:32 * (lo + 7)], nl)
            _check_against_static(ctx, grown, kb, vb, nl, proofs=True)
            assert grown.root == whole.root
            assert grown.get(ks[:100]) == (vs[:100], [True] * 100)


def test_proofs_climb_to_the_root_with_the_oracle_poseidon(ctx):
    """A 40-leaf nLevels-12 tree grown one key at a time: after every add, every key's proof climbs to the returned root with the oracle's Poseidon (no GPU code
    on the checking side)."""
    from zkcensus_amd import census
    rng = random.Random(40)
    nl = 12
    ks = rng.sample(range(1 << nl), 40); vs = [rng.randrange(ol.R) for _ in ks]; vs[3] = ol.R - 1
    with census.CensusTree(ctx, nl) as tree:
        for j, (k, v) in enumerate(zip(ks, vs)):
            assert tree.add([k], [v]) == [0]
            root, sib, dep, ex = tree.gen_proof(ks[:j + 1])
            assert all(ex) and root == tree.root
            for i in range(j + 1):
                s = sib_list(sib, i, nl)
                assert all(x == 0 for x in s[dep[i]:])
                assert oracle_verdict(ks[i], vs[i], s, root, nl) == VALID, (j, i)
        assert len(tree) == 40


def test_shapes_and_refusals(ctx):
    from zkcensus_amd import census
    T = census.CensusTree
    kv = {}
    with census.CensusTree(ctx, 160) as tree:
        def same():
            assert tree.root == census.smt_build(ctx, list(kv), list(kv.values()), 160, siblings=False)[0]
        assert tree.root == 0 and len(tree) == 0
        # two keys parting at bit 40: a chain of 41 inner nodes; then a third key that leaves the chain at bit 20
        a, b, c = 5, 5 + (1 << 40), 5 + (1 << 20)
        assert tree.add([a, b], [7, 9]) == [0, 0]; kv.update({a: 7, b: 9}); same()
        assert tree.gen_proof([a, b])[2] == [41, 41]
        assert tree.add([c], [11]) == [0]; kv[c] = 11; same()
        r, sib, dep, ex = tree.gen_proof([a, b, c])
        _, ssib, sdep = census.smt_build(ctx, [a, b, c], [7, 9, 11], 160)
        assert (dep, sib) == (sdep, ssib) and dep == [41, 41, 21]
        # updating the key at the bottom of the chain
        assert tree.update([b], [123]) == [0]; kv[b] = 123; same()
        before = tree.root
        # refusals, none of which changes the root: a key already in the tree, a key repeated within one batch, an absent key, a value or key equal to r
        assert tree.add([a], [1]) == [T.KEY_EXISTS]
        assert tree.update([77], [1]) == [T.KEY_ABSENT]
        assert tree.add([78], [ol.R]) == [T.NOT_BELOW_R] and tree.add([ol.R], [1]) == [T.NOT_BELOW_R]
        assert tree.update([a], [ol.R]) == [T.NOT_BELOW_R]
        assert tree.root == before and len(tree) == 3
        assert tree.get([77, a]) == ([0, 7], [False, True])
        r, sib, dep, ex = tree.gen_proof([77])
        assert r == before and ex == [False] and dep == [0] and sib == b'\0' * 32 * 161
        # a mixed batch: the accepted entries are applied, in order; a repeated key keeps its first value
        st = tree.add([1000, a, 1001, 1002, 1000], [1, 2, ol.R, 3, 4])
        assert st == [T.OK, T.KEY_EXISTS, T.NOT_BELOW_R, T.OK, T.KEY_EXISTS]
        kv.update({1000: 1, 1002: 3}); same()
        assert tree.get([1000, 1001]) == ([1, 0], [True, False])
        st = tree.update([1000, 1001, 1000], [5, 6, 8])
        assert st == [T.OK, T.KEY_ABSENT, T.OK]
        kv[1000] = 8; same()
    # a collision on the first nLevels path bits
    with census.CensusTree(ctx, 12) as tree:
        assert tree.add([1], [1]) == [0]
        before = tree.root
        assert tree.add([1 + (1 << 12), 2], [2, 3]) == [T.COLLISION, T.OK]
        assert tree.root == census.smt_build(ctx, [1, 2], [1, 3], 12, siblings=False)[0] != before and len(tree) == 2
        assert tree.add([1 + (1 << 13)], [2]) == [T.COLLISION]
        assert tree.get([1 + (1 << 12)])[1] == [False]


def test_census_inputs_from_resident_trees_equal_the_static_census(ctx):
    """The 8 192-voter synthetic census grown as two resident trees (census: address -> weight, SIK: address -> SIK) in batches of 512: the inputs of 64 voters
    equal the static census builder's blocks and pass the witness; a wrong password, a stranger and a voter missing from the SIK tree get their status and a zeroed block."""
    from zkcensus_amd import census
    from zkcensus_amd.inputs import bytes_to_arbo
    T = census.CensusTree
    N, nl = 8192, 160
    nIn = 12 + 2 * (nl + 1); blk = 32 * nIn
    eid, address, password, signature, avail = census._voter_data(N, census.ELECTION_ID_HEX)
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    flat_ref, croot, sroot = census.synthetic_census_flat(ctx, N, nl)
    with census.CensusTree(ctx, nl) as ct, census.CensusTree(ctx, nl) as stree:
        for lo in range(0, N, 512):
            assert ct.add(address[lo:lo + 512], avail[lo:lo + 512]) == [0] * 512
            assert stree.add(address[lo:lo + 512], sik[lo:lo + 512]) == [0] * 512
        assert (ct.root, stree.root) == (croot, sroot)
        idx = list(range(0, N, 128))
        vh = lambda i: bytes_to_arbo(avail[i].to_bytes((avail[i].bit_length() + 7) // 8 or 1, 'big'))
        pick = lambda xs: [xs[i] for i in idx]
        flat, cr, sr, st = census.census_inputs_from_trees(ctx, ct, stree, eid, pick(address), pick(password), pick(signature), [1] * 64, [vh(i) for i in idx])
        assert st == [0] * 64 and (cr, sr) == (croot, sroot)
        assert flat == b''.join(flat_ref[blk * i:blk * (i + 1)] for i in idx)
        ws, wst = ctx.witness([flat[blk * j:blk * (j + 1)] for j in range(64)], nl)
        assert wst == [0] * 64
        # a wrong password (SIK mismatch), a stranger, a voter the SIK tree does not hold: statuses and zeroed blocks; the voters beside them are unaffected
        stranger = 12345
        assert ct.add([stranger], [3]) == [0]
        i0, i1 = idx[0], idx[1]
        flat, cr, sr, st = census.census_inputs_from_trees(ctx, ct, stree, eid, [address[i0], 999, stranger, address[i1]], [password[i0] + 1, 1, 1, password[i1]],
                                                           [signature[i0], 1, 1, signature[i1]], [1] * 4, [vh(i0), vh(i0), vh(i0), vh(i1)])
        assert st == [T.SIK_MISMATCH, T.NOT_IN_CENSUS, T.NOT_IN_SIK, T.OK]
        assert flat[:3 * blk] == b'\0' * 3 * blk
        assert sr == sroot and cr == ct.root != croot
        # the last voter's block: the static census's, but for the census root and census siblings of the grown census tree
        r, csib, _, ex = ct.gen_proof([address[i1]])
        assert r == cr and ex == [True]
        want = bytearray(flat_ref[blk * i1:blk * (i1 + 1)])
        want[32 * 7:32 * 8] = W(cr); want[32 * 12:32 * (12 + nl + 1)] = csib
        assert flat[3 * blk:] == bytes(want)
