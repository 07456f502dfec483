"""GPU: voters removed from a resident census tree (CensusTree.delete, zkc_tree_delete) and keys proven absent (CensusTree.gen_absence_proof,
zkc_tree_gen_absence_proof; census.check_absence, zkc_smt_check_absence).  After every delete batch the tree equals zkc_smt_build over what is left, root, sibling
lists and depths byte for byte; the roots of the delete shapes equal a pure-Python tree over the oracle's Poseidon; refused entries change nothing; churn at constant
size keeps the node arrays bounded; every absence proof the tree hands out is valid, each kind of tampering gets its exact verdict, and the verdicts equal a
pure-Python reading of circomlib's SMTVerifier (fnc = 1) and do not depend on the kernel form or on how a batch is cut."""
import ctypes
import random
import pytest
import oracle_lib as ol
from census_lib import (W, words, VALID, ROOT_MISMATCH, NOT_BELOW_R, LAST_SIBLING, KEY_PRESENT, OFF_PATH, ZKC_ERR_BAD_ARG, equals_rebuild, fresh_keys, oracle_verdict,
                        sib_list, tree_keys)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


def py_root(items, d=0):
    """the arbo root of (key, value) pairs in pure Python over the oracle's Poseidon"""
    if not items:
        return 0
    if len(items) == 1:
        return ol.poseidon([items[0][0], items[0][1], 1])
    return ol.poseidon([py_root([x for x in items if not (x[0] >> d) & 1], d + 1), py_root([x for x in items if (x[0] >> d) & 1], d + 1)])


@pytest.mark.parametrize('nl,order', [(160, 'random'), (160, 'adversarial'), (12, 'random'), (12, 'adversarial')])
def test_delete_equals_rebuild(ctx, nl, order):
    """2 500 keys deleted in batches of 1, 7, 64 and 1 000 in turn down to empty, in random order or in path order (bit-reversed low bits: whole subtrees go
    one after the other, so lifts and chain collapses happen all the time); after every batch the tree equals zkc_smt_build over what is left.  Re-adding every key
    gives the first root back."""
    from zkcensus_amd import census
    rng = random.Random(nl * 7 + len(order))
    n = 2500
    ks = tree_keys(rng, nl, n); vs = [rng.randrange(ol.R) for _ in ks]
    kv = dict(zip(ks, vs))
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks, vs) == [0] * n
        first = tree.root
        equals_rebuild(ctx, tree, kv, nl)
        if order == 'random':
            gone = rng.sample(ks, n)
        else:
            rev = lambda k: int(format(k & ((1 << 24) - 1), '024b')[::-1], 2)
            gone = sorted(ks, key=rev)
        sizes = [1, 7, 64, 1000]; b = 0; lo = 0
        while lo < n:
            batch = gone[lo:lo + sizes[b % 4]]
            assert tree.delete(batch) == [0] * len(batch)
            for k in batch:
                del kv[k]
            equals_rebuild(ctx, tree, kv, nl)
            lo += len(batch); b += 1
        assert tree.root == 0 and len(tree) == 0
        assert tree.add(ks, vs) == [0] * n
        assert tree.root == first
        equals_rebuild(ctx, tree, dict(zip(ks, vs)), nl)


def test_delete_shapes(ctx):
    """Each shape against a rebuild and against the pure-Python tree: two keys sharing 150 path bits (deleting either lifts the other to the root: the root is that
    leaf's hash); a long chain that collapses into a higher node; a sibling that is an inner node (no lift, the parent stays a one-child chain node); both children
    of a node deleted in one batch."""
    from zkcensus_amd import census
    nl = 160

    def run(items, deletes):
        kv = dict(items)
        with census.CensusTree(ctx, nl) as tree:
            assert tree.add(list(kv), list(kv.values())) == [0] * len(kv)
            assert tree.root == py_root(list(kv.items()))
            for batch in deletes:
                assert tree.delete(batch) == [0] * len(batch)
                for k in batch:
                    del kv[k]
                assert tree.root == py_root(list(kv.items()))
                equals_rebuild(ctx, tree, kv, nl)
            return tree.root
    a = 0b1011; b = a + (1 << 150)
    for gone, left in [(a, b), (b, a)]:
        assert run([(a, 5), (b, 6)], [[gone]]) == ol.poseidon([left, 5 if left == a else 6, 1])
    # x on the left of the root; a and b on the right, sharing 100 bits: deleting a lifts b from depth 101 to depth 1
    x = 0b10; a = 1 + (1 << 40); b = a + (1 << 100)
    assert run([(x, 1), (a, 2), (b, 3)], [[a]]) == ol.poseidon([ol.poseidon([x, 1, 1]), ol.poseidon([b, 3, 1])])
    # a chain of 60 levels whose bottom pair goes one by one: the last leaf climbs all the way past the chain to the root's child
    c = 1 + (1 << 60); d = c + (1 << 70)
    run([(x, 1), (c, 2), (d, 3), (a, 4)], [[c], [a]])
    # the sibling is an inner node: a, b under the root's left child; deleting c (the root's right child) leaves the root with one inner child
    a, b, c = 0b00, 0b10, 0b1
    assert run([(a, 1), (b, 2), (c, 3)], [[c]]) == ol.poseidon([ol.poseidon([ol.poseidon([a, 1, 1]), ol.poseidon([b, 2, 1])]), 0])
    # deeper: the sibling inner node is several levels down a chain
    a, b, c = 1 << 50, (1 << 50) + (1 << 51), 1 << 10
    run([(a, 1), (b, 2), (c, 3), (0b1, 4)], [[c]])
    # both children of a node deleted in one batch; then the two children of another node, leaving an inner node alone on one side
    a, b, c, e = 0b000, 0b100, 0b010, 0b1
    assert run([(a, 1), (b, 2), (c, 3), (e, 4)], [[a, b]]) == ol.poseidon([ol.poseidon([c, 3, 1]), ol.poseidon([e, 4, 1])])
    run([(0b0000, 1), (0b1000, 2), (0b0100, 3), (0b1100, 4), (0b1, 5)], [[0b0100, 0b1100], [0b1], [0b0000, 0b1000]])


def test_delete_batch_semantics(ctx):
    from zkcensus_amd import census
    T = census.CensusTree
    with census.CensusTree(ctx, 160) as tree:
        ks = [11, 12, 13, 14, 1 << 90]; vs = [1, 2, 3, 4, 5]
        assert tree.add(ks, vs) == [0] * 5
        full = tree.root
        # a repeated key: KEY_ABSENT the second time; an absent key and a key >= r: refused, nothing changes
        assert tree.delete([12, 12]) == [T.OK, T.KEY_ABSENT]
        after = tree.root
        assert after == py_root([(11, 1), (13, 3), (14, 4), (1 << 90, 5)])
        assert tree.delete([999, ol.R, ol.R + 11]) == [T.KEY_ABSENT, T.NOT_BELOW_R, T.NOT_BELOW_R]
        assert tree.root == after and len(tree) == 4
        assert tree.delete([]) == []
        # add, delete, add of the same key across calls: the same root
        assert tree.add([12], [2]) == [T.OK] and tree.root == full
        assert tree.delete([12]) == [T.OK] and tree.root == after
        assert tree.add([12], [2]) == [T.OK] and tree.root == full
        # within one batch: delete then re-add is not possible (add and delete are separate calls), but delete, then a failed delete, then delete of another key
        assert tree.delete([13, 13, 14]) == [T.OK, T.KEY_ABSENT, T.OK]
        assert tree.root == py_root([(11, 1), (12, 2), (1 << 90, 5)])
        assert tree.get([13, 11]) == ([0, 1], [False, True])
        assert tree.update([13], [1]) == [T.KEY_ABSENT]
        # delete everything, then the tree is usable again
        assert tree.delete([11, 12, 1 << 90]) == [T.OK] * 3 and tree.root == 0 and len(tree) == 0
        assert tree.gen_proof([11])[:3] == (0, b'\0' * 32 * 161, [0])
        assert tree.add([5], [6]) == [T.OK] and tree.root == ol.poseidon([5, 6, 1])
        lib = tree._lib
        st = (ctypes.c_int32 * 1)(77)
        assert lib.zkc_tree_delete(tree._h, None, 1, st) == ZKC_ERR_BAD_ARG and list(st) == [77]
        assert lib.zkc_tree_delete(tree._h, W(5), 1, None) == ZKC_ERR_BAD_ARG
        assert lib.zkc_tree_refs(tree._h, None) == ZKC_ERR_BAD_ARG
        assert tree.root == ol.poseidon([5, 6, 1])


def test_frozen_root_and_census_inputs_after_delete(ctx):
    """A membership proof taken before a delete holds against the frozen root only.  After removing one voter from the census tree and another from the SIK tree,
    census_inputs_from_trees gives NOT_IN_CENSUS / NOT_IN_SIK for them and, for the others, the blocks of two trees built fresh over the remaining voters."""
    from zkcensus_amd import census
    T = census.CensusTree
    N, nl = 512, 160
    eid, address, password, signature, avail = census._voter_data(N, census.ELECTION_ID_HEX)
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    vh = [[1, 2]] * 4
    with census.CensusTree(ctx, nl) as ct, census.CensusTree(ctx, nl) as stree:
        assert ct.add(address, avail) == [0] * N and stree.add(address, sik) == [0] * N
        frozen = ct.root
        r, sib, dep, ex = ct.gen_proof([address[5]])
        assert ex == [True] and r == frozen
        assert ct.delete([address[0]]) == [T.OK] and stree.delete([address[1]]) == [T.OK]
        assert ct.check_proofs([address[5]], [avail[5]], sib, frozen) == [VALID]
        assert ct.check_proofs([address[5]], [avail[5]], sib) == [ROOT_MISMATCH]
        pick = lambda xs: [xs[i] for i in range(4)]
        flat, cr, sr, st = census.census_inputs_from_trees(ctx, ct, stree, eid, pick(address), pick(password), pick(signature), [1] * 4, vh)
        assert st == [T.NOT_IN_CENSUS, T.NOT_IN_SIK, T.OK, T.OK]
        nIn = 12 + 2 * (nl + 1); blk = 32 * nIn
        assert flat[:2 * blk] == b'\0' * 2 * blk
        with census.CensusTree(ctx, nl) as ct2, census.CensusTree(ctx, nl) as st2:
            assert ct2.add(address[1:], avail[1:]) == [0] * (N - 1)
            assert st2.add(address[:1] + address[2:], sik[:1] + sik[2:]) == [0] * (N - 1)
            assert (ct2.root, st2.root) == (ct.root, stree.root) == (cr, sr)
            f2, _, _, st2s = census.census_inputs_from_trees(ctx, ct2, st2, eid, address[2:4], password[2:4], signature[2:4], [1] * 2, vh[:2])
            assert st2s == [T.OK, T.OK] and flat[2 * blk:] == f2


def test_churn_is_bounded(ctx):
    """A 4 096-leaf tree, 50 rounds of deleting 1 024 voters and adding 1 024 fresh ones: the node arrays grow by at most one batch's worth after the first round,
    and the tree still equals a rebuild."""
    from zkcensus_amd import census
    rng = random.Random(4096)
    nl = 160
    seen = set()
    fresh = lambda m: fresh_keys(rng, seen, m, 160)
    ks = fresh(4096)
    kv = {k: rng.randrange(ol.R) for k in ks}
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * 4096
        first = None
        for rnd in range(50):
            gone = rng.sample(list(kv), 1024)
            assert tree.delete(gone) == [0] * 1024
            for k in gone:
                del kv[k]
            new = fresh(1024); nv = [rng.randrange(ol.R) for _ in new]
            assert tree.add(new, nv) == [0] * 1024
            kv.update(zip(new, nv))
            live, alloc = tree.refs()
            assert live <= alloc and len(tree) == 4096
            if first is None:
                first = alloc
        assert alloc <= first + 2 * 1024, (first, alloc)
        equals_rebuild(ctx, tree, kv, nl)


def _check_all(ctx, tree, keys, root=None):
    """gen_absence_proof for absent keys, checked on the GPU against the tree's root and against the pure-Python reading; returns the proof pieces"""
    from zkcensus_amd import census
    nl = tree.nLevels
    r, sib, dep, ok, ov, o0, st = tree.gen_absence_proof(keys)
    assert st == [0] * len(keys)
    assert r == tree.root
    v = tree.check_absence(keys, ok, ov, o0, sib)
    assert v == [VALID] * len(keys)
    for i in range(len(keys)):
        s = sib_list(sib, i, nl)
        assert all(x == 0 for x in s[dep[i]:])
        assert oracle_verdict(keys[i], ov[i], s, r, nl, ok[i], o0[i]) == VALID
    assert census.check_absence(ctx, keys, ok, ov, o0, sib, [r] * len(keys), nl) == [VALID] * len(keys)
    return r, sib, dep, ok, ov, o0


def test_absence_proofs(ctx):
    from zkcensus_amd import census
    T = census.CensusTree
    rng = random.Random(55)
    nl = 160
    with census.CensusTree(ctx, nl) as tree:
        # the empty tree
        r, sib, dep, ok, ov, o0, st = tree.gen_absence_proof([7])
        assert (r, dep, ok, ov, o0, st) == (0, [0], [0], [0], [1], [0]) and sib == b'\0' * 32 * (nl + 1)
        assert tree.check_absence([7], ok, ov, o0, sib) == [VALID]
        # a single leaf at the root: any other key's path runs into it at depth 0
        assert tree.add([9], [10]) == [0]
        r, sib, dep, ok, ov, o0 = _check_all(ctx, tree, [7, 8])
        assert dep == [0, 0] and o0 == [0, 0] and ok == [9, 9] and ov == [10, 10]
        ks = tree_keys(rng, nl, 3000); vs = [rng.randrange(ol.R) for _ in ks]
        assert tree.add(ks, vs) == [0] * 3000
        present = set(ks) | {9}
        # random absent keys; keys sharing a long prefix with a present key; just-deleted keys
        rand = [k for k in tree_keys(rng, nl, 300) if k not in present]
        near = [k ^ (1 << rng.randrange(20, 159)) for k in ks[:200]]
        near = [k for k in near if k not in present]
        gone = ks[-100:]
        assert tree.delete(gone) == [0] * 100
        for group in (rand, near, gone):
            r, sib, dep, ok, ov, o0 = _check_all(ctx, tree, group)
        r, sib, dep, ok, ov, o0 = _check_all(ctx, tree, rand + near + gone)
        assert 0 < sum(o0) < len(o0)                                   # both kinds occur
        # a present key
        r2, _, dep2, ok2, ov2, o02, st2 = tree.gen_absence_proof([ks[0], rand[0], ol.R])
        assert st2 == [T.KEY_EXISTS, T.OK, T.NOT_BELOW_R] and dep2[0] == dep2[2] == 0 and ok2[0] == ov2[0] == o02[0] == 0
        # tampering: one proof of each kind with depth > 0
        keys = rand + near + gone
        i1 = next(i for i in range(len(keys)) if o0[i] == 0 and dep[i] > 0)
        i0 = next(i for i in range(len(keys)) if o0[i] == 1 and dep[i] > 0)
        blk = 32 * (nl + 1)

        def one(i, key=None, okey=None, oval=None, old0=None, sibs=None, root=None):
            s = sib_list(sib, i, nl) if sibs is None else sibs
            args = (keys[i] if key is None else key, ok[i] if okey is None else okey, ov[i] if oval is None else oval, o0[i] if old0 is None else old0)
            rt = r if root is None else root
            got = census.check_absence(ctx, [args[0]], [args[1]], [args[2]], [args[3]], words(s), rt, nl)[0]
            assert got == oracle_verdict(args[0], args[2], s, rt, nl, args[1], args[3])
            return got
        for i in (i0, i1):
            assert one(i) == VALID
            s = sib_list(sib, i, nl); s[dep[i] - 1] = (s[dep[i] - 1] + 1) % ol.R or 1
            assert one(i, sibs=s) == ROOT_MISMATCH
            s = sib_list(sib, i, nl); s[nl] = 1
            assert one(i, sibs=s) == LAST_SIBLING
            s = sib_list(sib, i, nl); s[0] = ol.R
            assert one(i, sibs=s) == NOT_BELOW_R
            assert one(i, key=ol.R) == NOT_BELOW_R and one(i, root=ol.R) == NOT_BELOW_R and one(i, oval=ol.R + 3) == NOT_BELOW_R
            assert one(i, okey=ol.R) == NOT_BELOW_R
            assert one(i, old0=0, okey=keys[i]) == KEY_PRESENT
            assert one(i, old0=0, okey=keys[i] ^ 1) == OFF_PATH
            assert one(i, old0=0, okey=keys[i] ^ (1 << (dep[i] - 1))) == OFF_PATH
            assert one(i, root=r + 1) == ROOT_MISMATCH
        assert one(i1, old0=1) == ROOT_MISMATCH
        assert one(i0, old0=0, okey=keys[i0] ^ (1 << 200)) == ROOT_MISMATCH          # on the path, but no such leaf is there
        from zkcensus_amd import ZkcError
        with pytest.raises(ZkcError):
            census.check_absence(ctx, [keys[i0]], [0], [0], [2], sib[blk * i0:blk * (i0 + 1)], r, nl)
        # a key added afterwards: its absence proof holds against the root it was taken under, not against the one after the add
        k = rand[1]
        r0, sib0, _, ok0, ov0, o00, st0 = tree.gen_absence_proof([k])
        assert st0 == [0] and tree.add([k], [1]) == [0]
        assert tree.check_absence([k], ok0, ov0, o00, sib0, r0) == [VALID]
        assert tree.check_absence([k], ok0, ov0, o00, sib0) == [ROOT_MISMATCH]
        assert tree.gen_absence_proof([k])[6] == [T.KEY_EXISTS]


def test_absence_at_12_levels(ctx):
    """A crowded nLevels-12 tree: absence proofs of keys whose low 12 bits are free (empty child or a leaf above) are valid, with the oracle agreeing."""
    from zkcensus_amd import census
    rng = random.Random(1212)
    nl = 12
    low = rng.sample(range(1 << nl), 1500)
    ks = [l | (rng.getrandbits(200) << nl) for l in low]; vs = [rng.randrange(ol.R) for _ in ks]
    free = sorted(set(range(1 << nl)) - set(low))
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks, vs) == [0] * len(ks)
        absent = [l | (rng.getrandbits(200) << nl) for l in rng.sample(free, 400)]
        r, sib, dep, ok, ov, o0 = _check_all(ctx, tree, absent)
        assert 0 < sum(o0) < len(o0)
        # the same low bits as a present key and different high bits: a COLLISION for add, and the gen_absence_proof walk ends at that very leaf
        twin = ks[0] ^ (1 << 100)
        r, sib, dep, ok, ov, o0, st = tree.gen_absence_proof([twin])
        assert st == [0] and o0 == [0] and ok == [ks[0]]
        assert tree.check_absence([twin], ok, ov, o0, sib) == [VALID]


def test_both_kernel_forms_and_every_depth(ctx):
    """Synthetic exclusion proofs at every depth 0..160, both is_old0 kinds, roots right and wrong (climbed with the oracle's Poseidon): one batch (one lane per proof)
    and batches of at most 64 (one wave per proof) give the same verdicts, and they are the oracle's."""
    from zkcensus_amd import census
    rng = random.Random(161)
    nl = 160
    keys, oks, ovs, o0s, sibs, roots, want = [], [], [], [], b'', [], []
    for d in range(nl + 1):
        for old0 in (0, 1):
            key = rng.getrandbits(160)
            okey = 0 if old0 else key ^ (1 << rng.randrange(max(d, 160), 250))     # shares the first d bits, differs above
            oval = 0 if old0 else rng.randrange(ol.R)
            s = [rng.randrange(1, ol.R) if l < d else 0 for l in range(nl + 1)]
            cur = 0 if old0 else ol.poseidon([okey, oval, 1])
            for l in range(d - 1, -1, -1):
                cur = ol.poseidon([s[l], cur]) if (key >> l) & 1 else ol.poseidon([cur, s[l]])
            bad = rng.random() < 0.3
            keys.append(key); oks.append(okey); ovs.append(oval); o0s.append(old0); sibs += words(s)
            roots.append((cur + 1) % ol.R if bad else cur); want.append(ROOT_MISMATCH if bad else VALID)
    n = len(keys); blk = 32 * (nl + 1)
    whole = census.check_absence(ctx, keys, oks, ovs, o0s, sibs, roots, nl)
    assert whole == want
    for i in rng.sample(range(n), 40):
        assert oracle_verdict(keys[i], ovs[i], sib_list(sibs, i, nl), roots[i], nl, oks[i], o0s[i]) == want[i]
    cut = []
    for lo in range(0, n, 64):
        hi = min(n, lo + 64)
        cut += census.check_absence(ctx, keys[lo:hi], oks[lo:hi], ovs[lo:hi], o0s[lo:hi], sibs[blk * lo:blk * hi], roots[lo:hi], nl)
    assert cut == want
    assert [census.check_absence(ctx, [keys[i]], [oks[i]], [ovs[i]], [o0s[i]], sibs[blk * i:blk * (i + 1)], roots[i], nl)[0] for i in range(0, n, 23)] == want[::23]


def test_two_to_the_17_proofs_in_one_call(ctx):
    """2^17 absence proofs from a resident tree (nLevels 40, so the host buffers stay small), checked in one call and in two halves: the same verdicts, all valid, and
    the same with every tenth root wrong."""
    from zkcensus_amd import census
    rng = random.Random(17)
    nl = 40
    ks = [l | (rng.getrandbits(200) << nl) for l in rng.sample(range(1 << nl), 8192)]; vs = [rng.randrange(ol.R) for _ in ks]      # distinct low 40 bits, random high bits
    present = set(ks)
    n = 1 << 17
    absent = [k for k in dict.fromkeys(rng.getrandbits(nl) for _ in range(n + 4096)) if k not in present][:n]
    assert len(absent) == n
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks, vs) == [0] * len(ks)
        r, sib, dep, ok, ov, o0, st = tree.gen_absence_proof(absent)
        assert st == [0] * n and 0 < sum(o0) < n
        roots = [r + 1 if i % 10 == 3 else r for i in range(n)]
        want = [ROOT_MISMATCH if i % 10 == 3 else VALID for i in range(n)]
        assert census.check_absence(ctx, absent, ok, ov, o0, sib, roots, nl) == want
        h = n // 2; blk = 32 * (nl + 1)
        halves = (census.check_absence(ctx, absent[:h], ok[:h], ov[:h], o0[:h], sib[:blk * h], roots[:h], nl)
                  + census.check_absence(ctx, absent[h:], ok[h:], ov[h:], o0[h:], sib[blk * h:], roots[h:], nl))
        assert halves == want
        for i in rng.sample(range(n), 64):
            assert oracle_verdict(absent[i], ov[i], sib_list(sib, i, nl), roots[i], nl, ok[i], o0[i]) == want[i]
        assert min(census.check_stats(ctx)) >= 0
