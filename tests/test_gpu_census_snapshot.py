"""GPU: snapshots of a resident census tree (CensusTree.snapshot, zkc_tree_snapshot; include/zkcensus_snapshot.h).  A snapshot is a read-only view of the tree at
the version it was taken; the live tree goes on changing underneath and copies the paths it modifies.  Every live snapshot equals zkc_smt_build over the set recorded
in Python when it was taken -- root, sibling lists, depths, values, size, absence proofs -- after any later add / update / delete; census_inputs_from_trees over a census
snapshot gives the blocks of a tree built fresh from the frozen set, and the witness accepts them; holding a snapshot costs references in proportion to the changes,
and releasing it gives them back for reuse; snapshots may be released in any order, outlive the live tree, and refuse changes."""
import ctypes
import random
import threading
import pytest
import oracle_lib as ol
from census_lib import W, ZKC_ERR_BAD_ARG, equals_rebuild, fresh_tree, tree_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


def depths(tree, keys):
    """gen_proof's depths alone (no sibling buffer)"""
    from zkcensus_amd import census
    kb = census._le(keys); n = len(kb) // 32
    r = ctypes.create_string_buffer(32); dep = (ctypes.c_int32 * n)(); ex = (ctypes.c_int32 * n)()
    tree.ctx._check(tree._lib.zkc_tree_gen_proof(tree._h, kb, n, r, None, dep, ex))
    assert all(ex)
    return list(dep)


def run_batch(tree, kv, op, keys, values, nl):
    """one change call, its statuses checked against the Python model `kv` (updated in place) entry by entry"""
    from zkcensus_amd import census
    T = census.CensusTree
    low = lambda k: k & ((1 << nl) - 1)
    if op == 'add':
        st = tree.add(keys, values)
        lows = {low(k) for k in kv} if nl < 64 else None
        for k, v, s in zip(keys, values, st):
            want = T.KEY_EXISTS if k in kv else T.COLLISION if lows is not None and low(k) in lows else T.OK
            assert s == want
            if s == T.OK:
                kv[k] = v
                if lows is not None:
                    lows.add(low(k))
    elif op == 'update':
        st = tree.update(keys, values)
        for k, v, s in zip(keys, values, st):
            assert s == (T.OK if k in kv else T.KEY_ABSENT)
            if s == T.OK:
                kv[k] = v
    else:
        st = tree.delete(keys)
        for k, s in zip(keys, st):
            assert s == (T.OK if k in kv else T.KEY_ABSENT)
            if s == T.OK:
                del kv[k]
    return st


@pytest.mark.parametrize('nl,n', [(160, 4096), (12, 3000)])
def test_frozen_views_stay_exact(ctx, nl, n):
    """A random schedule of 12 add / update / delete batches, a snapshot taken after the build and after every batch; after every batch every live snapshot equals a
    rebuild of the set it was taken over (old values after later updates, deleted keys still there, later keys absent) and the live tree equals a rebuild of the current
    set.  At nLevels 12 the adds also meet collisions; re-added keys reuse what deletes freed."""
    from zkcensus_amd import census
    rng = random.Random(nl * 31 + n)
    ks = tree_keys(rng, nl, n)
    kv = {k: rng.randrange(ol.R) for k in ks}
    seen, gone = set(ks), []
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * n
        snaps = [(tree.snapshot(), dict(kv))]
        for b in range(12):
            op = ['add', 'update', 'delete'][b % 3] if b < 3 else rng.choice(['add', 'update', 'delete'])
            m = rng.choice([1, 17, 100, 300])
            present = list(kv)
            if op == 'add':
                if nl < 32:
                    m = min(m, ((1 << nl) - len(seen)) // 4)
                new = tree_keys(rng, nl, m, avoid=seen | set(kv))
                seen.update(new)
                keys = new + rng.sample(gone, min(len(gone), m // 4)) + rng.sample(present, min(3, m))
                if nl < 32:                                        # same low bits as a present key, other high bits: COLLISION
                    keys += [k ^ (1 << 100) for k in rng.sample(present, 3)]
            elif op == 'update':
                keys = rng.sample(present, m) + [rng.getrandbits(nl) | (1 << 220)]
            else:
                keys = rng.sample(present, m) + rng.sample(gone, min(len(gone), 2))
            rng.shuffle(keys)
            values = [rng.randrange(ol.R) for _ in keys]
            before = set(kv)
            run_batch(tree, kv, op, keys, values, nl)
            gone += [k for k in before if k not in kv]
            later = keys + gone[-50:]
            equals_rebuild(ctx, tree, kv, nl, later)
            for s, skv in snaps:
                equals_rebuild(ctx, s, skv, nl, later)
            snaps.append((tree.snapshot(), dict(kv)))
            assert tree.snapshot_count() == len(snaps)
        assert all(s.is_snapshot for s, _ in snaps) and not tree.is_snapshot
        for s, _ in snaps:
            s.close()
        assert tree.snapshot_count() == 0
        equals_rebuild(ctx, tree, kv, nl, gone[-50:])


def test_election_inputs_against_a_frozen_root(ctx):
    """An election freezes the census: after the snapshot the live census adds voters, deletes one and changes another's weight.  census_inputs_from_trees(snapshot,
    live SIK tree) gives the blocks of a census tree built fresh from the frozen set, the witness accepts them with censusRoot = the frozen root; the deleted voter is
    still OK, a voter added after the snapshot is NOT_IN_CENSUS."""
    from zkcensus_amd import census
    from zkcensus_amd.inputs import bytes_to_arbo
    T = census.CensusTree
    N, nl = 520, 160
    nIn = 12 + 2 * (nl + 1); blk = 32 * nIn
    eid, address, password, signature, avail = census._voter_data(N, census.ELECTION_ID_HEX)
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    vh = lambda w: bytes_to_arbo(w.to_bytes((w.bit_length() + 7) // 8 or 1, 'big'))
    M = 512                                                    # voters 512 .. 519 register after the election opened
    with census.CensusTree(ctx, nl) as ct, census.CensusTree(ctx, nl) as stree:
        assert ct.add(address[:M], avail[:M]) == [0] * M and stree.add(address[:M], sik[:M]) == [0] * M
        frozen_set = dict(zip(address[:M], avail[:M]))
        with ct.snapshot() as snap:
            frozen = snap.root
            assert ct.add(address[M:], avail[M:]) == [0] * (N - M) and stree.add(address[M:], sik[M:]) == [0] * (N - M)
            assert ct.delete([address[0]]) == [T.OK]
            assert ct.update([address[1]], [77]) == [T.OK]
            assert ct.root != frozen and snap.root == frozen
            idx = [0, 1, 2, 3, 100, 511, M, M + 7]
            pick = lambda xs: [xs[i] for i in idx]
            args = (eid, pick(address), pick(password), pick(signature), [1] * len(idx), [vh(avail[i]) for i in idx])
            flat, cr, sr, st = census.census_inputs_from_trees(ctx, snap, stree, *args)
            assert st == [T.OK] * 6 + [T.NOT_IN_CENSUS] * 2
            assert cr == frozen and sr == stree.root
            assert flat[6 * blk:] == b'\0' * 2 * blk
            with fresh_tree(ctx, frozen_set, nl) as f:
                f2, cr2, sr2, st2 = census.census_inputs_from_trees(ctx, f, stree, *args)
            assert (f2, cr2, sr2, st2) == (flat, cr, sr, st)
            for j in range(6):
                assert flat[blk * j + 32 * 7:blk * j + 32 * 8] == W(frozen)
            ws, wst = ctx.witness([flat[blk * j:blk * (j + 1)] for j in range(6)], nl)
            assert wst == [0] * 6
            # the live census: the deleted voter is gone, the late voter is in, the updated weight is the new one
            _, _, _, st3 = census.census_inputs_from_trees(ctx, ct, stree, *args)
            assert st3 == [T.NOT_IN_CENSUS] + [T.OK] * 7
            assert ct.get([address[1]])[0] == [77] and snap.get([address[1]])[0] == [avail[1]]


def test_sharing_not_copying(ctx):
    """A 2^16-voter tree holding a snapshot through 256 adds, 256 updates and 256 deletes grows by at most 768 x (max depth + 2) references, far below its own count; after
    the release it holds exactly the references of a tree built fresh from its set.  30 cycles of snapshot / constant-size churn / release keep the allocated references
    within the first cycle's growth twice over: released references are reused, not leaked."""
    from zkcensus_amd import census
    rng = random.Random(1 << 16)
    nl, n = 160, 1 << 16
    ks = tree_keys(rng, nl, n + 256 + 256 * 31)
    pool = ks[n:]; ks = ks[:n]
    kv = {k: rng.randrange(ol.R) for k in ks}
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * n
        live0, _ = tree.refs()
        with tree.snapshot() as snap:
            new = pool[:256]; pool = pool[256:]
            run_batch(tree, kv, 'add', new, [rng.randrange(ol.R) for _ in new], nl)
            run_batch(tree, kv, 'update', rng.sample(ks, 256), [rng.randrange(ol.R) for _ in range(256)], nl)
            run_batch(tree, kv, 'delete', rng.sample(list(kv), 256), None, nl)
            live1, _ = tree.refs()
            maxdep = max(depths(tree, list(kv)))
            assert 0 < live1 - live0 <= 768 * (maxdep + 2), (live0, live1, maxdep)
            assert live1 - live0 < live0 // 4
        with fresh_tree(ctx, kv, nl) as f:
            assert tree.refs()[0] == f.refs()[0]
        assert tree.root == census.smt_build(ctx, list(kv), list(kv.values()), nl, siblings=False)[0]
    # churn cycles on a tree with no free references yet, so that the first cycle's growth is what a cycle needs
    kv = {k: rng.randrange(ol.R) for k in ks}
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * n
        _, alloc0 = tree.refs()
        growth = None
        for c in range(30):
            with tree.snapshot() as snap:
                root = snap.root
                new = pool[:256]; pool = pool[256:]
                run_batch(tree, kv, 'delete', rng.sample(list(kv), 256), None, nl)
                run_batch(tree, kv, 'add', new, [rng.randrange(ol.R) for _ in new], nl)
                assert snap.root == root and len(snap) == n and len(tree) == n
            if growth is None:
                growth = tree.refs()[1] - alloc0
                assert growth > 0
        assert tree.refs()[1] <= alloc0 + 2 * growth, (alloc0, growth, tree.refs())
        with fresh_tree(ctx, kv, nl) as f:
            assert tree.refs()[0] == f.refs()[0]
        assert tree.root == census.smt_build(ctx, list(kv), list(kv.values()), nl, siblings=False)[0]


def test_release_in_any_order(ctx):
    """Five snapshots taken across changes (one of them a snapshot of a snapshot) and released in shuffled order: after each release the rest and the live tree still
    equal their rebuilds; after the last, the tree holds a fresh tree's references."""
    from zkcensus_amd import census
    rng = random.Random(5)
    nl = 160
    ks = tree_keys(rng, nl, 2048 + 5 * 200 + 20)
    pool = ks[2048:]; ks = ks[:2048]
    kv = {k: rng.randrange(ol.R) for k in ks}
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * len(kv)
        snaps = []
        for i in range(5):
            snaps.append((tree.snapshot() if i != 3 else snaps[1][0].snapshot(), dict(kv) if i != 3 else snaps[1][1]))
            new = pool[:200]; pool = pool[200:]
            run_batch(tree, kv, 'add', new, [rng.randrange(ol.R) for _ in new], nl)
            run_batch(tree, kv, 'update', rng.sample(list(kv), 100), [rng.randrange(ol.R) for _ in range(100)], nl)
            run_batch(tree, kv, 'delete', rng.sample(list(kv), 150), None, nl)
        rng.shuffle(snaps)
        while snaps:
            s, _ = snaps.pop()
            s.close()
            assert tree.snapshot_count() == len(snaps)
            for s2, skv in snaps:
                equals_rebuild(ctx, s2, skv, nl, pool[:20])
            equals_rebuild(ctx, tree, kv, nl, pool[:20])
        with fresh_tree(ctx, kv, nl) as f:
            assert tree.refs()[0] == f.refs()[0]


def test_refusals_and_lifetime(ctx):
    """Changes on a snapshot are refused before anything is touched; a snapshot of a snapshot has its root and outlives it; snapshot_count follows every handle;
    freeing the live tree first leaves its snapshots working; census_inputs over a census snapshot and the live tree of the same store returns instead of blocking."""
    from zkcensus_amd import census, ZkcError
    T = census.CensusTree
    rng = random.Random(55)
    nl = 160
    ks = tree_keys(rng, nl, 600)
    kv = {k: rng.randrange(1, 1000) for k in ks[:500]}
    tree = census.CensusTree(ctx, nl)
    assert tree.add(list(kv), list(kv.values())) == [0] * 500
    assert tree.snapshot_count() == 0
    s1 = tree.snapshot()
    frozen, frozen_kv = tree.root, dict(kv)
    assert s1.is_snapshot and s1.root == frozen and len(s1) == 500 and tree.snapshot_count() == s1.snapshot_count() == 1
    lib = tree._lib
    st = (ctypes.c_int32 * 1)(77)
    assert lib.zkc_tree_add(s1._h, W(ks[550]), W(1), 1, st) == ZKC_ERR_BAD_ARG and list(st) == [77]
    assert lib.zkc_tree_update(s1._h, W(ks[0]), W(1), 1, st) == ZKC_ERR_BAD_ARG and list(st) == [77]
    assert lib.zkc_tree_delete(s1._h, W(ks[0]), 1, st) == ZKC_ERR_BAD_ARG and list(st) == [77]
    with pytest.raises(ZkcError) as e:
        s1.add([ks[550]], [1])
    assert e.value.code == ZKC_ERR_BAD_ARG
    assert s1.root == tree.root == frozen and len(tree) == 500
    # null outputs on real handles: refused, nothing written
    assert lib.zkc_tree_snapshot(tree._h, None) == ZKC_ERR_BAD_ARG and lib.zkc_tree_snapshot_count(s1._h, None) == ZKC_ERR_BAD_ARG
    assert tree.snapshot_count() == 1
    # the live tree changes; a snapshot of the snapshot has the frozen root and outlives the first
    assert tree.add(ks[500:550], [5] * 50) == [0] * 50 and tree.delete(ks[:20]) == [0] * 20
    kv.update(dict.fromkeys(ks[500:550], 5))
    for k in ks[:20]:
        del kv[k]
    s2 = s1.snapshot()
    assert s2.root == frozen and tree.snapshot_count() == 2
    s1.close()
    assert s2.snapshot_count() == 1
    equals_rebuild(ctx, s2, frozen_kv, nl, ks[500:560])
    s3 = tree.snapshot()
    assert tree.snapshot_count() == 2
    # census_inputs: the census snapshot and the live tree of the same store (the live tree as the SIK tree: its values are no SIKs, so SIK_MISMATCH) in a thread
    out = {}

    def call():
        out['r'] = census.census_inputs_from_trees(ctx, s2, tree, [1, 2], [ks[0], ks[30], ks[520]], [1] * 3, [1] * 3, [1] * 3, [[1, 2]] * 3)
    th = threading.Thread(target=call, daemon=True)
    th.start(); th.join(120)
    assert not th.is_alive(), 'census_inputs over two handles of one store blocked'
    assert out['r'][3] == [T.NOT_IN_SIK, T.SIK_MISMATCH, T.NOT_IN_CENSUS] and out['r'][1] == frozen
    # the live tree freed first: both snapshots keep working and still count each other
    tree.close()
    assert s2.snapshot_count() == 2
    equals_rebuild(ctx, s2, frozen_kv, nl, ks[500:560])
    equals_rebuild(ctx, s3, kv, nl, ks[:20])
    s3.close()
    assert s2.snapshot_count() == 1
    equals_rebuild(ctx, s2, frozen_kv, nl)
    s2.close()


def test_two_to_the_17_snapshot_keys(ctx):
    """A 2^17-voter snapshot (nLevels 40, so the host buffers stay small) through 4 096 changes to the live tree: gen_proof of every snapshot key equals a rebuild of
    the snapshot's set, and the live tree equals a rebuild of its own."""
    from zkcensus_amd import census
    rng = random.Random(17)
    nl, n = 40, 1 << 17
    ks = tree_keys(rng, nl, n + 1366)
    new = ks[n:]; ks = ks[:n]
    vs = [rng.randrange(ol.R) for _ in ks]
    kv = dict(zip(ks, vs))
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks, vs) == [0] * n
        with tree.snapshot() as snap:
            frozen = dict(kv)
            run_batch(tree, kv, 'add', new, [rng.randrange(ol.R) for _ in new], nl)
            run_batch(tree, kv, 'update', rng.sample(ks, 1365), [rng.randrange(ol.R) for _ in range(1365)], nl)
            run_batch(tree, kv, 'delete', rng.sample(ks, 1365), None, nl)
            assert len(kv) == n + 1
            root, sib, dep = census.smt_build(ctx, ks, vs, nl)
            r, s, d, ex = snap.gen_proof(ks)
            assert r == root == snap.root and all(ex) and d == dep and s == sib
            assert snap.get(ks)[0] == vs and len(snap) == n and frozen == dict(zip(ks, vs))
        live = list(kv)
        root, sib, dep = census.smt_build(ctx, live, [kv[k] for k in live], nl)
        r, s, d, ex = tree.gen_proof(live)
        assert r == root and all(ex) and d == dep and s == sib
