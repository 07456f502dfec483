"""GPU: the census kernels by value against a GPU-free model (tests/arbo_model.py: arbo's tree in plain Python over the oracle's Poseidon) -- zkc_poseidon_batch,
zkc_smt_build, zkc_census_inputs, the resident zkc_tree_*, zkc_smt_check_proofs and zkc_smt_check_absence.  The older census tests hold the resident tree against
zkc_smt_build, which hashes with the same kernels, and climb paths, which proves a path self-consistent and not that the tree has arbo's shape.  Here the model says
what the root, every sibling list and every absence proof of a key set must be: at every nLevels edge from 1 to 253, on chains up to 253 nodes long, at 63 / 64 / 65
nodes on a depth (the narrow / wide launch split of zkc_hash_levels), at value edges of the hash, and at every depth of the checkers.  Every comparison is exact."""
import random
import pytest
import oracle_lib as ol
import arbo_model as am
from census_lib import words, VALID, ROOT_MISMATCH, model_voters, oracle_verdict, sib_list
from edge_voters import ADDRESSES

pytestmark = pytest.mark.gpu
R = ol.R
A2, A1 = int('10' * 127, 2), int('01' * 127, 2)                   # 0x2aaa...a and 0x1555...5 (edge_voters.ADDRESSES): each path bit taken both ways between them
assert ('addr_1010', A2) in ADDRESSES and ('addr_0101', A1) in ADDRESSES and A2 < R


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


# ---- a. the hash by value ----
HASH_VALUES = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 29) - 1, 1 << 29, 1 << 58, (1 << 232) - 1, 1 << 232, (1 << 253) - 1, 1 << 253,
               sum(((1 << 29) - 1) << (29 * i) for i in range(9)) % R,          # nine 29-bit limbs of all ones, reduced
               A2, A1]
UNREDUCED = [R, R + 1, 2 * R + 1, 1 << 254, 1 << 255, (1 << 256) - 1]


def hash_rows(width, values, rng):
    """width 2: every pair; wider: each value in each position, the other inputs random"""
    if width == 2:
        return [(a, b) for a in values for b in values]
    rows = []
    for pos in range(width):
        for v in values:
            row = [rng.randrange(R) for _ in range(width)]; row[pos] = v
            rows.append(tuple(row))
    return rows


@pytest.mark.parametrize('width', [2, 3, 4])
def test_poseidon_batch_by_value(ctx, width):
    """zkc_poseidon_batch against the oracle over the value list (limb boundaries of the 29-bit form, both ends of the field, alternating bits), and in batches of
    1, 63, 64, 65 and 1 000 rows (one lane per hash, 64 lanes per workgroup)"""
    from zkcensus_amd import census
    rng = random.Random(width)
    assert len(HASH_VALUES) == 17 and all(0 <= v < R for v in HASH_VALUES)
    rows = hash_rows(width, HASH_VALUES, rng)
    assert len(rows) == (289 if width == 2 else 17 * width)
    assert census.poseidon_batch(ctx, rows) == [ol.poseidon(list(r)) for r in rows]
    ran = 0
    for n in (1, 63, 64, 65, 1000):
        rows = [tuple(rng.randrange(R) for _ in range(width)) for _ in range(n)]
        got = census.poseidon_batch(ctx, rows)
        assert len(got) == n and got == ol.pmap(lambda r: ol.poseidon(list(r)), rows), n
        ran += n
    assert ran == 1193


@pytest.mark.parametrize('width', [2, 3, 4])
def test_poseidon_batch_hashes_the_residue_of_an_unreduced_word(ctx, width):
    """zkc_poseidon_batch is the one census entry point that does not refuse a word at or above r: like the oracle it hashes the residue (include/zkcensus.h)"""
    from zkcensus_amd import census
    rng = random.Random(100 + width)
    rows = hash_rows(width, UNREDUCED, rng) if width > 2 else [(a, b) for a in UNREDUCED + [3] for b in UNREDUCED + [5]][:-1]
    assert len(rows) == (48 if width == 2 else 6 * width) and all(max(r) >= R for r in rows)
    want = [ol.poseidon(list(r)) for r in rows]
    assert want == [ol.poseidon([x % R for x in r]) for r in rows]              # the oracle hashes the residue
    assert census.poseidon_batch(ctx, rows) == want


def census_voters(nl, c):
    """voters of election c (0..5) for zkc_census_inputs at nl: edge addresses whose low nl bits are distinct (most of the list ends in all zeros or all ones, so each
    election starts at another place in it and all twelve get their turn), passwords / signatures / election ids from {0, 1, r - 1}"""
    E = [0, 1, R - 1]
    address, seen = [], set()
    start = [0, 2, 4, 6, 8, 11][c]
    for _, a in ADDRESSES[start:] + ADDRESSES[:start]:
        if a & ((1 << nl) - 1) not in seen:
            seen.add(a & ((1 << nl) - 1)); address.append(a)
    n = len(address)
    eid = (E[c % 3], E[(c + 2 + c // 3) % 3])
    password = [E[(i + c) % 3] for i in range(n)]; signature = [E[(i // 3 + i + 2 * c) % 3] for i in range(n)]
    vh = [(i, R - 1 - i) for i in range(n)]
    return eid, address, password, signature, vh


@pytest.mark.parametrize('nl', [3, 10])
def test_census_inputs_by_value(ctx, nl):
    """zkc_census_inputs at the smallest nLevels it takes and at 10: the SIK and nullifier words equal the oracle's, both roots and both sibling lists the model's, whole
    blocks byte for byte; at nLevels 10 the circuit (the oracle's witness generator) accepts each block"""
    from zkcensus_amd import census
    ran, combos, used = 0, set(), set()
    for c in range(6):
        eid, address, password, signature, vh = census_voters(nl, c)
        n = len(address)
        assert n >= 5
        used |= set(address)
        combos |= {(password[i], signature[i], eid) for i in range(n)}
        flat, croot, sroot = census.census_inputs(ctx, eid, address, password, signature, [1] * n, [1] * n, vh, nl)
        want = model_voters(eid, address, password, signature, [1] * n, [1] * n, vh, nl)
        nIn = 12 + 2 * (nl + 1)
        assert len(flat) == 32 * nIn * n
        fv = census.FlatVoters(flat, nl)
        for i in range(n):
            got = fv[i]
            assert got['nullifier'] == str(ol.poseidon([signature[i], password[i], eid[0], eid[1]])), (c, i)
            assert got == want[i], (c, i)
            assert flat[32 * nIn * i:32 * nIn * (i + 1)] == ol.flat_inputs(want[i], nl), (c, i)
            if nl == 10:
                assert ol.witness(flat[32 * nIn * i:32 * nIn * (i + 1)], nl)[0] == 0, (c, i)
            ran += 1
        sik = [ol.poseidon([a, p, s]) for a, p, s in zip(address, password, signature)]
        assert (croot, sroot) == (am.root(dict(zip(address, [1] * n)), nl), am.root(dict(zip(address, sik)), nl))
        # the SIK tree's values are the SIK words: its proofs hold them
        assert census.check_proofs(ctx, address, sik, b''.join(words(int(x) for x in v['sikSiblings']) for v in want), sroot, nl) == [VALID] * n
    assert ran >= 30 and used == {a for _, a in ADDRESSES} and len({(p, s) for p, s, _ in combos}) == 9 and len({e for _, _, e in combos}) == 6


# ---- what the tree tests share ----
def sib_bytes(kv, nl, keys):
    return b''.join(words(am.proof(kv, nl, k)[0]) for k in keys)


def assert_build_is_model(ctx, kv, nl):
    """zkc_smt_build over kv: root, sibling bytes and depths are the model's"""
    from zkcensus_amd import census
    ks = list(kv)
    root, sib, dep = census.smt_build(ctx, ks, [kv[k] for k in ks], nl)
    assert root == am.root(kv, nl)
    assert dep == [am.proof(kv, nl, k)[1] for k in ks]
    assert sib == sib_bytes(kv, nl, ks)


def assert_tree_is_model(tree, kv, nl, absent=()):
    """a resident tree holding kv: root, size, every key's siblings / depth / value are the model's; the keys of `absent` are absent, and their absence proofs are the
    model's.  Returns the number of proofs compared."""
    ks = list(kv); absent = list(absent)
    assert not set(absent) & set(ks)
    assert tree.root == am.root(kv, nl) and len(tree) == len(ks)
    if not ks and not absent:
        return 0
    r, sib, dep, ex = tree.gen_proof(ks + absent)
    assert r == am.root(kv, nl)
    assert ex == [True] * len(ks) + [False] * len(absent)
    assert dep == [am.proof(kv, nl, k)[1] for k in ks] + [0] * len(absent)
    assert sib == sib_bytes(kv, nl, ks + absent)
    assert tree.get(ks + absent) == ([kv[k] for k in ks] + [0] * len(absent), [True] * len(ks) + [False] * len(absent))
    if absent:
        r, sib, dep, ok, ov, o0, st = tree.gen_absence_proof(absent)
        want = [am.absence_proof(kv, nl, k) for k in absent]
        assert st == [0] * len(absent) and r == am.root(kv, nl)
        assert (dep, ok, ov, o0) == ([w[1] for w in want], [w[2] for w in want], [w[3] for w in want], [w[4] for w in want])
        assert sib == b''.join(words(w[0]) for w in want)
    return len(ks) + len(absent)


# ---- b. nLevels edges ----
LEVELS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 160, 161, 192, 193, 252, 253]


def level_edge_set(nl, rng):
    """(kv, absent): about 40 keys (fewer where 2^nl is small) -- 0, 1, 2^nl - 1, r - 1, r - 2 where they do not collide on the first nl bits; pairs parting at bits 0,
    nl // 2 and nl - 1; a key with every bit from nl to 252 set; the rest random -- with values from {0, 1, r - 1, random}, key 0 holding value 0; and 10 absent keys
    (fewer where 2^nl is small), the first a twin of key 0 that differs only above nl, the rest drawn so that both is_old0 kinds occur where the tree has an empty child.
    At nl >= 2 no key has low bits 10, so that such a child exists from nl = 3 on."""
    mask = (1 << nl) - 1
    kv, low = {}, set()

    def put(k, v=None):
        if 0 <= k < R and k & mask not in low and not (nl >= 2 and k & 3 == 2):
            low.add(k & mask)
            kv[k] = rng.choice([0, 1, R - 1, rng.randrange(R)]) if v is None else v
            return True
        return False
    put(0, 0); put(1); put(mask); put(R - 1); put(R - 2)
    for b in (0, nl // 2, nl - 1):
        for _ in range(40):                                                      # a pair sharing its low b bits, parting at bit b, random above
            k0 = rng.getrandbits(253) & ~(1 << b); k1 = (k0 & ((1 << b) - 1)) | (1 << b) | (rng.getrandbits(253) >> (b + 1) << (b + 1))
            free = lambda k: k & mask not in low and not (nl >= 2 and k & 3 == 2)
            if free(k0) and free(k1) and (k0 ^ k1) & mask:
                put(k0); put(k1)
                break
    put(((1 << 253) - (1 << nl)) | rng.getrandbits(nl))
    room = min(40, (1 << nl) - (1 << (nl - 2)) if nl >= 2 else 2)
    for _ in range(4000):
        if len(kv) >= room:
            break
        put(rng.getrandbits(253))
    twin = 1 << (nl if nl < 253 else 253)
    assert twin < R and twin not in kv and 0 in kv
    absent, kinds = [twin], [0, 0]
    kinds[am.absence_proof(kv, nl, twin)[4]] += 1
    for _ in range(400):
        k = rng.getrandbits(253) if rng.random() < 0.5 else (rng.getrandbits(253) & ~3) | 2
        if k in kv or k in absent or len(absent) >= 10:
            continue
        o0 = am.absence_proof(kv, nl, k)[4]
        if kinds[o0] < 5:
            kinds[o0] += 1; absent.append(k)
    return kv, absent, kinds


@pytest.mark.parametrize('nl', LEVELS)
def test_level_edges(ctx, nl):
    """Every nLevels at which a word or launch boundary of the tree code lies, and both ends of the range: zkc_smt_build, a tree filled in one add, trees grown key by
    key in insertion order and in reverse, absence proofs, and the tree after a third of the keys is deleted -- all equal to the model; a colliding key changes nothing."""
    from zkcensus_amd import census
    rng = random.Random(1000 + nl)
    kv, absent, kinds = level_edge_set(nl, rng)
    n = len(kv)
    assert n == (2 if nl == 1 else 3 if nl == 2 else 6 if nl == 3 else 40) and kv[0] == 0
    assert len(absent) == 10 or nl < 3
    if nl >= 3:
        assert min(kinds) > 0, kinds
    if nl >= 31:
        per = am.inner_nodes_per_depth(kv, nl)
        assert per[nl - 1] >= 1 and per[nl // 2] >= 1 and len(per) == nl              # the pair parting at the last level is there, below a chain
    assert_build_is_model(ctx, kv, nl)
    ran = 0
    ks = list(kv)
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks, [kv[k] for k in ks]) == [0] * n
        ran += assert_tree_is_model(tree, kv, nl, absent)
        # a key that agrees with a present one on the first nl bits
        twin = absent[0]
        assert tree.add([twin], [5]) == [census.CensusTree.COLLISION]
        assert_tree_is_model(tree, kv, nl, absent[:1])
        gone = rng.sample(ks, max(1, n // 3))
        assert tree.delete(gone) == [0] * len(gone)
        left = {k: v for k, v in kv.items() if k not in gone}
        ran += assert_tree_is_model(tree, left, nl, gone + absent)
        if left:
            assert_build_is_model(ctx, left, nl)
    for order in (ks, ks[::-1]):
        with census.CensusTree(ctx, nl) as tree:
            part = {}
            for k in order:
                assert tree.add([k], [kv[k]]) == [0]
                part[k] = kv[k]
                assert tree.root == am.root(part, nl), len(part)
            ran += assert_tree_is_model(tree, kv, nl, absent)
    assert ran == 3 * (n + len(absent)) + (n - len(gone)) + len(gone) + len(absent)


# ---- c. long chains at nLevels 253 ----
CHAIN_BITS = [0, 28, 29, 31, 32, 63, 64, 127, 128, 159, 160, 191, 192, 223, 224, 251, 252]


def chain_keys(b, rng):
    """two keys sharing their low b bits and parting at bit b, and (b >= 2) a third that shares b // 2 bits with them and leaves the chain there; all below 2^253"""
    low = rng.getrandbits(b) if b else 0
    k0 = low | (rng.getrandbits(252 - b) << (b + 1) if b < 252 else 0); k1 = low | (1 << b) | (rng.getrandbits(252 - b) << (b + 1) if b < 252 else 0)
    if b < 2:
        return k0, k1, None
    h = b // 2
    third = ((low ^ (1 << h)) & ((1 << (h + 1)) - 1)) | (rng.getrandbits(252 - h) << (h + 1))
    return k0, k1, third


def chain_trees(b):
    """the trees of one chain case, in the order the resident tree passes through them: the pair, with the third key, after deleting one of the pair"""
    rng = random.Random(2000 + b)
    k0, k1, third = chain_keys(b, rng)
    v = lambda: rng.choice([0, 1, R - 1, rng.randrange(R)])
    pair = {k0: v(), k1: v()}
    if third is None:
        return [pair, None, {k1: pair[k1]}], k0
    full = dict(pair); full[third] = v()
    gone = (k0, k1)[b & 1]
    return [pair, full, {k: x for k, x in full.items() if k != gone}], gone


@pytest.fixture(scope='module')
def chain_proofs():
    """every membership proof and absence proofs of both kinds of every chain tree, each once as it is and once with the value off by one: (absence?, key, value,
    siblings, root, old key, is_old0); and the oracle's verdict of each (census_lib.oracle_verdict, on host threads)"""
    nl = 253
    cases = []
    for b in CHAIN_BITS:
        rng = random.Random(3000 + b)
        for kv in chain_trees(b)[0]:
            if kv is None:
                continue
            rt = am.root(kv, nl)
            for k, v in kv.items():
                s = am.proof(kv, nl, k)[0]
                cases += [(False, k, v, s, rt, None, 0), (False, k, (v + 1) % R, s, rt, None, 0)]
            kinds = [0, 0]
            for k in [next(iter(kv)) ^ (1 << 253)] + [next(iter(kv)) ^ (1 << rng.randrange(b + 1)) for _ in range(6)] + [rng.getrandbits(253) for _ in range(4)]:
                if k in kv or k >= R:
                    continue
                s, d, okey, oval, o0 = am.absence_proof(kv, nl, k)
                if kinds[o0] < 1:
                    kinds[o0] += 1
                    cases += [(True, k, oval, s, rt, okey, o0), (True, k, (oval + 1) % R, s, rt, okey, o0)]
    want = ol.pmap(lambda c: oracle_verdict(c[1], c[2], c[3], c[4], nl, c[5] if c[0] else None, c[6]), cases)
    return cases, want


@pytest.mark.parametrize('b', CHAIN_BITS)
def test_long_chains(ctx, b):
    """nLevels 253: a chain of b one-child nodes above two leaves (key words 0 .. 7, a zkc_tree_narrow run of up to 253 depths), through zkc_smt_build and through a
    resident tree -- the pair, then a third key leaving the chain half way, then one of the pair deleted, which lifts the other: each state equals the model"""
    from zkcensus_amd import census
    nl = 253
    (pair, full, left), gone = chain_trees(b)
    k0, k1 = list(pair)
    assert am.inner_nodes_per_depth(pair, nl) == [1] * (b + 1) + [0] * (nl - b - 1)
    assert [am.proof(pair, nl, k)[1] for k in pair] == [b + 1, b + 1]
    held = set(pair) | set(full or ())
    absent = [k for k in dict.fromkeys((k0 ^ (1 << 253), k1 ^ (1 << 253), k0 ^ 1, k0 ^ (1 << b) ^ (1 << 200), k1 ^ (1 << (b // 2)), 12345)) if k < R and k not in held]
    assert len(absent) >= 4
    ran = 0
    for kv in (pair, full, left):
        if kv is not None:
            assert_build_is_model(ctx, kv, nl)
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add([k0, k1], [pair[k0], pair[k1]]) == [0, 0]
        ran += assert_tree_is_model(tree, pair, nl, absent)
        if full is not None:
            third = list(full)[2]
            assert am.proof(full, nl, third)[1] == b // 2 + 1 and am.proof(full, nl, k0)[1] == b + 1
            assert tree.add([third], [full[third]]) == [0]
            ran += assert_tree_is_model(tree, full, nl, absent)
        assert tree.delete([gone]) == [0]
        survivor = k1 if gone == k0 else k0
        assert am.proof(left, nl, survivor)[1] == (0 if full is None else b // 2 + 1)           # lifted from b + 1 levels down
        ran += assert_tree_is_model(tree, left, nl, absent + [gone])
    assert ran == (2 + len(absent)) + (0 if full is None else 3 + len(absent)) + len(left) + len(absent) + 1


def run_checker(ctx, cases, nl, how):
    """the verdicts of check_proofs / check_absence over `cases` (chain_proofs' layout), membership and absence proofs each in their own calls: how = 'lane' -- one batch
    of more than 64, padded with repeats; 'wave' -- batches of at most 64; 'single' -- one proof per call"""
    from zkcensus_amd import census
    out = [None] * len(cases)
    for absence in (False, True):
        idx = [i for i, c in enumerate(cases) if c[0] == absence]
        if not idx:
            continue
        if how == 'lane':
            batches = [idx + [idx[i % len(idx)] for i in range(max(0, 65 - len(idx)))]]
            assert len(batches[0]) > 64
        else:
            step = 64 if how == 'wave' else 1
            batches = [idx[lo:lo + step] for lo in range(0, len(idx), step)]
        for bt in batches:
            cs = [cases[i] for i in bt]
            sibs = b''.join(words(c[3]) for c in cs)
            if absence:
                got = census.check_absence(ctx, [c[1] for c in cs], [c[5] for c in cs], [c[2] for c in cs], [c[6] for c in cs], sibs, [c[4] for c in cs], nl)
            else:
                got = census.check_proofs(ctx, [c[1] for c in cs], [c[2] for c in cs], sibs, [c[4] for c in cs], nl)
            assert len(got) == len(bt)
            for i, g in zip(bt, got):
                assert out[i] in (None, g)
                out[i] = g
    return out


@pytest.mark.parametrize('how', ['lane', 'wave', 'single'])
def test_checkers_on_the_chain_proofs(ctx, chain_proofs, how):
    """every proof and absence proof of the chain trees, and each with its value off by one, in one batch (a lane per proof), in batches of at most 64 (a wave per
    proof) and singly: the verdicts are the oracle's for every one"""
    cases, want = chain_proofs
    assert sum(not c[0] for c in cases) == 2 * (16 * 7 + 3) and sum(c[0] for c in cases) >= 2 * (16 * 3 + 2)        # 7 membership proofs per chain (3 at b = 0), an absence proof per tree at least
    assert {VALID, ROOT_MISMATCH} == set(want) and want.count(VALID) >= len(want) // 2
    assert any(c[0] and c[6] for c in cases) and any(c[0] and not c[6] for c in cases)
    assert run_checker(ctx, cases, 253, how) == want


# ---- d. every depth in the checkers, nLevels 253 ----
@pytest.fixture(scope='module')
def depth_proofs():
    """one membership proof and two absence proofs (is_old0 0 and 1) per depth 0 .. 253 at nLevels 253, keys random below r or (every second depth) 0x2aaa... / 0x1555...,
    siblings random and non-zero below the depth, roots climbed with the oracle's Poseidon, a third of them then made wrong"""
    nl = 253
    rng = random.Random(253)
    cases = []
    for d in range(nl + 1):
        for kind in range(3):                                                    # 0: membership, 1: absence at a leaf, 2: absence at an empty child
            for _ in range(200):
                key = (A2, A1)[(d >> 1) & 1] if d & 1 else rng.randrange(R)
                okey = key ^ (1 << rng.randrange(d, 254)) if kind == 1 else 0 if kind == 2 else None
                if okey is None or okey < R:
                    break
            assert okey is None or okey < R
            val = 0 if kind == 2 else rng.randrange(R)
            s = [rng.randrange(1, R) if l < d else 0 for l in range(nl + 1)]
            cases.append([kind != 0, key, val, s, None, okey, int(kind == 2), rng.random() < 1 / 3])

    def climb(c):
        cur = 0 if c[6] else ol.poseidon([c[5] if c[0] else c[1], c[2], 1])
        for l in range(len([x for x in c[3] if x]) - 1, -1, -1):
            cur = ol.poseidon([c[3][l], cur]) if (c[1] >> l) & 1 else ol.poseidon([cur, c[3][l]])
        return cur
    roots = ol.pmap(climb, cases)
    want = []
    for c, rt in zip(cases, roots):
        c[4] = (rt + 1) % R if c[7] else rt
        want.append(ROOT_MISMATCH if c[7] else VALID)
    return [tuple(c[:7]) for c in cases], want


@pytest.mark.parametrize('how', ['lane', 'wave'])
def test_every_depth_to_253(ctx, depth_proofs, how):
    """membership and both kinds of absence at every depth 0 .. 253 (the path bits of key words 5 .. 7, which nLevels 160 never reads), as one batch and in waves"""
    cases, want = depth_proofs
    assert len(cases) == 3 * 254 and [sum(1 for c in cases if c[0] == a and c[6] == o) for a, o in ((False, 0), (True, 0), (True, 1))] == [254] * 3
    assert sorted({len([x for x in c[3] if x]) for c in cases}) == list(range(254))
    assert 200 < want.count(ROOT_MISMATCH) < 310
    assert run_checker(ctx, cases, 253, how) == want
    if how == 'lane':                                                            # the model's own reading of the same proofs, on a sample (the full list is by construction)
        for i in random.Random(7).sample(range(len(cases)), 12):
            c = cases[i]
            assert oracle_verdict(c[1], c[2], c[3], c[4], 253, c[5] if c[0] else None, c[6]) == want[i]


# ---- e. the narrow / wide boundary of zkc_hash_levels ----
def boundary_set(m, rng):
    """nLevels 9: every seven-bit prefix once (bits 7, 8 clear, random bits above bit 9), and for m of the prefixes a second key with bit 7 set: 64 nodes at depth 6,
    m at depth 7"""
    kv = {p | (rng.getrandbits(200) << 10): rng.randrange(R) for p in range(128)}
    second = rng.sample(range(128), m)
    kv.update({p | (1 << 7) | (rng.getrandbits(200) << 10): rng.randrange(R) for p in second})
    return kv, second


@pytest.mark.parametrize('m', [63, 64, 65])
def test_narrow_wide_boundary(ctx, m):
    """A depth with 64 nodes is hashed with the narrow run, one with 65 by the level kernel (and then lies below narrow depths): zkc_smt_build and a tree filled in one
    add equal the model, root and every proof"""
    from zkcensus_amd import census
    nl = 9
    kv, _ = boundary_set(m, random.Random(m))
    assert am.inner_nodes_per_depth(kv, nl) == [1, 2, 4, 8, 16, 32, 64, m, 0]
    assert_build_is_model(ctx, kv, nl)
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * len(kv)
        assert assert_tree_is_model(tree, kv, nl, [0x200 | 5 | (1 << 100)]) == 128 + m + 1


def test_dirty_nodes_on_the_boundary(ctx):
    """On a resident tree with 65 nodes at depth 7: batches that update one leaf under each of 63, 64 and 65 of them dirty exactly that many nodes at depth 7 (and at
    most 64 on every depth above); the root is the model's after each"""
    from zkcensus_amd import census
    nl = 9
    rng = random.Random(765)
    kv, second = boundary_set(65, rng)
    by_low = {k & 0x7f: k for k in kv if not k & 0x80}
    ran = 0
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * len(kv)
        for m in (63, 64, 65, 64):
            ks = [by_low[p] for p in rng.sample(second, m)]
            assert len({k & 0x7f for k in ks}) == m                                # m distinct depth-7 nodes
            vs = [rng.randrange(R) for _ in ks]
            assert tree.update(ks, vs) == [0] * m
            kv.update(zip(ks, vs))
            assert tree.root == am.root(kv, nl), m
            ran += 1
        assert assert_tree_is_model(tree, kv, nl) == 193
    assert ran == 4


def between_set(rng):
    """nLevels 32, 200 keys sharing a 20-bit prefix: all 128 seven-bit continuations (bits 20 .. 26), a second key with bit 27 set under 65 of them, and 7 keys that
    part from a first key only at bit 30 -- deepest first: three narrow depths, a wide one (65 nodes at depth 27), then 27 narrow ones"""
    pre = rng.getrandbits(20)
    first = {c: pre | (c << 20) | (rng.getrandbits(4) << 28) | (rng.getrandbits(200) << 32) for c in range(128)}
    kv = {k: rng.randrange(R) for k in first.values()}
    picks = rng.sample(range(128), 72)
    for c in picks[:65]:
        kv[pre | (c << 20) | (1 << 27) | (rng.getrandbits(4) << 28) | (rng.getrandbits(200) << 32)] = rng.randrange(R)
    for c in picks[65:]:                                                          # under continuations without a second key: the first key's subtree starts at depth 27
        kv[(first[c] & ((1 << 30) - 1)) | ((~first[c]) & (1 << 30)) | (rng.getrandbits(201) << 31)] = rng.randrange(R)
    return kv


def test_wide_depth_between_narrow_runs(ctx):
    from zkcensus_amd import census
    nl = 32
    rng = random.Random(3232)
    kv = between_set(rng)
    assert len(kv) == 200
    assert am.inner_nodes_per_depth(kv, nl) == [1] * 20 + [1, 2, 4, 8, 16, 32, 64, 65 + 7, 7, 7, 7, 0]
    assert_build_is_model(ctx, kv, nl)
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(list(kv), list(kv.values())) == [0] * 200
        absent = [rng.getrandbits(253) for _ in range(3)] + [next(iter(kv)) ^ (1 << 31), next(iter(kv)) ^ (1 << 40)]
        assert assert_tree_is_model(tree, kv, nl, absent) == 205
        # one leaf under each of 65 depth-27 nodes updated in one batch: a wide dirty depth between narrow ones
        deep = [k for k in kv if am.proof(kv, nl, k)[1] >= 28]
        under = {}
        for k in deep:
            under.setdefault(k & ((1 << 27) - 1), k)
        ks = list(under.values())[:65]
        assert len(ks) == 65
        vs = [rng.randrange(R) for _ in ks]
        assert tree.update(ks, vs) == [0] * 65
        kv.update(zip(ks, vs))
        assert assert_tree_is_model(tree, kv, nl) == 200
