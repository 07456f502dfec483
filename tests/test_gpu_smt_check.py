"""GPU: census proofs checked in batches (census.check_proofs, zkc_smt_check_proofs, csrc/zkc_smt_check.hip) -- arbo CheckProof against any root.  The reference's two
arbo-made paths are valid; every proof zkc_smt_build and the resident tree hand out is valid against their root, with the verdicts of a sample equal to a pure-Python
climb with the oracle's Poseidon; each kind of tampering gets its exact verdict; a proof taken before a census grew holds against the frozen root only; the verdicts
agree with the witness's census-root assert; and they do not depend on how a batch is cut into chunks."""
import ctypes
import os
import random
import pytest
import oracle_lib as ol
from census_lib import words, VALID, ROOT_MISMATCH, NOT_BELOW_R, LAST_SIBLING, oracle_verdict, sib_list, tree_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


def test_reference_paths(ctx):
    """inputs_example.json: the census path (address -> availableWeight under censusRoot) and the SIK path (address -> H(address, password, signature) under sikRoot),
    singly and replicated 1 000 times each, interleaved, one root per proof."""
    from zkcensus_amd import census
    ex = ol.load_json(os.path.join('ref', 'inputs_example.json'))
    nl = 160
    addr = int(ex['address'])
    sik = ol.poseidon([addr, int(ex['password']), int(ex['signature'])])
    csib = words(int(x) for x in ex['censusSiblings']); ssib = words(int(x) for x in ex['sikSiblings'])
    assert len(csib) == len(ssib) == 32 * (nl + 1)
    assert census.check_proofs(ctx, [addr], [int(ex['availableWeight'])], csib, int(ex['censusRoot']), nl) == [VALID]
    assert census.check_proofs(ctx, [addr], [sik], ssib, int(ex['sikRoot']), nl) == [VALID]
    assert census.check_proofs(ctx, [addr], [sik], ssib, int(ex['censusRoot']), nl) == [ROOT_MISMATCH]
    n = 2000
    vals = [int(ex['availableWeight']) if i % 2 == 0 else sik for i in range(n)]
    roots = [int(ex['censusRoot']) if i % 2 == 0 else int(ex['sikRoot']) for i in range(n)]
    sibs = b''.join(csib if i % 2 == 0 else ssib for i in range(n))
    assert census.check_proofs(ctx, [addr] * n, vals, sibs, roots, nl) == [VALID] * n


@pytest.mark.parametrize('nl', [160, 12])
def test_every_proof_of_a_tree_is_valid(ctx, nl):
    """2^17 random keys at nLevels 160; at nLevels 12 (a shallow, crowded tree) 3 000 keys with distinct low 12 bits.  Proofs from zkc_smt_build and from the resident
    tree (checked through CensusTree.check_proofs, against its current root, which it leaves alone): all valid; a seeded sample of 512 agrees with the oracle's climb."""
    from zkcensus_amd import census
    rng = random.Random(nl)
    ks = tree_keys(rng, nl, 1 << 17 if nl == 160 else 3000)
    vs = [rng.randrange(ol.R) for _ in ks]
    kb, vb = words(ks), words(vs)
    n = len(ks)
    root, sib, dep = census.smt_build(ctx, kb, vb, nl)
    assert census.check_proofs(ctx, kb, vb, sib, root, nl) == [VALID] * n
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(kb, vb) == [0] * n
        r, tsib, tdep, ex = tree.gen_proof(kb)
        assert r == root and all(ex)
        assert tree.check_proofs(kb, vb, tsib) == [VALID] * n
        assert tree.root == root and len(tree) == n
    sample = rng.sample(range(n), 512)
    got = census.check_proofs(ctx, [ks[i] for i in sample], [vs[i] for i in sample], b''.join(sib[32 * (nl + 1) * i:32 * (nl + 1) * (i + 1)] for i in sample), root, nl)
    assert got == [oracle_verdict(ks[i], vs[i], sib_list(sib, i, nl), root, nl) for i in sample] == [VALID] * 512


def test_tamper_classes(ctx):
    """Valid proofs and seven kinds of tampered ones in one shuffled batch, one root per proof: each gets its exact verdict, and the oracle agrees on every one."""
    from zkcensus_amd import census
    rng = random.Random(7)
    nl = 160
    ks = tree_keys(rng, nl, 4096); vs = [rng.randrange(1, ol.R - 1) for _ in ks]
    root, sib, dep = census.smt_build(ctx, ks, vs, nl)
    cases = []                                       # (key, value, siblings, root, expected)

    def proof(i):
        return ks[i], vs[i], sib_list(sib, i, nl), root
    idx = [i for i in range(len(ks)) if dep[i] >= 2]
    for c in range(len(idx) // 8 * 8):
        i = idx[c]; k, v, s, r = proof(i); d = dep[i]; kind = c % 9
        if kind == 0:                                # one flipped bit in a sibling below the depth
            l = rng.randrange(d)
            x = s[l] ^ (1 << rng.randrange(250))
            if x >= ol.R or x == 0:
                continue
            s[l] = x; want = ROOT_MISMATCH
        elif kind == 1:
            v += 1; want = ROOT_MISMATCH
        elif kind == 2:                              # one key bit flipped at a level below the depth
            k ^= 1 << rng.randrange(d); want = ROOT_MISMATCH
        elif kind == 3:
            r = (r + 1 + rng.randrange(1000)) % ol.R; want = ROOT_MISMATCH
        elif kind == 4:                              # the last non-zero sibling zeroed: the depth changes
            s[d - 1] = 0; want = ROOT_MISMATCH
        elif kind == 5:
            s[nl] = rng.randrange(1, ol.R); want = LAST_SIBLING
        elif kind == 6:                              # one of key, value, a sibling (below the depth, at the depth, or in slot nLevels), root equal to r
            which = rng.randrange(6)
            if which == 0: k = ol.R
            elif which == 1: v = ol.R
            elif which == 2: s[rng.randrange(d)] = ol.R
            elif which == 3: s[d + 3] = ol.R
            elif which == 4: s[nl] = ol.R
            else: r = ol.R
            want = NOT_BELOW_R
        else:
            want = VALID
        cases.append((k, v, s, r, want))
    rng.shuffle(cases)
    got = census.check_proofs(ctx, [c[0] for c in cases], [c[1] for c in cases], b''.join(words(c[2]) for c in cases), [c[3] for c in cases], nl)
    assert got == [c[4] for c in cases]
    assert {c[4] for c in cases} == {VALID, ROOT_MISMATCH, NOT_BELOW_R, LAST_SIBLING}
    check = rng.sample(range(len(cases)), 300)
    assert [oracle_verdict(*cases[j][:4], nl) for j in check] == [got[j] for j in check]


def test_frozen_root(ctx):
    """Proofs taken before 1 024 voters joined hold against the root the election froze and not against the new one; proofs taken after, the other way round.  One
    call, one root per proof."""
    from zkcensus_amd import census
    rng = random.Random(1024)
    nl = 160
    ks = tree_keys(rng, nl, 5120); vs = [rng.randrange(1, 101) for _ in ks]
    with census.CensusTree(ctx, nl) as tree:
        assert tree.add(ks[:4096], vs[:4096]) == [0] * 4096
        old_keys = rng.sample(ks[:4096], 512)
        old_vals = tree.get(old_keys)[0]
        r0, osib, _, ex = tree.gen_proof(old_keys)
        assert all(ex)
        assert tree.add(ks[4096:], vs[4096:]) == [0] * 1024
        r1, nsib, _, ex = tree.gen_proof(old_keys)
        assert all(ex) and r1 != r0
        assert tree.check_proofs(old_keys, old_vals, osib, r0) == [VALID] * 512
        got = census.check_proofs(ctx, old_keys * 4, old_vals * 4, osib + osib + nsib + nsib, [r0] * 512 + [r1] * 512 + [r0] * 512 + [r1] * 512, nl)
        assert got == [VALID] * 512 + [ROOT_MISMATCH] * 1024 + [VALID] * 512


def synth_proofs(rng, depths, nl):
    """one proof per depth: random key and value, random non-zero siblings below the depth, the root climbed with the oracle's Poseidon"""
    out = []
    for d in depths:
        k, v = rng.getrandbits(250), rng.randrange(ol.R)
        s = [rng.randrange(1, ol.R) for _ in range(d)] + [0] * (nl + 1 - d)
        cur = ol.poseidon([k, v, 1])
        for l in range(d - 1, -1, -1):
            cur = ol.poseidon([s[l], cur]) if (k >> l) & 1 else ol.poseidon([cur, s[l]])
        out.append((k, v, s, cur))
    return out


def test_edges(ctx):
    """n = 0, 1, 64 (the wave-per-proof form), 65 (one lane per proof); a one-leaf tree (depth 0); deep_voters (depth 160, every sibling non-zero, one root per voter);
    depths 0 .. 160 mixed in one batch and in one wave; the argument checks on a real context."""
    from zkcensus_amd import census
    from zkcensus_amd import _native
    rng = random.Random(160)
    nl = 160
    assert census.check_proofs(ctx, [], [], b'', 0, nl) == []
    # a one-leaf tree: depth 0, root = the leaf hash
    root, sib, dep = census.smt_build(ctx, [5], [7], nl)
    assert dep == [0] and root == ol.poseidon([5, 7, 1])
    assert census.check_proofs(ctx, [5], [7], sib, root, nl) == [VALID]
    assert census.check_proofs(ctx, [5, 5, 6], [7, 8, 7], sib * 3, root, nl) == [VALID, ROOT_MISMATCH, ROOT_MISMATCH]
    # every depth 0 .. 160, shuffled, in one batch (lane form) and in waves of 64 (wave form); a tampered copy of each
    ps = synth_proofs(rng, list(range(nl + 1)), nl)
    rng.shuffle(ps)
    tam = [(k, v + 1, s, r) for k, v, s, r in ps]
    allp = ps + tam
    got = census.check_proofs(ctx, [p[0] for p in allp], [p[1] for p in allp], b''.join(words(p[2]) for p in allp), [p[3] for p in allp], nl)
    assert got == [VALID] * len(ps) + [ROOT_MISMATCH] * len(tam)
    for lo in range(0, len(allp), 64):
        part = allp[lo:lo + 64]
        assert census.check_proofs(ctx, [p[0] for p in part], [p[1] for p in part], b''.join(words(p[2]) for p in part), [p[3] for p in part], nl) == got[lo:lo + 64]
    for n in (1, 64, 65):
        part = allp[:n // 2] + allp[len(ps):len(ps) + n - n // 2]
        want = [VALID] * (n // 2) + [ROOT_MISMATCH] * (n - n // 2)
        assert census.check_proofs(ctx, [p[0] for p in part], [p[1] for p in part], b''.join(words(p[2]) for p in part), [p[3] for p in part], nl) == want
    # deep_voters: census and SIK paths 160 levels down, every sibling non-zero
    dv = census.deep_voters(ctx, 48, nl)
    sik = [ol.poseidon([int(v['address']), int(v['password']), int(v['signature'])]) for v in dv]
    keys = [int(v['address']) for v in dv] * 2
    vals = [int(v['availableWeight']) for v in dv] + sik
    sibs = b''.join(words(int(x) for x in v['censusSiblings']) for v in dv) + b''.join(words(int(x) for x in v['sikSiblings']) for v in dv)
    roots = [int(v['censusRoot']) for v in dv] + [int(v['sikRoot']) for v in dv]
    assert census.check_proofs(ctx, keys, vals, sibs, roots, nl) == [VALID] * 96
    assert census.check_proofs(ctx, keys[:48], vals[:48], sibs[:32 * (nl + 1) * 48], roots[:48], nl) == [VALID] * 48
    # the argument checks on a real context
    lib = _native.load()
    w = b'\0' * 32
    st = (ctypes.c_int32 * 1)(77)
    for bad in (0, 254, -1):
        assert lib.zkc_smt_check_proofs(ctx._h, bad, 1, w, w, b'\0' * 32 * 256, w, 0, st) == 4
    for k in range(5):
        args = [w, w, b'\0' * 32 * (nl + 1), w, st]
        args[k] = None
        assert lib.zkc_smt_check_proofs(ctx._h, nl, 1, *args[:4], 0, args[4]) == 4
    assert list(st) == [77]
    assert lib.zkc_smt_check_proofs(ctx._h, nl, 0, None, None, None, None, 0, None) == 0


def test_agrees_with_the_witness(ctx):
    """64 voters' inputs from two resident trees, 16 of them with one census sibling below the voter's depth tampered: the checker says ROOT_MISMATCH exactly where
    the witness says ZKC_W_ERR_CENSUS_ROOT, VALID exactly where it says ZKC_W_OK."""
    from zkcensus_amd import census
    from zkcensus_amd.inputs import bytes_to_arbo
    rng = random.Random(64)
    N, nl = 512, 160
    nIn = 12 + 2 * (nl + 1); blk = 32 * nIn
    eid, address, password, signature, avail = census._voter_data(N, census.ELECTION_ID_HEX)
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    with census.CensusTree(ctx, nl) as ct, census.CensusTree(ctx, nl) as stree:
        assert ct.add(address, avail) == [0] * N and stree.add(address, sik) == [0] * N
        idx = rng.sample(range(N), 64)
        vh = lambda i: bytes_to_arbo(avail[i].to_bytes((avail[i].bit_length() + 7) // 8 or 1, 'big'))
        pick = lambda xs: [xs[i] for i in idx]
        flat, cr, sr, st = census.census_inputs_from_trees(ctx, ct, stree, eid, pick(address), pick(password), pick(signature), [1] * 64, [vh(i) for i in idx])
        assert st == [0] * 64
        flat = bytearray(flat)
        _, _, dep, _ = ct.gen_proof(pick(address))
        tampered = set(rng.sample(range(64), 16))
        for j in tampered:
            l = rng.randrange(dep[j])
            o = blk * j + 32 * (12 + l)
            flat[o] ^= 1 << rng.randrange(8)
        blocks = [bytes(flat[blk * j:blk * (j + 1)]) for j in range(64)]
        _, wst = ctx.witness(blocks, nl)
        assert sorted(j for j in range(64) if wst[j] == 3) == sorted(tampered)
        word = lambda b, k: int.from_bytes(b[32 * k:32 * k + 32], 'little')
        got = census.check_proofs(ctx, [word(b, 8) for b in blocks], [word(b, 3) for b in blocks], b''.join(b[32 * 12:32 * (12 + nl + 1)] for b in blocks),
                                  [word(b, 7) for b in blocks], nl)
        assert [j for j in range(64) if got[j] == ROOT_MISMATCH] == [j for j in range(64) if wst[j] == 3]
        assert [j for j in range(64) if got[j] == VALID] == [j for j in range(64) if wst[j] == 0]


def test_size_and_chunking(ctx):
    """2^18 proofs in one call (2^20 with ZKC_TEST_FULL=1), every 997th with its value off by one: the verdicts of one call equal those of two calls on the halves."""
    from zkcensus_amd import census
    rng = random.Random(18)
    nl = 160
    n = 1 << (20 if os.environ.get('ZKC_TEST_FULL') == '1' else 18)
    ks = tree_keys(rng, nl, n)
    vs = [rng.randrange(1, 101) for _ in ks]
    kb, vb = words(ks), words(vs)
    root, sib, dep = census.smt_build(ctx, kb, vb, nl)
    bad = set(range(0, n, 997))
    vt = words(v + 1 if i in bad else v for i, v in enumerate(vs))
    want = [ROOT_MISMATCH if i in bad else VALID for i in range(n)]
    got = census.check_proofs(ctx, kb, vt, sib, root, nl)
    assert got == want
    h, blk = n // 2, 32 * (nl + 1)
    assert census.check_proofs(ctx, kb[:32 * h], vt[:32 * h], sib[:blk * h], root, nl) + census.check_proofs(ctx, kb[32 * h:], vt[32 * h:], sib[blk * h:], root, nl) == want
    host, up, kern = census.check_stats(ctx)
    assert host > 0 and up > 0 and kern > 0
