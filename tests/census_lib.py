"""What the census GPU tests share (test_gpu_smt_check, test_gpu_census_tree, _delete, _snapshot, _values): byte helpers, the ZKC_SMT_* verdicts, key sets, the comparison of
a resident tree with zkc_smt_build over the same set, a pure-Python proof climber over the oracle's Poseidon, and voters' circuit inputs from arbo_model trees.  A plain
module beside oracle_lib.py: no fixtures."""
import oracle_lib as ol

W = ol.le32
words = lambda xs: b''.join(W(x) for x in xs)
VALID, ROOT_MISMATCH, NOT_BELOW_R, LAST_SIBLING, KEY_PRESENT, OFF_PATH = range(6)      # ZKC_SMT_* (include/zkcensus.h)
ZKC_ERR_BAD_ARG = 4


def sib_list(sib, i, nl):
    """proof i's nl + 1 siblings as integers, from the zero-padded layout of zkc_smt_build / gen_proof"""
    blk = 32 * (nl + 1)
    return [int.from_bytes(sib[blk * i + 32 * l:blk * i + 32 * l + 32], 'little') for l in range(nl + 1)]


def oracle_verdict(key, value, sibs, root, nl, old_key=None, is_old0=False):
    """The verdict of one census proof in Python over the oracle's Poseidon (no call into the library on this side).  Membership (old_key None): arbo CheckProof with
    the circuit's extra rules, the climb starts at H(key, value, 1).  Absence (old_key given; value is the old value): circomlib SMTVerifier with fnc = 1 over this
    project's conventions, the climb starts at 0 (is_old0) or at H(old_key, value, 1) and follows the key's path bits."""
    absent = old_key is not None
    if any(x >= ol.R for x in [key, value, root] + ([old_key] if absent else []) + sibs):
        return NOT_BELOW_R
    if sibs[nl]:
        return LAST_SIBLING
    d = max((l + 1 for l in range(nl) if sibs[l]), default=0)
    if absent and not is_old0 and old_key == key:
        return KEY_PRESENT
    if absent and not is_old0 and (old_key ^ key) & ((1 << d) - 1):
        return OFF_PATH
    cur = 0 if absent and is_old0 else ol.poseidon([old_key if absent else key, value, 1])
    for l in range(d - 1, -1, -1):
        cur = ol.poseidon([sibs[l], cur]) if (key >> l) & 1 else ol.poseidon([cur, sibs[l]])
    return VALID if cur == root else ROOT_MISMATCH


def model_voters(election_id, address, password, signature, avail, vote, vote_hash, nl):
    """The 12-key circuit inputs (oracle_lib.INPUT_KEYS, decimal strings) of voters whose census tree (address -> available weight) and SIK tree (address ->
    H(address, password, signature)) are arbo_model trees: no GPU code on this side.  Lists of ints; vote_hash: pairs; election_id: a pair."""
    import arbo_model as am
    sik = [ol.poseidon([a, p, s]) for a, p, s in zip(address, password, signature)]
    ckv, skv = dict(zip(address, avail)), dict(zip(address, sik))
    out = []
    for i, a in enumerate(address):
        v = {'electionId': list(election_id), 'nullifier': ol.poseidon([signature[i], password[i], election_id[0], election_id[1]]), 'availableWeight': avail[i],
             'voteHash': list(vote_hash[i]), 'sikRoot': am.root(skv, nl), 'censusRoot': am.root(ckv, nl), 'address': a, 'password': password[i],
             'signature': signature[i], 'voteWeight': vote[i], 'censusSiblings': am.proof(ckv, nl, a)[0], 'sikSiblings': am.proof(skv, nl, a)[0]}
        assert list(v) == ol.INPUT_KEYS
        out.append({k: [str(y) for y in x] if isinstance(x, list) else str(x) for k, x in v.items()})
    return out


def tree_keys(rng, nl, n, avoid=()):
    """n distinct random keys below r; at nLevels < 32 their low nl bits are distinct too (and of `avoid`'s), the high bits random"""
    if nl >= 32:
        return [k for k in dict.fromkeys(rng.getrandbits(nl) for _ in range(n + 64)) if k not in avoid][:n]
    taken = {k & ((1 << nl) - 1) for k in avoid}
    free = [l for l in range(1 << nl) if l not in taken]
    return [l | (rng.getrandbits(200) << nl) for l in rng.sample(free, n)]


def fresh_keys(rng, seen, m, bits):
    """m random keys of `bits` bits that `seen` (a set, updated) does not hold yet"""
    out = []
    while len(out) < m:
        k = rng.getrandbits(bits)
        if k not in seen:
            seen.add(k); out.append(k)
    return out


def fresh_tree(ctx, kv, nl):
    from zkcensus_amd import census
    t = census.CensusTree(ctx, nl)
    if kv:
        assert t.add(list(kv), list(kv.values())) == [0] * len(kv)
    return t


def equals_rebuild(ctx, tree, kv, nl, others=()):
    """tree (live or snapshot) equals zkc_smt_build over kv (a dict): root, size, every key's siblings / depth / value; the keys of `others` that kv does not hold are
    absent from it (no siblings, depth 0, value 0), and their absence proofs are those of a tree built fresh from kv and valid against the tree's root"""
    from zkcensus_amd import census
    ks = list(kv)
    absent = [k for k in dict.fromkeys(others) if k not in kv]
    if not ks and not absent:                                  # nothing to ask the tree for: an empty call is not made
        assert tree.root == 0 and len(tree) == 0
        return
    root, sib, dep = census.smt_build(ctx, ks, [kv[k] for k in ks], nl) if ks else (0, b'', [])
    assert tree.root == root and len(tree) == len(ks)
    r, s, d, ex = tree.gen_proof(ks + absent)
    blk = 32 * (nl + 1)
    assert r == root and ex == [True] * len(ks) + [False] * len(absent)
    assert d == dep + [0] * len(absent)
    assert s[:blk * len(ks)] == sib and s[blk * len(ks):] == b'\0' * blk * len(absent)
    vals, ex = tree.get(ks + absent)
    assert vals == [kv[k] for k in ks] + [0] * len(absent) and ex == [True] * len(ks) + [False] * len(absent)
    if absent:
        got = tree.gen_absence_proof(absent)
        with fresh_tree(ctx, kv, nl) as f:
            assert got == f.gen_absence_proof(absent)
        r, sib_a, dep_a, ok, ov, o0, st = got
        assert st == [0] * len(absent) and r == root
        assert tree.check_absence(absent, ok, ov, o0, sib_a) == [VALID] * len(absent)
