"""CPU: tests/arbo_model.py, the GPU-free model that the census GPU tests compare the trees with (tests/test_gpu_census_values.py), pinned without a GPU: hand-written
roots, two keys parting at a given bit, every proof and absence proof of random trees climbed by census_lib.oracle_verdict, and smtverifier.circom itself -- through
the oracle's witness -- accepting voters whose two trees are model trees."""
import random
import pytest
import oracle_lib as ol
import arbo_model as am
from census_lib import VALID, model_voters, oracle_verdict

H = ol.poseidon


def test_hand_written_roots():
    """one, two, three and four keys at nLevels 160 (and the small ones at the nLevels that just fits), each root spelled out with the oracle's Poseidon"""
    cases = [
        ({}, 0),
        ({5: 6}, H([5, 6, 1])),
        ({0: 0}, H([0, 0, 1])),                                                                      # key 0 with value 0 is a real leaf
        ({0b0: 1, 0b1: 2}, H([H([0, 1, 1]), H([1, 2, 1])])),
        ({0b1: 2, 0b0: 1}, H([H([0, 1, 1]), H([1, 2, 1])])),                                         # the order of insertion does not matter
        ({0b00: 1, 0b10: 2}, H([H([H([0, 1, 1]), H([2, 2, 1])]), 0])),                                # H(H(H(a,1,1), H(b,2,1)), 0): a chain node with an empty right child
        ({0b01: 1, 0b11: 2}, H([0, H([H([1, 1, 1]), H([3, 2, 1])])])),
        ({0b00: 1, 0b10: 2, 0b1: 3}, H([H([H([0, 1, 1]), H([2, 2, 1])]), H([1, 3, 1])])),
        ({0b10: 1, 1 + (1 << 40): 2, 1 + (1 << 40) + (1 << 100): 3},                                 # x left of the root; a, b on the right, sharing 100 bits
         None),
        ({0b000: 1, 0b100: 2, 0b010: 3, 0b1: 4}, H([H([H([H([0, 1, 1]), H([4, 2, 1])]), H([2, 3, 1])]), H([1, 4, 1])])),
        ({0b00: 1, 0b01: 2, 0b10: 3, 0b11: 4}, H([H([H([0, 1, 1]), H([2, 3, 1])]), H([H([1, 2, 1]), H([3, 4, 1])])])),
    ]
    a = 1 + (1 << 40); b = a + (1 << 100)
    chain = H([H([a, 2, 1]), H([b, 3, 1])])                       # a and b part at bit 100, where a has 0
    for l in range(99, 0, -1):                                    # above it both have bit 40 set and bits 1..39, 41..99 clear
        chain = H([0, chain]) if l == 40 else H([chain, 0])
    cases[8] = (cases[8][0], H([H([2, 1, 1]), chain]))            # bit 0: x = 0b10 left, a and b right
    for kv, want in cases:
        assert am.root(kv, 160) == want, kv
        nl = max([k.bit_length() for k in kv] + [1])
        if nl <= 3:
            assert am.root(kv, nl) == want, (kv, nl)
    assert am.inner_nodes_per_depth({0b00: 1, 0b10: 2, 0b1: 3}, 3) == [1, 1, 0]
    assert am.inner_nodes_per_depth({}, 2) == [0, 0] and am.inner_nodes_per_depth({7: 7}, 1) == [0]
    assert am.proof({5: 6}, 160, 5) == ([0] * 161, 0, True)
    assert am.proof({5: 6}, 160, 4) == ([0] * 161, 0, False)
    assert am.absence_proof({}, 160, 7) == ([0] * 161, 0, 0, 0, 1)
    assert am.absence_proof({9: 10}, 160, 7) == ([0] * 161, 0, 9, 10, 0)
    s, d, ok, ov, o0 = am.absence_proof({0b00: 1, 0b10: 2}, 160, 0b1)
    assert (s[0], s[1:], d, ok, ov, o0) == (H([H([0, 1, 1]), H([2, 2, 1])]), [0] * 160, 1, 0, 0, 1)
    with pytest.raises(KeyError):
        am.absence_proof({9: 10}, 160, 9)


@pytest.mark.parametrize('b', [0, 31, 32, 252])
def test_two_keys_parting_at_bit(b):
    """two keys sharing their low b bits at nLevels 253: both leaves b + 1 levels down, the only non-zero sibling at level b, b chain nodes with one child each"""
    rng = random.Random(b)
    nl = 253
    low = rng.getrandbits(b) if b else 0
    k0 = low | (rng.getrandbits(252 - b) << (b + 1) if b < 252 else 0); k1 = low | (1 << b)
    assert k0 < ol.R and k1 < ol.R
    kv = {k1: 11, k0: 12}
    assert am.inner_nodes_per_depth(kv, nl) == [1] * (b + 1) + [0] * (nl - b - 1)
    cur = H([H([k0, 12, 1]), H([k1, 11, 1])])
    for l in range(b - 1, -1, -1):
        cur = H([0, cur]) if (low >> l) & 1 else H([cur, 0])
    assert am.root(kv, nl) == cur
    for k, v, other in ((k0, 12, H([k1, 11, 1])), (k1, 11, H([k0, 12, 1]))):
        s, d, ex = am.proof(kv, nl, k)
        assert ex and d == b + 1 and s == [0] * b + [other] + [0] * (nl - b) and len(s) == nl + 1
        assert oracle_verdict(k, v, s, cur, nl) == VALID
    if b < 252:
        with pytest.raises(ValueError):
            am.root(kv, b)                                         # the two agree on their first b bits
        assert am.root(kv, b + 1) == cur


@pytest.mark.parametrize('nl', [12, 253])
def test_every_proof_of_a_random_tree_climbs_to_its_root(nl):
    """200 random keys: every membership proof and the absence proofs of 200 other keys (both is_old0 kinds occur) are VALID for census_lib.oracle_verdict, which knows
    nothing of the tree's shape; depths are 1 + the last non-zero sibling; a wrong value is not"""
    rng = random.Random(nl)
    low = rng.sample(range(1 << 12), 400)
    ks = [l | (rng.getrandbits(241) << 12) for l in low]           # distinct low 12 bits, below 2^253 < r
    kv = {k: rng.randrange(ol.R) for k in ks[:200]}
    rt = am.root(kv, nl)
    depth_of = lambda s: max((l + 1 for l in range(nl) if s[l]), default=0)
    n = 0
    for k, v in kv.items():
        s, d, ex = am.proof(kv, nl, k)
        assert ex and len(s) == nl + 1 and d == depth_of(s) and oracle_verdict(k, v, s, rt, nl) == VALID
        n += 1
    assert oracle_verdict(ks[0], (kv[ks[0]] + 1) % ol.R, am.proof(kv, nl, ks[0])[0], rt, nl) != VALID
    kinds = [0, 0]
    for k in ks[200:] + [ks[0] ^ (1 << 252)]:                      # the last: a twin of a present key that differs only above nl (at nLevels 12) or at the last level
        s, d, okey, oval, o0 = am.absence_proof(kv, nl, k)
        assert len(s) == nl + 1 and d == depth_of(s) and (okey in kv and kv[okey] == oval if not o0 else (okey, oval) == (0, 0))
        assert oracle_verdict(k, oval, s, rt, nl, okey, o0) == VALID
        assert am.proof(kv, nl, k) == ([0] * (nl + 1), 0, False)
        kinds[o0] += 1
    assert n == 200 and sum(kinds) == 201 and min(kinds) > 0, kinds
    assert sum(am.inner_nodes_per_depth(kv, nl)) >= 199


def test_the_circuit_accepts_the_model():
    """nLevels 10, 16 voters whose census and SIK trees are model trees: the oracle's witness generator (census.circom with smtverifier.circom) accepts each"""
    rng = random.Random(10)
    nl, n = 10, 16
    address = [l | (rng.getrandbits(150) << nl) for l in rng.sample(range(1 << nl), n)]
    password = [rng.getrandbits(88) for _ in range(n)]; signature = [rng.getrandbits(512) % ol.R for _ in range(n)]
    avail = [rng.randrange(1, 101) for _ in range(n)]
    voters = model_voters((rng.getrandbits(128), rng.getrandbits(128)), address, password, signature, avail, [1] * n, [(rng.getrandbits(128), 7)] * n, nl)
    assert len(voters) == n and len({v['censusRoot'] for v in voters}) == 1 and len({v['sikRoot'] for v in voters}) == 1
    assert max(max(i + 1 for i, s in enumerate(v['censusSiblings']) if s != '0') for v in voters) >= 4
    assert [ol.witness(v, nl)[0] for v in voters] == [0] * n
    bad = dict(voters[3]); bad['censusRoot'] = voters[3]['sikRoot']
    assert ol.witness(bad, nl)[0] != 0


def test_a_collision_raises():
    """two keys that agree on their first nLevels bits; one level more holds both"""
    assert 5 + (1 << 253) < ol.R
    for kv, nl in (({1: 1, 1 + (1 << 12): 2}, 12), ({0: 1, 2: 2}, 1), ({5: 1, 5 + (1 << 253): 2}, 253), ({3: 1, 7: 1, 9: 1}, 2), ({1: 1, 1 + (1 << 252): 2}, 252)):
        with pytest.raises(ValueError):
            am.root(kv, nl)
        with pytest.raises(ValueError):
            am.inner_nodes_per_depth(kv, nl)
        if nl < 253:
            assert am.root(kv, nl + 1) != 0
    for nl in (0, 254):
        with pytest.raises(ValueError):
            am.root({1: 1}, nl)
    with pytest.raises(ValueError):
        am.root({ol.R: 1}, 160)
    with pytest.raises(ValueError):
        am.root({1: ol.R}, 160)
