"""TEST INFRASTRUCTURE: the inputs of tests/test_gpu_abc_rows.py and of its child process tests/host/abc_rows_digest.py, built from one seed so that both processes prove the
same voters with the same (r, s).  nLevels = 10.  The pool's first voters are chosen for buildABC's template copy (csrc/zkc_abc_rows.h), whose row list follows the DEEPEST
proof of a pass per tree:
  0  the shallowest voter of a 16-voter synthetic census          1  a voter at the bottom of both trees (census.deep_voters: nothing of its witness folds)
  2  another census voter                                          3, 4  census tree 9 levels down and sik tree 1, and the other way round: the pass' two depths come from different proofs
  5 ..  census voters, then voters at random depths of both trees
and one foreign witness (random field elements behind wire 0), which unfolds the pass it is in."""
import os, random, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
NL, POOL = 10, 65
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# (first voter, count) of the pool per batch, in the order both processes prove them: the deepest-and-shallowest pair, the two-proof early layout, the two depths from different
# proofs, and 65 voters = two passes under the default pass size of 64
BATCHES = ((0, 1), (0, 2), (0, 5), (0, POOL))


def depth_of(v, key):
    return max([i + 1 for i, s in enumerate(v[key]) if int(s) != 0] or [0])


def build(ctx, hash_fn):
    """-> (voters [POOL], rs [POOL + 1] as 64-byte strings, foreign witness)"""
    from census_gen import random_voter
    from zkcensus_amd import census
    rng = random.Random(20261020)
    syn = sorted(census.synthetic_census(ctx, 16, NL), key=lambda v: depth_of(v, 'censusSiblings') + depth_of(v, 'sikSiblings'))
    deep = census.deep_voters(ctx, 1, NL)[0]
    pool = [syn[0], deep, syn[1], random_voter(rng, hash_fn, nLevels=NL, depth_c=9, depth_s=1), random_voter(rng, hash_fn, nLevels=NL, depth_c=1, depth_s=9)] + list(syn[2:])
    while len(pool) < POOL:
        pool.append(random_voter(rng, hash_fn, nLevels=NL, depth_c=rng.randint(0, NL), depth_s=rng.randint(0, NL)))
    rs = [rng.randrange(R).to_bytes(32, 'little') + rng.randrange(R).to_bytes(32, 'little') for _ in range(POOL + 1)]
    nw = ctx.n_wires(NL)
    foreign = (1).to_bytes(32, 'little') + b''.join(rng.randrange(R).to_bytes(32, 'little') for _ in range(nw - 1))
    return pool, rs, foreign
