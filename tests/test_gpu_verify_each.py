"""GPU: the batch verifier with a verdict per proof (zkc_verify_batch_each, groth16.verify_each).  The expected verdict of a member is always the oracle's on that member
alone (the pinned pairing verifier: VALID or INVALID) unless the tampering is an encoding error, whose class the case states.  Every case also checks that verify_batch
returns the AND of the verdicts for the same inputs and seed, and that the context verifies an honest batch afterwards."""
import contextlib
import math
import os
import random
import sys
import json
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
SEED = bytes(range(32))


@pytest.fixture(scope='module')
def twelve():
    """Twelve honest proofs at nLevels = 10, made as tests/test_gpu_batch_verify.py makes its twelve: (ctx, groth16, vk, [proof], [public-signal block])"""
    import torch, numpy as np
    import zkcensus_amd
    from zkcensus_amd import groth16, setup
    from census_gen import random_voter
    nl, base = 10, 12
    ctx = zkcensus_amd.Context(0)
    _, zp, vp = setup.ensure_test_artifacts(nl)
    pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read()); vk = json.load(open(vp))
    rng = random.Random(12)
    voters = [random_voter(rng, ol.poseidon, nLevels=nl, depth_c=rng.randint(1, nl), depth_s=rng.randint(1, nl)) for _ in range(base)]
    ws, st = ctx.witness(voters, nLevels=nl); assert st == [0] * base
    d = torch.from_numpy(np.frombuffer(b''.join(ws), dtype=np.uint8).copy()).cuda()
    rs = b''.join(rng.randrange(ol.R).to_bytes(32, 'little') for _ in range(2 * base))
    proofs, pubs = pk.prove_batch_dev(d.data_ptr(), base, rs)
    P = [proofs[256 * i:256 * (i + 1)] for i in range(base)]; U = [pubs[256 * i:256 * (i + 1)] for i in range(base)]
    assert all(ol.verify(vk, u, p) for p, u in zip(P, U))
    yield ctx, groth16, vk, P, U
    pk.close(); ctx.close()


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


_oracle_said = {}


def oracle_verdict(vk, u, p):
    """The oracle on one member alone, computed once per distinct (signals, proof)"""
    if (u, p) not in _oracle_said:
        _oracle_said[(u, p)] = 0 if ol.verify(vk, u, p) else 1
    return _oracle_said[(u, p)]


def check(twelve, P, U, stated=None, seed=SEED):
    """verify_each on (P, U): member i gets stated[i] where the case states a class, else the oracle's verdict; verify_batch agrees; the context still works.
    Returns (verdicts, stats)."""
    ctx, groth16, vk, P0, U0 = twelve
    stated = stated or {}
    expected = [stated[i] if i in stated else oracle_verdict(vk, U[i], P[i]) for i in range(len(P))]
    got = groth16.verify_each(ctx, vk, b''.join(U), b''.join(P), seed)
    stats = groth16.verify_each_stats(ctx)
    print('N=%d bad=%d stats=%s' % (len(P), sum(1 for v in expected if v), stats))
    assert got == expected, [(i, g, e) for i, (g, e) in enumerate(zip(got, expected)) if g != e]
    assert groth16.verify_batch(ctx, vk, b''.join(U), b''.join(P), seed) is all(v == groth16.PROOF_VALID for v in got)
    n = min(len(P), 12)
    assert groth16.verify_batch(ctx, vk, b''.join(U0[:n]), b''.join(P0[:n]), seed) is True
    return got, stats


def repeated(P, U, N):
    return [P[i % len(P)] for i in range(N)], [U[i % len(U)] for i in range(N)]


def other_c(P, Pn, i):
    """member i with the C of the next of the twelve: every point still on its curve, only the pairing equation can tell"""
    return Pn[i][:192] + P[(i + 1) % len(P)][192:]


@pytest.mark.parametrize('path', ['0', '1'])
def test_every_class_in_one_batch(twelve, path):
    """N = 24 with the Miller loops on host threads and on the GPU: an honest batch costs nothing extra; then one call with every kind of bad member at once."""
    ctx, groth16, vk, P, U = twelve
    Pn, Un = repeated(P, U, 24)
    with env(ZKC_VERIFY_BATCH_GPU=path):
        got, stats = check(twelve, Pn, Un)
        assert got == [groth16.PROOF_VALID] * 24 and stats == (0, 0, 0, 0)
        Pb, Ub = list(Pn), list(Un)
        Pb[5] = Pn[5][:192] + Pn[7][192:]                                                   # another proof's C
        Pb[2], Pb[3] = Pn[3][:64] + Pn[2][64:], Pn[2][:64] + Pn[3][64:]                     # A points swapped
        Pb[9] = b'\xff' * 32 + Pn[9][32:]                                                   # a coordinate >= q
        pt = ol.twist_point_outside_g2()
        Pb[4] = Pn[4][:64] + b''.join(ol.le32(v) for v in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])) + Pn[4][192:]      # B on the twist, outside G2
        Pb[6] = Pn[6][:64] + bytes(128) + Pn[6][192:]                                       # B at infinity: the oracle decides
        Ub[11] = Un[11][:64] + b'\xff' * 32 + Un[11][96:]                                   # a public signal >= r
        y = int.from_bytes(Pn[0][32:64], 'little')
        Pb[0] = Pn[0][:32] + ol.le32((ol.Q - y) % ol.Q) + Pn[0][64:]                        # -A
        stated = {5: groth16.PROOF_INVALID, 2: groth16.PROOF_INVALID, 3: groth16.PROOF_INVALID, 9: groth16.PROOF_MALFORMED, 4: groth16.PROOF_MALFORMED,
                  11: groth16.PROOF_PUBLIC_RANGE, 0: groth16.PROOF_INVALID}
        for i in (5, 2, 3, 0):
            assert oracle_verdict(vk, Ub[i], Pb[i]) == groth16.PROOF_INVALID
        got, _ = check(twelve, Pb, Ub, stated)
        # a member that fails both kinds of format check is MALFORMED
        Ub[9] = b'\xff' * 32 + Un[9][32:]
        check(twelve, Pb, Ub, stated)


@pytest.mark.parametrize('N,chunk', [(129, None), (301, '100'), (257, '2')])
def test_tree_shapes_and_round_boundaries(twelve, N, chunk):
    """Odd levels, several rounds of pairs, rounds of two: one bad member at the start, at 100 and at the end, the sibling pair (100, 101), a whole round bad, and all of
    them together.  One bad member is found by bisection -- at most two range checks per level of the tree over the rounds and of the tree inside the round, and one leaf of
    two verified singly -- which is what the bounds on the counters say."""
    ctx, groth16, vk, P, U = twelve
    Pn, Un = repeated(P, U, N)
    placements = [[0], [100], [N - 1], [100, 101]] + ([list(range(100, 200))] if chunk == '100' else [])
    placements.append(sorted({i for pl in placements for i in pl}))
    with env(ZKC_VERIFY_CHUNK=chunk):
        for bad in placements:
            Pb = list(Pn)
            for i in bad: Pb[i] = other_c(P, Pn, i)
            got, stats = check(twelve, Pb, Un)
            assert [i for i, v in enumerate(got) if v == groth16.PROOF_INVALID] == bad
            if len(bad) == 1:
                assert stats[0] <= 2 * math.ceil(math.log2(N)) + 2 and stats[1] <= 2 and stats[3] == 0, stats


@pytest.mark.parametrize('N', [1, 2, 3, 5])
def test_tiny_batches_on_the_gpu_path(twelve, N):
    ctx, groth16, vk, P, U = twelve
    with env(ZKC_VERIFY_BATCH_GPU='1'):
        got, stats = check(twelve, P[:N], U[:N])
        assert got == [0] * N and stats == (0, 0, 0, 0)
        for bad_at in sorted({0, N - 1}):
            Pb = list(P[:N]); Pb[bad_at] = other_c(P, P, bad_at)
            got, _ = check(twelve, Pb, U[:N])
            assert [i for i, v in enumerate(got) if v] == [bad_at]


def test_budget_ends_the_descent(twelve):
    """N = 64 with 40 bad members: the range checks reach max(16, N / 4) = 16, the rest is verified singly, and the verdicts are still exact"""
    ctx, groth16, vk, P, U = twelve
    Pn, Un = repeated(P, U, 64)
    bad = sorted(random.Random(5).sample(range(64), 40))
    Pb = list(Pn)
    for i in bad: Pb[i] = other_c(P, Pn, i)
    with env(ZKC_VERIFY_BATCH_GPU='1'):
        got, stats = check(twelve, Pb, Un)
    assert [i for i, v in enumerate(got) if v == groth16.PROOF_INVALID] == bad
    assert stats[3] == 1 and stats[1] <= 64 and stats[0] <= 16, stats


def test_seeded_and_unseeded_calls_agree(twelve):
    ctx, groth16, vk, P, U = twelve
    Pn, Un = repeated(P, U, 24)
    Pb = list(Pn); Pb[7] = other_c(P, Pn, 7); Pb[20] = other_c(P, Pn, 20)
    for path in ('0', '1'):
        with env(ZKC_VERIFY_BATCH_GPU=path):
            a, _ = check(twelve, Pb, Un, seed=SEED)
            b, _ = check(twelve, Pb, Un, seed=None)
            c, _ = check(twelve, Pb, Un, seed=bytes(range(100, 132)))
            assert a == b == c and [i for i, v in enumerate(a) if v] == [7, 20]
