"""TEST INFRASTRUCTURE: the inputs of the blinding-edge tests (tests/test_gpu_blinding_edges.py, tests/test_00_gpu_switches.py and its child tests/host/blind_digest.py), built from one
seed on the CPU alone so that a parent process that never touches the GPU, its child and the in-process GPU tests all prove the very same bytes.

The blinding step (csrc/zkc_finalize.hip) multiplies by r, s and r s: the pairs below are the values at which a windowed scalar product, an addition with infinity or a
reduction mod R goes wrong -- zero scalars, r s = +-1, a scalar whose only non-zero 4-bit window is the top one, windows that are all 0xF, a single low or middle window."""
import os, random, sys
import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
R = ol.R
SEED = 20261018
NL = 10
K = random.Random(SEED).randrange(2, R)                 # the k of the list: random, fixed by the seed
KINV = pow(K, -1, R)
RANDOM_PAIR = (random.Random(SEED + 1).randrange(R), random.Random(SEED + 2).randrange(R))
EDGE_PAIRS = [(0, 0), (0, K), (K, 0), (1, 1), (R - 1, R - 1), (R - 1, 1), (K, KINV), (K, R - KINV), (1 << 252, 1 << 252), ((1 << 252) - 1, (1 << 252) - 1),
              (15, 15 * 16**31), (16**40, 16**17)]
ALL_PAIRS = EDGE_PAIRS + [RANDOM_PAIR]
assert all(0 <= x < R for p in ALL_PAIRS for x in p) and K * KINV % R == 1 and K * (R - KINV) % R == R - 1


def layout(n):
    """(r, s) for the n proofs of a batch: proofs 0, 1, 63, 64 (where present) and the last one carry an edge pair, the whole list rotates over the other slots; the rotation
    starts at a different pair for every n, so that the batches of 3, 4 and 5 proofs see the twelve edge pairs between them"""
    start = {3: 0, 4: 8, 5: 3, 64: 0, 65: 5}.get(n, n)
    fixed = sorted({0, 1, 63, 64, n - 1} & set(range(n)))
    out = [None] * n
    for j, i in enumerate(fixed):
        out[i] = EDGE_PAIRS[(start + j) % len(EDGE_PAIRS)]
    k = 0
    for i in range(n):
        if out[i] is None:
            out[i] = ALL_PAIRS[(start + len(fixed) + k) % len(ALL_PAIRS)]; k += 1
    return out


def rs_bytes(pairs):
    return b''.join(r.to_bytes(32, 'little') + s.to_bytes(32, 'little') for r, s in pairs)


_voters = None


def voter_witnesses():
    """65 accepted voters of the nLevels-10 circuit (random depths 0..nLevels in both trees; the first four are depth 0 and depth nLevels in both, and crossed) as witness bytes
    from the CPU oracle, and one foreign vector [1] + random that is no witness of the circuit and gets no fold constants"""
    global _voters
    if _voters is None:
        from census_gen import random_voter
        rng = random.Random(SEED + 3)
        depths = [(0, 0), (NL, NL), (0, NL), (NL, 0)] + [(rng.randrange(0, NL + 1), rng.randrange(0, NL + 1)) for _ in range(61)]
        voters = [random_voter(rng, ol.poseidon, nLevels=NL, depth_c=dc, depth_s=ds) for dc, ds in depths]
        ws = ol.pmap(lambda v: ol.witness(v, NL), voters)
        assert all(rc == 0 for rc, _ in ws)
        nW = len(ws[0][1]) // 32
        foreign = b''.join([(1).to_bytes(32, 'little')] + [rng.randrange(R).to_bytes(32, 'little') for _ in range(nW - 1)])
        # what unfolds a pass (zkc_fold_check, last flag of either tree): the n2bOld block of a witness differs from the voter-independent template.  Every voter carries the
        # same bytes there and the foreign vector does not, so a pass of given witnesses that holds it runs unfolded (dc = 255 for each of its proofs)
        from zkcensus_amd import r1cs
        L = r1cs.Layout(NL)
        for blk in (L.off_census, L.off_sikver):
            lo, hi = 32 * (blk + L.off_n2bold), 32 * (blk + L.off_n2bold + 253 + 127 + 133)
            assert len({w[lo:hi] for _, w in ws}) == 1 and foreign[lo:hi] != ws[0][1][lo:hi]
        _voters = ([w for _, w in ws], foreign)
    return _voters


def foreign_index(n):
    return 64 if n == 65 else 1                           # index 64 is the first lane of the second 64-lane block


def batch(n, with_foreign=True):
    """-> (witnesses [n] as bytes, (r, s) [n], index of the foreign witness or None).  Voter i of every batch is the same voter."""
    ws, foreign = voter_witnesses()
    wl = list(ws[:n]); fi = foreign_index(n) if with_foreign else None
    if fi is not None:
        wl[fi] = foreign
    return wl, layout(n), fi


# ---- the degenerate generic instance: a proof whose MSM results are (nearly) all the point at infinity ----
DEGEN_SEED = 777
DEGEN_PUB = 2
W_A_ONLY, W_B_ONLY = 1, 2                               # the two public wires: one stands in A rows only, the other in B rows only (a public wire has no point in the C section)


def degenerate_instance(directory):
    """A hand-made system of 300 constraints over 40 wires: no row names wire 0 and every side is a linear form without a constant, so the all-zero assignment satisfies
    every constraint.  Wire 1 stands in A rows only, wire 2 in B rows only (both public), the others anywhere.  -> (.r1cs path, {name: witness bytes}):
      'zero'    (1, 0, .., 0): B1', B2', C' and H are the point at infinity.  A' is NOT: the setup follows snarkjs, whose rows nCons + i (A = wire i, i <= nPublic) give wire 0
                the A polynomial L_nCons, so A' = L_nCons(tau) G here (closed_form.proof_scalars adds the same rows): r B1' starts from infinity, s A' does not
      'a_only'  wire 1 alone non-zero: A' changes, B1' = B2' = C' = H = infinity still (B = 0 on the whole domain)
      'b_only'  wire 2 alone non-zero: B1' and B2' finite, C' = infinity, and H finite (A B = L_nCons B vanishes on the domain without being zero)
      'a_inf'   wire 1 chosen so that A' IS infinity: A(tau) = L_nCons(tau) + w_1 A_1(tau) is linear in w_1 and tau is known (the closed form's seed), so
                w_1 = -A(tau)[w_1 = 0] / (A(tau)[w_1 = 1] - A(tau)[w_1 = 0]) makes A(tau) = 0.  Any w_1 satisfies every constraint (B = 0 on the whole domain).  All five MSM
                results are infinity: pi_a = alpha + r delta, pi_b = beta2 + s delta2, and at (0, 0) the proof is (alpha, beta2, infinity)"""
    import closed_form as cf
    from zkcensus_amd import r1cs
    rng = random.Random(DEGEN_SEED)
    nW, nC = 40, 300
    cs = r1cs.R1CS(nW, DEGEN_PUB)
    anywhere = list(range(1, nW)); anywhere.remove(W_A_ONLY); anywhere.remove(W_B_ONLY)
    lc = lambda pool, n: {w: rng.randrange(1, R) for w in rng.sample(pool, n)}
    for k in range(nC):
        cs.add(lc(anywhere + [W_A_ONLY] * (k % 3 == 0), 1 + rng.randrange(3)), lc(anywhere + [W_B_ONLY] * (k % 3 == 1), 1 + rng.randrange(3)), lc(anywhere, rng.randrange(3)))
    assert any(W_A_ONLY in a for a, _, _ in cs.cons) and any(W_B_ONLY in b for _, b, _ in cs.cons)
    assert not any(0 in side for con in cs.cons for side in con) and not any(W_A_ONLY in b or W_A_ONLY in c or W_B_ONLY in a or W_B_ONLY in c for a, b, c in cs.cons)
    wits = {}
    for name, wire in (('zero', None), ('a_only', W_A_ONLY), ('b_only', W_B_ONLY)):
        w = [1] + [0] * (nW - 1)
        if wire is not None:
            w[wire] = rng.randrange(1, R)
        assert cs.check(w) == -1
        wits[name] = b''.join(x.to_bytes(32, 'little') for x in w)
    path = os.path.join(str(directory), 'degenerate.r1cs')
    cs.write(path)
    alpha = cf.toxic_waste(DEGEN_SEED)[1]
    at = lambda w1: (cf.proof_scalars(path, DEGEN_SEED, [1, w1] + [0] * (nW - 2), 0, 0)[0] - alpha) % R          # A(tau) for wire 1 = w1
    w1 = -at(0) * pow(at(1) - at(0), -1, R) % R
    assert at(w1) == 0 and cs.check([1, w1] + [0] * (nW - 2)) == -1
    wits['a_inf'] = b''.join(x.to_bytes(32, 'little') for x in [1, w1] + [0] * (nW - 2))
    return path, wits


def setup_key(r1cs_path, seed=DEGEN_SEED):
    """-> (.zkey bytes, verification key) from the test-only setup with known toxic waste (the closed form's seed)"""
    import ctypes, json
    from zkcensus_amd import _native
    z, v = r1cs_path[:-5] + '.zkey', r1cs_path[:-5] + '_vkey.json'
    err = ctypes.create_string_buffer(512)
    rc = _native.load().zkc_setup_from_r1cs(r1cs_path.encode(), seed, z.encode(), v.encode(), err, 512)
    assert rc == 0, err.value
    return open(z, 'rb').read(), json.load(open(v))


DEGEN_PAIRS = [(0, 0), (0, K), (K, 0), (R - 1, R - 1), (K, KINV), ((1 << 252) - 1, 1 << 252), RANDOM_PAIR]
