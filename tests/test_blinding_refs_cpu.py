"""CPU: the two references of the blinding-edge GPU tests agree with each other before those tests rely on them.  For the degenerate generic instance
(tests/blinding_cases.py: MSM results at infinity) the C oracle's prover (oracle/groth16.c: transforms and Pippenger over the .zkey) gives the bytes of the toxic-waste closed
form (tests/closed_form.py: field arithmetic alone) at every edge (r, s) the GPU test uses, (0, 0) included -- and both can express pi_c = infinity: 64 zero bytes.  The edge
list and the layouts the batches share are checked here too, so that a slip in them shows without a GPU."""
import pytest
import oracle_lib as ol
import closed_form as cf
import blinding_cases as bc


@pytest.fixture(scope='module')
def degen(tmp_path_factory):
    r1, wits = bc.degenerate_instance(tmp_path_factory.mktemp('degenerate'))
    zk, vk = bc.setup_key(r1)
    return r1, zk, vk, wits


def test_edge_pairs_are_what_they_claim():
    R, K = bc.R, bc.K
    nib = lambda x: [(x >> (4 * i)) & 15 for i in range(64)]
    assert len(bc.EDGE_PAIRS) == 12 and len(set(bc.ALL_PAIRS)) == 13
    assert [r * s % R for r, s in bc.EDGE_PAIRS[6:8]] == [1, R - 1]
    assert nib(1 << 252) == [0] * 63 + [1] and nib((1 << 252) - 1) == [15] * 63 + [0]             # only the top window; every window 0xF below a zero top window
    assert nib(15 * 16**31) == [0] * 31 + [15] + [0] * 32 and nib(16**40)[40] == 1 and sum(nib(16**40)) == 1 and nib(16**17)[17] == 1
    for n in (3, 4, 5, 64, 65):
        lay = bc.layout(n)
        assert len(lay) == n and all(lay[i] in bc.EDGE_PAIRS for i in {0, 1, 63, 64, n - 1} if i < n)
        assert bc.foreign_index(n) == (64 if n == 65 else 1)
    assert set(bc.layout(64)) == set(bc.layout(65)) == set(bc.ALL_PAIRS)                             # the full passes see every pair
    assert set(bc.layout(3)) | set(bc.layout(4)) | set(bc.layout(5)) == set(bc.EDGE_PAIRS)         # and the small ones every edge pair between them


def test_oracle_equals_closed_form_on_the_degenerate_instance(degen):
    """Recorded here: both references express pi_c = infinity (64 zero bytes).  For the witness (1, 0, .., 0) pi_a is not alpha alone -- snarkjs' public-input rows give
    wire 0 an A polynomial, so at (0, 0) that proof is pi_a = (alpha + L_nCons(tau)) G1, pi_b = beta G2, pi_c = infinity.  The 'a_inf' witness cancels that term with wire 1:
    A' = infinity, pi_a = (alpha + r delta) G1, and at (0, 0) the proof is the key's alpha1, its beta2 and infinity."""
    r1, zk, vk, wits = degen
    tau, alpha, beta, gamma, delta = cf.toxic_waste(bc.DEGEN_SEED)
    for name, w in wits.items():
        for r, s in bc.DEGEN_PAIRS:
            rc, proof, pub = ol.prove(zk, w, r, s, npub=bc.DEGEN_PUB)
            assert rc == 0, (name, r, s)
            a, b, c = cf.proof_scalars(r1, bc.DEGEN_SEED, w, r, s)
            assert proof == cf.proof_from_scalars(ol, a, b, c), (name, r, s)
            assert ol.verify(vk, pub, proof), (name, r, s)
            if name == 'a_inf':
                assert a == (alpha + r * delta) % bc.R and c == (s * a + r * b - r * s * delta) % bc.R   # A' = B1' = C' = H = infinity
            if name != 'b_only':
                assert b == (beta + s * delta) % bc.R                                                # B(tau) = 0: pi_b = beta2 + s delta2
            if (r, s) == (0, 0) and name != 'b_only':                                              # C' = H = infinity and no blinding term: pi_c = infinity
                assert c == 0 and proof[192:] == bytes(64) and proof[64:192] == ol.msm_g2(cf.G2_GEN, ol.le32(b))
                assert (a == alpha) == (name == 'a_inf')                                           # A' = L_nCons(tau) G1 is not infinity unless wire 1 cancels it
                if name == 'a_inf':
                    assert proof == ol.g1_json(vk['vk_alpha_1']) + ol.g2_json(vk['vk_beta_2']) + bytes(64)
            else:
                assert proof[192:] != bytes(64)
    # the three witnesses differ where they should: wire 1 moves A alone; wire 2 moves B and with it H and pi_c (and A too: a public wire has its own A row)
    sc = {n: cf.proof_scalars(r1, bc.DEGEN_SEED, w, 0, 0) for n, w in wits.items()}
    assert sc['a_only'][0] != sc['zero'][0] and sc['a_only'][1] == sc['zero'][1] == beta % bc.R
    assert sc['b_only'][1] != beta % bc.R and sc['b_only'][2] != 0 == sc['zero'][2] == sc['a_only'][2]


def test_oracle_proves_the_foreign_witness():
    """The foreign vector of the batches ([1] + random: no witness of the circuit) goes through the oracle's prover like any other (the quotient is computed, not checked): rc = 0,
    so the GPU tests compare its proof with the oracle's bytes too.  The verifier refuses it, as it must."""
    import json
    from zkcensus_amd import setup
    _, zp, vp = setup.ensure_test_artifacts(bc.NL)
    zk = open(zp, 'rb').read()
    ws, foreign = bc.voter_witnesses()
    assert len(ws) == 65 and len(foreign) == len(ws[0])
    rc, proof, pub = ol.prove(zk, foreign, *bc.RANDOM_PAIR)
    assert rc == 0
    assert not ol.verify(json.load(open(vp)), pub, proof)
