"""GPU: the three forms of the blinding step (csrc/zkc_finalize.hip, Groth16 stage a7) at the values where a scalar product or an addition with infinity goes wrong.

  lane per product   zkc_finalize_products / _combine: every pass of three proofs or more -- the batch path, the service, bench.py.  Batches of 3, 4, 5 (either side of the
                     "more than four proofs" reduction windows), 64 and 65 proofs; the last two through a key loaded with ZKC_INFLIGHT=128, so that 65 proofs are ONE pass and
                     proof 64 is the first lane of the second 64-lane block of both kernels (the q >= nq guard, the tabs + (task nq + q) 16 scratch layout)
  tree               zkc_blind_tree_*: passes of one or two proofs on the default key
  wave per task      zkc_finalize: passes of one or two proofs on a key loaded with ZKC_BLIND_TREE=0 (and every pass under ZKC_FINALIZE_WAVES: tests/test_00_gpu_switches.py)

Every batch carries the edge (r, s) list of tests/blinding_cases.py -- r = 0, s = 0, r s = +-1, only the top 4-bit window, every window 0xF, single windows -- laid out so that
proofs 0, 1, 63, 64 and the last one hold an edge pair, and one FOREIGN witness ([1] + random) that gets no fold constants.  A pass of given witnesses that holds a foreign one is
unfolded as a whole (zkc_prove.hip: dc = 255 for every proof, fold_const returns infinity; blinding_cases.voter_witnesses asserts that the foreign vector differs from every
voter in the block that decides it), so each batch is proved a second time with a voter in the foreign slot: that pass is
folded, and every other proof must come out the same.  References: the CPU oracle (ol.prove, byte equality, every proof; ol.verify for every voter's proof) and, for the generic
key, the toxic-waste closed form.  The oracle proves the foreign witness too (rc = 0, tests/test_blinding_refs_cpu.py), so it stays in the comparison.  No tolerances anywhere."""
import json, os
import pytest
import oracle_lib as ol
import closed_form as cf
import blinding_cases as bc

pytestmark = pytest.mark.gpu
SIZES = (3, 4, 5, 64, 65)


def _load_with(zkc, ctx, zk, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return zkc.ProvingKey(ctx, zk)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.fixture(scope='module')
def env():
    import torch  # noqa: F401
    import zkcensus_amd as zkc
    from zkcensus_amd import setup
    _, zp, vp = setup.ensure_test_artifacts(bc.NL)
    zk = open(zp, 'rb').read()
    ctx = zkc.Context(0)
    keys = {'default': zkc.ProvingKey(ctx, zk), 'one_pass': _load_with(zkc, ctx, zk, ZKC_INFLIGHT='128'), 'general': _load_with(zkc, ctx, zk, ZKC_BLIND_TREE='0')}
    assert keys['default'].pass_size == 64 and keys['one_pass'].pass_size == 128
    yield zkc, ctx, keys, zk, json.load(open(vp))
    for k in keys.values():
        k.close()
    ctx.close()


def _dev(wl):
    import torch, numpy as np
    return torch.from_numpy(np.frombuffer(b''.join(wl), dtype=np.uint8).copy()).cuda()


_oracle = {}


def oracle_proofs(zk, vk, wl, pairs, voters):
    """ol.prove for every (witness, r, s), on host threads, computed once per distinct triple; a voter's proof is also put to the pinned verifier"""
    def one(job):
        w, (r, s), accepted = job
        rc, proof, pub = ol.prove(zk, w, r, s)
        assert rc == 0
        assert not accepted or ol.verify(vk, pub, proof), (r, s)
        return proof
    todo = {}
    for w, p, v in zip(wl, pairs, voters):
        if (w, p) not in _oracle:
            todo[(w, p)] = (w, p, v)
    for key, proof in zip(todo, ol.pmap(one, todo.values())):
        _oracle[key] = proof
    return [_oracle[(w, p)] for w, p in zip(wl, pairs)]


@pytest.mark.parametrize('n', SIZES)
def test_batches_at_scalar_edges_equal_the_oracle(env, n):
    """The production form.  Observed on one MI355X box with a 16-core CPU share: the batch of 65 takes 4.6 s and the batch of 64 3.5 s, nearly all of it the oracle's
    CPU proofs under ol.pmap (130 lone proofs and six pairs in the test below take 0.34 s in all); the batches of 3, 4 and 5 take 1.9 s each."""
    zkc, ctx, keys, zk, vk = env
    pk = keys['one_pass'] if n >= 64 else keys['default']
    wl, pairs, fi = bc.batch(n)
    d_w = _dev(wl)
    proofs, pubs = pk.prove_batch_dev(d_w.data_ptr(), n, bc.rs_bytes(pairs))
    want = oracle_proofs(zk, vk, wl, pairs, [q != fi for q in range(n)])
    for q in range(n):
        assert proofs[256 * q:256 * q + 256] == want[q], (n, q, pairs[q], 'foreign' if q == fi else 'voter')
        assert pubs[256 * q:256 * q + 256] == wl[q][32:32 + 256]
    # the same batch with a voter in the foreign slot: a folded pass (fold_const finite for every proof); the other proofs do not change by a byte
    wl2, _, _ = bc.batch(n, with_foreign=False)
    d_w2 = _dev(wl2)
    proofs2, _ = pk.prove_batch_dev(d_w2.data_ptr(), n, bc.rs_bytes(pairs))
    want2 = oracle_proofs(zk, vk, wl2, pairs, [True] * n)
    for q in range(n):
        assert proofs2[256 * q:256 * q + 256] == want2[q], (n, q, pairs[q], 'folded pass')
    if n == 65:                                        # and as 33 + 32 on the default key
        assert keys['default'].prove_batch_dev(d_w.data_ptr(), n, bc.rs_bytes(pairs))[0] == proofs


def test_each_proof_alone_in_the_tree_and_the_wave_form(env):
    """Every proof of the batch of 65 proved alone with its (r, s): the default key takes the tree form, the ZKC_BLIND_TREE=0 key zkc_finalize; both give the batch's bytes
    (the oracle's).  Then pairs of proofs (passes of two), and the batch of 3 through the ZKC_BLIND_TREE=0 key, whose passes of three take the lane-per-product form like any."""
    zkc, ctx, keys, zk, vk = env
    wl, pairs, fi = bc.batch(65)
    want = oracle_proofs(zk, vk, wl, pairs, [q != fi for q in range(65)])
    d_w = _dev(wl)
    nW = len(wl[0])
    for q in range(65):
        rs = bc.rs_bytes(pairs[q:q + 1])
        for form in ('default', 'general'):
            assert keys[form].prove_batch_dev(d_w.data_ptr() + q * nW, 1, rs)[0] == want[q], (form, q, pairs[q])
    for q in (0, 12, 63):                               # passes of two; (63, 64) is a voter beside the foreign witness
        rs = bc.rs_bytes(pairs[q:q + 2])
        for form in ('default', 'general'):
            assert keys[form].prove_batch_dev(d_w.data_ptr() + q * nW, 2, rs)[0] == want[q] + want[q + 1], (form, q)
    wl3, pairs3, _ = bc.batch(3)
    d_w3 = _dev(wl3)
    assert keys['general'].prove_batch_dev(d_w3.data_ptr(), 3, bc.rs_bytes(pairs3)) == keys['default'].prove_batch_dev(d_w3.data_ptr(), 3, bc.rs_bytes(pairs3))


def test_degenerate_operands_on_a_generic_key(env, tmp_path):
    """MSM results at infinity (tests/blinding_cases.degenerate_instance): the witness (1, 0, .., 0) leaves B1', B2', C' and H at infinity, so r B1' starts from P.is_inf(), every
    sum of the combine step adds infinity operands, and at (r, s) = (0, 0) pi_c itself is infinity: 64 zero bytes, as both references write it (tests/test_blinding_refs_cpu.py).
    There A' is finite (wire 0 has an A polynomial from snarkjs' public-input rows); the 'a_inf' witness cancels it with wire 1, so that A' is infinity too: s A' starts from
    P.is_inf(), pi_a = alpha + r delta is an addition of the affine alpha1 to infinity, and at (0, 0) the proof is (alpha1, beta2, infinity).  Two more witnesses with one
    non-zero wire: A' alone changes; B1', B2' and H alone are finite.  Each alone in the tree form and in zkc_finalize, and as three copies with three edge pairs in one pass; expected bytes from the closed form."""
    zkc, ctx, keys, zk, vk = env
    r1, wits = bc.degenerate_instance(tmp_path)
    gzk, gvk = bc.setup_key(r1)
    forms = {'default': zkc.ProvingKey(ctx, gzk), 'general': _load_with(zkc, ctx, gzk, ZKC_BLIND_TREE='0')}
    try:
        for name, w in wits.items():
            want = {}
            for r, s in bc.DEGEN_PAIRS:
                a, b, c = cf.proof_scalars(r1, bc.DEGEN_SEED, w, r, s)
                want[(r, s)] = cf.proof_from_scalars(ol, a, b, c)
                for form, pk in forms.items():
                    proof, pub = pk.prove(w, r, s)
                    assert proof == want[(r, s)], (name, form, r, s)
                    assert pub == w[32:32 * (1 + bc.DEGEN_PUB)]
            assert (want[(0, 0)][192:] == bytes(64)) == (name != 'b_only')
            if name == 'a_inf':
                assert want[(0, 0)] == ol.g1_json(gvk['vk_alpha_1']) + ol.g2_json(gvk['vk_beta_2']) + bytes(64)
            d_w = _dev([w] * 3)
            for trio in (bc.DEGEN_PAIRS[0:3], bc.DEGEN_PAIRS[3:6], [bc.DEGEN_PAIRS[6], bc.DEGEN_PAIRS[1], bc.DEGEN_PAIRS[0]]):      # (0, 0) first, and last
                for form, pk in forms.items():
                    assert pk.prove_batch_dev(d_w.data_ptr(), 3, bc.rs_bytes(trio))[0] == b''.join(want[p] for p in trio), (name, form, trio)
    finally:
        for pk in forms.values():
            pk.close()
