"""GPU: the transforms at every size they split differently, and the prove entry points' refusal of unreduced host witnesses.

- zkc_ntt_dev (ntt_run: its stage split changes with every logn) forward AND inverse at each logn from 3 to 20 against the oracle's transform, on
  three different vectors in one call (nvec = 3): random; an edge vector (zeros, r - 1, deltas at 0 and n - 1); a constant.  Each output vector
  is checked against its own reference, so a mix-up of the per-vector offset shows.
- The prover's transform pair (ntt_pair_run, taken from a 2^12 domain on; ntt_run below): h evaluations against the oracle at every domain from 2^9
  to 2^16, and full proofs on both sides of the switch (2^11, 2^12) against the toxic-waste closed form and the verifier.
- A host witness with a value >= r is refused (ZKC_ERR_FORMAT, the wire named) by ProvingKey.prove and the proving service, for a generic key whose
  sections take 15-bit windows and for a lone census proof (8-bit G2 windows), before any work on the device; the reduced witness proves byte-equal
  to the oracle."""
import random
import pytest
import oracle_lib as ol
import closed_form as cf
import big_circuit as bc
from test_generic_circuit import setup_key

pytestmark = pytest.mark.gpu
R = ol.R
RM = 1 << 256


def _dev(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


def _mont(vals):
    return b''.join((v * RM % R).to_bytes(32, 'little') for v in vals)


@pytest.mark.parametrize('logn', list(range(3, 21)))
def test_ntt_every_size_three_vectors(gpu, logn):
    ctx, torch = gpu
    from zkcensus_amd import engines
    n = 1 << logn
    rng = random.Random(1000 + logn)
    rand = [rng.randrange(R) for _ in range(n)]
    edge = [0] * (n // 2) + [R - 1] * (n // 2)
    edge[0] = 1; edge[n - 1] = 1; edge[n // 2] = 0                                  # deltas at 0 and n - 1 inside the zero / r - 1 halves
    const = [rng.randrange(1, R)] * n
    vecs = [rand, edge, const]
    src = _dev(torch, b''.join(_mont(v) for v in vecs))
    step = max(1, n // (1 << 16))                                                    # every element up to 2^16, a stride above
    idx = sorted(set(range(0, n, step)) | {1, n - 1})
    for inverse in (0, 1):
        dst = torch.empty_like(src)
        (engines.ifft if inverse else engines.fft)(ctx, src.data_ptr(), dst.data_ptr(), logn, nvec=3)
        torch.cuda.synchronize()
        got = dst.cpu().numpy().tobytes()
        for k, v in enumerate(vecs):
            exp = ol.ntt(v, inverse=bool(inverse))
            base = 32 * n * k
            for i in idx:
                assert got[base + 32 * i:base + 32 * i + 32] == (exp[i] * RM % R).to_bytes(32, 'little'), \
                    '%s NTT 2^%d, vector %d, element %d' % ('inverse' if inverse else 'forward', logn, k, i)


def _wide_key(tmp_path, logn, n_wires=600, n_pub=2):
    """few wires, many rows: a key whose domain is 2^logn"""
    n_cons = (1 << logn) - (1 << (logn - 3))
    r1 = str(tmp_path / ('wide%d.r1cs' % logn))
    w = bc.big_instance(r1, n_cons, n_wires, n_pub, seed=logn)
    zk, vk = setup_key(r1, 4242 + logn)
    return r1, w, zk, vk


@pytest.mark.parametrize('logn', list(range(9, 17)))
def test_transform_pair_every_domain(gpu, tmp_path, logn):
    ctx, torch = gpu
    import zkcensus_amd
    r1, w, zk, vk = _wide_key(tmp_path, logn)
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    try:
        assert pk.domain_size == 1 << logn
        assert pk.debug_stage(_dev(torch, w).data_ptr(), 1) == ol.h_evals(zk, w), 'h evaluations on the odd coset, domain 2^%d' % logn
        if logn in (11, 12):                                                        # ntt_run below 2^12, the transform pair from 2^12 on
            proof, pub = pk.prove(w, 17, 19)
            a, b, c = cf.proof_scalars(r1, 4242 + logn, w, 17, 19)
            assert proof == cf.proof_from_scalars(ol, a, b, c), 'proof at domain 2^%d differs from the closed form' % logn
            assert ol.verify(vk, pub, proof)
    finally:
        pk.close()


def _bad_at(w, wire, add):
    v = int.from_bytes(w[32 * wire:32 * wire + 32], 'little') + add
    return w[:32 * wire] + v.to_bytes(32, 'little') + w[32 * wire + 32:]


def _refused(fn, code=5):
    import zkcensus_amd
    with pytest.raises(zkcensus_amd.ZkcError) as ei:
        fn()
    assert ei.value.code == code and 'wire 5 ' in str(ei.value), str(ei.value)


def test_unreduced_witness_refused_generic_c15(gpu, tmp_path):
    """23 000 wires: the key's sections take 15-bit windows, whose digits cannot hold a value of 2^255 and more"""
    ctx, torch = gpu
    import zkcensus_amd
    n_pub = 2
    r1 = str(tmp_path / 'c15.r1cs')
    w = bc.big_instance(r1, 3000, 23000, n_pub, seed=15)
    zk, vk = setup_key(r1, 1515)
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    try:
        assert pk.n_vars == 23000
        for add in (1 << 255, R, (1 << 256) - 1 - int.from_bytes(w[160:192], 'little')):
            _refused(lambda: pk.prove(_bad_at(w, 5, add), 3, 5))
        svc = zkcensus_amd.ProvingService([0])
        try:
            _refused(lambda: svc.prove(zk, _bad_at(w, 5, 1 << 255), rs=(3).to_bytes(32, 'little') + (5).to_bytes(32, 'little'), n_public=n_pub))
        finally:
            svc.close()
        proof, pub = pk.prove(w, 3, 5)                                              # the reduced witness: byte-equal to the oracle
        rc, oproof, opub = ol.prove(zk, w, 3, 5, npub=n_pub)
        assert rc == 0 and proof == oproof and pub == opub
        assert ol.verify(vk, pub, proof)
    finally:
        pk.close()


def test_unreduced_witness_refused_lone_census_proof(gpu):
    """a lone census proof takes the 8-bit G2 table, whose 32 windows read 256 bits and drop the top carry"""
    ctx, torch = gpu
    import sys, os, json
    import zkcensus_amd
    from zkcensus_amd import setup
    sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
    from census_gen import random_voter
    _, zkey_path, vkey_path = setup.ensure_test_artifacts(10)
    zk = open(zkey_path, 'rb').read()
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    try:
        voter = random_voter(random.Random(55), ol.poseidon, nLevels=10, depth_c=6, depth_s=4)
        rc, w = ol.witness(voter, nLevels=10)
        assert rc == 0
        _refused(lambda: pk.prove(_bad_at(w, 5, 1 << 255), 12345, 67890))
        _refused(lambda: pk.prove(_bad_at(w, 5, R), 12345, 67890))
        proof, pub = pk.prove(w, 12345, 67890)
        rc, oproof, opub = ol.prove(zk, w, 12345, 67890)
        assert rc == 0 and proof == oproof and pub == opub
        assert ol.verify(json.load(open(vkey_path)), pub, proof)
    finally:
        pk.close()
