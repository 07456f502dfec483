"""GPU: the witness kernels (wave per path, lane per path), the prover (batch path folded and unfolded, lone path with its early layout, nLevels = 253) at the value edges
of tests/edge_voters.py -- address 0 and addresses of 253 / 254 bits, weights at and above 2^252 (the accepted wrap included), password / signature / electionId 0 and r - 1,
siblings r - 1, 1 and a single one at the top.  tests/test_witness_edges_cpu.py shows that the CPU oracle's status and witness for each of them are the circuit's; here every
status, witness, proof and public-signal block of the kernels must equal the oracle's bytes."""
import json, os, random
import pytest
import oracle_lib as ol
import edge_voters as ev

pytestmark = pytest.mark.gpu
R = ol.R
NL = 10


@pytest.fixture(scope='module')
def env():
    import torch, zkcensus_amd
    from zkcensus_amd import setup
    ctx = zkcensus_amd.Context(0)
    keys = {}

    def get(nl, nofold=False):                      # one load per key and module
        if (nl, nofold) not in keys:
            _, zp, vp = setup.ensure_test_artifacts(nl)
            zk = open(zp, 'rb').read()
            if nofold:
                os.environ['ZKC_NO_FOLD'] = '1'     # read when the key is loaded: the key is not recognised as the census circuit, every pass runs unfolded
            try:
                pk = zkcensus_amd.ProvingKey(ctx, zk)
            finally:
                os.environ.pop('ZKC_NO_FOLD', None)
            keys[(nl, nofold)] = (zk, pk, json.load(open(vp)))
        return keys[(nl, nofold)]
    yield ctx, get, torch
    for _, pk, _ in keys.values():
        pk.close()
    ctx.close()


_ORACLE = {}


def oracle_witnesses(nl, cases):
    """[(status, witness bytes)] of the CPU oracle, on host threads; those of the nLevels = 10 list are computed once for the module."""
    todo = [c for c in cases if (nl, c[0]) not in _ORACLE]
    got = dict(_ORACLE)
    for c, res in zip(todo, ol.pmap(lambda c: ol.witness(c[1], nLevels=nl), todo)):
        got[(nl, c[0])] = res
        if nl == NL:
            _ORACLE[(nl, c[0])] = res
    return [got[(nl, c[0])] for c in cases]


def dev_bytes(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def rs_bytes(rs):
    return b''.join(ol.le32(r) + ol.le32(s) for r, s in rs)


def fullprove(env, pk, nl, voters, rs):
    """zkc_fullprove_batch_dev over `voters`: (statuses, witnesses, proofs, public-signal blocks), one entry per voter"""
    import zkcensus_amd
    ctx, _, torch = env
    B, nW = len(voters), ctx.n_wires(nl)
    d_in = dev_bytes(torch, b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in voters))
    d_w = torch.zeros(B * nW * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(B, dtype=torch.int32, device='cuda')
    proofs, pubs = pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_st.data_ptr(), rs_bytes(rs))
    w = d_w.view(B, nW * 32).cpu().numpy()
    return d_st.cpu().tolist(), [w[i].tobytes() for i in range(B)], [proofs[256 * i:256 * i + 256] for i in range(B)], [pubs[256 * i:256 * i + 256] for i in range(B)]


def oracle_proofs(zk, wits, rs):
    def one(k):
        rc, proof, pub = ol.prove(zk, wits[k], rs[k][0], rs[k][1])
        assert rc == 0, k
        return proof, pub
    return ol.pmap(one, range(len(wits)))


def wave_cases(nl):
    if nl == 253:                                   # every key bit steers a level; bit 253 is the solved one
        return list(ev.address_cases(253, 253)) + list(ev.address_cases(253, 3))
    return ev.all_cases(nl)


@pytest.mark.parametrize('nl', [10, 160, 253])
def test_wave_kernel_vs_oracle(env, nl):
    """The stand-alone entry takes the wave-per-path kernel (up to 1024 voters): status and every wire of every voter, the rejected ones included (a weight
    failure stops nothing: all wires are defined)."""
    ctx, _, _ = env
    cases = wave_cases(nl)
    assert len(cases) == (24 if nl == 253 else 40)
    ws, st = ctx.witness([c[1] for c in cases], nLevels=nl)
    exp = oracle_witnesses(nl, cases)
    assert st == [c[2] for c in cases] == [e[0] for e in exp]
    for c, w, e in zip(cases, ws, exp):
        assert w == e[1], (nl, c[0])


def test_lane_kernel_vs_wave_and_oracle(env):
    """The lane-per-path kernel, reached as in test_gpu_witness.py: test_lane_and_wave_kernels_agree -- through the witness stage of zkc_fullprove_batch_dev, whose launches of more
    than 128 voters take it (the first pass of a call has a launch of its own, the passes behind it share one).  300 voters = the case list cycled; voters 150..299 are
    compared.  The rejected voters fail alone, with the circuit's status, and every neighbour's witness is the oracle's."""
    ctx, get, _ = env
    zk, pk, vk = get(NL)
    cases = ev.all_cases(NL)
    B = 300
    npasses = -(-B // pk.pass_size); per = -(-B // npasses)
    # launches: one pass -> all 300 voters together; otherwise pass 0 alone, then passes 1..7 together (zkc_prove.hip prove_batch_begin, ZKC_WITNESS_GROUP = 8)
    assert npasses <= 8 and (npasses == 1 or (per <= 150 and B - per > 128)), 'voters 150..299 would not all come from the lane kernel'
    many = [cases[i % len(cases)] for i in range(B)]
    st, wits, _, _ = fullprove(env, pk, NL, [c[1] for c in many], [(0, 0)] * B)
    ws_wave, st_wave = ctx.witness([c[1] for c in cases], nLevels=NL)
    exp = oracle_witnesses(NL, cases)
    assert st == [c[2] for c in many]
    assert sum(1 for s in st[150:] if s) >= 15                                   # the six rejected pairs, three to four times each
    for i in range(150, B):
        k = i % len(cases)
        assert st[i] == st_wave[k] == exp[k][0], (i, cases[k][0])
        assert wits[i] == ws_wave[k] == exp[k][1], (i, cases[k][0])


@pytest.fixture(scope='module')
def batch(env):
    """The accepted cases in ONE zkc_fullprove_batch_dev call on the folded key, (r, s) random with (0, 0) and (r - 1, r - 1) among them."""
    _, get, _ = env
    zk, pk, vk = get(NL)
    cases = [c for c in ev.all_cases(NL) if c[2] == 0]
    assert len(cases) == 34
    rng = random.Random(20261017)
    rs = [(0, 0), (R - 1, R - 1), (0, R - 1)] + [(rng.randrange(R), rng.randrange(R)) for _ in range(len(cases) - 3)]
    return cases, rs, fullprove(env, pk, NL, [c[1] for c in cases], rs)


def test_prover_batch_path_vs_oracle(env, batch):
    _, get, _ = env
    zk, pk, vk = get(NL)
    cases, rs, (st, wits, proofs, pubs) = batch
    exp = oracle_witnesses(NL, cases)
    assert st == [0] * len(cases)
    for c, w, e in zip(cases, wits, exp):
        assert e[0] == 0 and w == e[1], c[0]
    want = oracle_proofs(zk, [e[1] for e in exp], rs)
    for k, c in enumerate(cases):
        assert (proofs[k], pubs[k]) == want[k], c[0]
    assert all(ol.pmap(lambda k: ol.verify(vk, pubs[k], proofs[k]), range(len(cases))))


def test_prover_batch_unfolded_equals_folded(env, batch):
    """The same batch on a key loaded with ZKC_NO_FOLD=1 (not recognised as the census circuit: no level of any voter is replaced by the template's constant, and
    zkc_fullprove_batch_dev refuses it, so the witnesses of the folded call go in through zkc_prove_batch_dev): the same bytes."""
    _, get, torch = env
    _, pk_nofold, _ = get(NL, nofold=True)
    cases, rs, (st, wits, proofs, pubs) = batch
    B = len(cases)
    proofs2, pubs2 = pk_nofold.prove_batch_dev(dev_bytes(torch, b''.join(wits)).data_ptr(), B, rs_bytes(rs))
    for k, c in enumerate(cases):
        assert proofs2[256 * k:256 * k + 256] == proofs[k] and pubs2[256 * k:256 * k + 256] == pubs[k], c[0]


def test_prover_lone_path_vs_oracle(env):
    """Calls of one and of two voters: laid out early from zkc_input_depths (before the witness exists), blinded by the tree form, G2 through the 8-bit-window table.
    Every voter is proved alone, first in a pair and second in a pair."""
    _, get, _ = env
    zk, pk, vk = get(NL)
    cases = ev.by_name(ev.all_cases(NL), 'addr_0@d3', 'addr_2^253@d3', 'addr_r-1@d3', ev.weight_name(*ev.WRAP), 'sibling_top_only')
    rng = random.Random(5)
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in cases]
    exp = oracle_witnesses(NL, cases)
    want = oracle_proofs(zk, [e[1] for e in exp], rs)
    n = len(cases)
    for idx in [(k,) for k in range(n)] + [(k, (k + 1) % n) for k in range(n)]:
        st, wits, proofs, pubs = fullprove(env, pk, NL, [cases[k][1] for k in idx], [rs[k] for k in idx])
        assert st == [0] * len(idx), idx
        for j, k in enumerate(idx):
            assert wits[j] == exp[k][1] and (proofs[j], pubs[j]) == want[k], (idx, cases[k][0])
    assert all(ol.verify(vk, pub, proof) for proof, pub in want)


def test_prover_nl253_vs_oracle(env):
    """nLevels = 253: address 2^253 at depth 253 (nothing folds; the key's top bit is the solved one) and address 0 at depth 0 (everything folds, key0)."""
    ctx, get, _ = env
    nl = 253
    zk, pk, vk = get(nl)
    cases = ev.by_name(ev.address_cases(nl, 253), 'addr_2^253@d253') + ev.by_name(ev.address_cases(nl, 0), 'addr_0@d0')
    assert [int(x) for x in cases[1][1]['censusSiblings']] == [0] * 254
    ws, st = ctx.witness([c[1] for c in cases], nLevels=nl)
    exp = oracle_witnesses(nl, cases)
    assert st == [0, 0] == [e[0] for e in exp] and ws == [e[1] for e in exp]
    rs = [(R - 1, 1), (12345, 0)]
    gpu = [pk.prove(w, r, s) for w, (r, s) in zip(ws, rs)]
    want = oracle_proofs(zk, ws, rs)
    for k in range(2):
        assert gpu[k] == want[k], cases[k][0]
        assert ol.verify(vk, gpu[k][1], gpu[k][0])
