"""GPU: buildABC of a folded pass copies the rows no voter of the pass can change from the key's template abc and computes the voter rows only (csrc/zkc_abc_rows.h,
ZKC_ABC_FOLD).  Through the public prove calls at nLevels = 10, against the CPU oracle's proof bytes (the oracle computes every row of every proof): passes that mix the
shallowest and the deepest voters, the early layout of one and two proofs, five proofs whose two pass depths come from different proofs, 65 proofs in two passes, a foreign
witness that unfolds its pass, a folded call after an unfolded one on the same key; the same batches with the switch off in a child process; and at nLevels = 160 two call
slots in flight over the lanes that share the template block."""
import json, os, subprocess, sys
import pytest
import oracle_lib as ol
import abc_rows_cases as cases

pytestmark = pytest.mark.gpu
NL = cases.NL


def dev_bytes(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope='module')
def env():
    """the nLevels = 10 key, the pool's witnesses, and the oracle's proof of every pool voter and of the foreign witness: computed once, shared, never changed"""
    import torch, zkcensus_amd
    from zkcensus_amd import setup
    ctx = zkcensus_amd.Context(0)
    _, zp, vp = setup.ensure_test_artifacts(NL)
    zk = open(zp, 'rb').read()
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    pool, rs, foreign = cases.build(ctx, ol.poseidon)
    ws, st = ctx.witness(pool, nLevels=NL)
    assert st == [0] * cases.POOL
    ws = ws + [foreign]
    num = lambda b: int.from_bytes(b, 'little')

    def oracle(i):
        rc, p, u = ol.prove(zk, ws[i], num(rs[i][:32]), num(rs[i][32:]))
        assert rc == 0
        return p, u
    want = ol.pmap(oracle, range(cases.POOL + 1))
    yield ctx, pk, torch, pool, ws, rs, want
    pk.close(); ctx.close()


def prove_both_ways(env, first, b):
    """witnesses given (laid out from the fold flags) and inputs given (a one-pass call is laid out early, from its inputs' depths): the same bytes"""
    ctx, pk, torch, pool, ws, rs, want = env
    import zkcensus_amd
    rs_b = b''.join(rs[first:first + b])
    got = pk.prove_batch_dev(dev_bytes(torch, b''.join(ws[first:first + b])).data_ptr(), b, rs_b)
    d_in = dev_bytes(torch, b''.join(zkcensus_amd.flatten_inputs(v, NL) for v in pool[first:first + b]))
    d_w = torch.empty(b * ctx.n_wires(NL) * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(b, dtype=torch.int32, device='cuda')
    assert pk.fullprove_batch_dev(d_in.data_ptr(), b, d_w.data_ptr(), d_st.data_ptr(), rs_b) == got
    assert d_st.cpu().tolist() == [0] * b
    return got


def test_pool_holds_the_depths_it_is_meant_to(env):
    _, _, _, pool, _, _, _ = env
    d = [(cases.depth_of(v, 'censusSiblings'), cases.depth_of(v, 'sikSiblings')) for v in pool]
    assert d[1] == (NL, NL) and max(d[0]) < NL - 2                       # deepest and shallowest side by side
    assert d[3][0] > d[4][0] and d[4][1] > d[3][1]                       # voters 2 .. 4 as one pass: its census depth is voter 3's, its sik depth voter 4's
    assert max(x[0] for x in d[2:5]) == d[3][0] and max(x[1] for x in d[2:5]) == d[4][1]


@pytest.mark.parametrize('first,b', cases.BATCHES + ((2, 3),), ids=lambda x: str(x))
def test_folded_batches_equal_the_oracle(env, first, b):
    want = env[6]
    proofs, pubs = prove_both_ways(env, first, b)
    for i in range(b):
        assert (proofs[256 * i:256 * i + 256], pubs[256 * i:256 * i + 256]) == want[first + i], 'voter %d' % (first + i)


def test_foreign_witness_unfolds_its_pass_and_the_template_block_survives(env):
    ctx, pk, torch, pool, ws, rs, want = env
    folded = prove_both_ways(env, 0, 5)
    idx = [5, 6, 7, cases.POOL]                                          # three voters and the foreign witness: the pass computes every row
    proofs, pubs = pk.prove_batch_dev(dev_bytes(torch, b''.join(ws[i] for i in idx)).data_ptr(), 4, b''.join(rs[i] for i in idx))
    for k, i in enumerate(idx):
        assert (proofs[256 * k:256 * k + 256], pubs[256 * k:256 * k + 256]) == want[i], 'voter %d' % i
    assert prove_both_ways(env, 0, 5) == folded                          # nothing of the key's template abc was written by the unfolded pass
    assert folded[0] == b''.join(want[i][0] for i in range(5))


def _child(cfg):
    envp = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
    envp.update(cfg)
    r = subprocess.run([sys.executable, os.path.join(ol.ROOT, 'tests', 'host', 'abc_rows_digest.py')], env=envp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (cfg, r.returncode, r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])['sha256'], r.stderr


def test_switch_off_gives_the_same_bytes_and_the_default_takes_the_lists(env):
    import hashlib
    want = env[6]
    digests = [hashlib.sha256(b''.join(want[i][0] for i in range(f, f + b)) + b''.join(want[i][1] for i in range(f, f + b))).hexdigest() for f, b in cases.BATCHES]
    idx = [5, 6, 7, cases.POOL]
    digests.append(hashlib.sha256(b''.join(want[i][0] for i in idx) + b''.join(want[i][1] for i in idx)).hexdigest())
    off, err_off = _child({'ZKC_ABC_FOLD': '0', 'ZKC_TRACE_HOST': '1'})
    assert off == digests
    assert 'abc rows' not in err_off                                     # off: no row classes, no lists
    on, err_on = _child({'ZKC_TRACE_HOST': '1'})
    assert on == digests
    assert 'A/B rows never constant' in err_on and 'abc rows at depths (%d, %d)' % (NL, NL) in err_on      # the pass with the deep voter


def test_two_call_slots_share_the_template_block_nl160():
    """Six voters of the benchmark's census at nLevels = 160 through zkc_batch_begin / zkc_batch_finish: two call slots in flight, four times, each call with witness and
    status buffers of its own -- the bytes of the call alone, which the pinned verifier accepts and of which the oracle re-proves one."""
    import json as js, random, torch, zkcensus_amd
    from zkcensus_amd import census, setup
    nl, B = 160, 6
    ctx = zkcensus_amd.Context(0)
    _, zp, vp = setup.ensure_test_artifacts(nl)
    zk = open(zp, 'rb').read(); vk = js.load(open(vp))
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    try:
        voters = census.synthetic_census(ctx, 8192, nl)[1000:1000 + B]
        d_in = dev_bytes(torch, b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in voters))
        nW = ctx.n_wires(nl)
        d_w = [torch.zeros(B * nW * 32, dtype=torch.uint8, device='cuda') for _ in range(2)]; d_st = [torch.zeros(B, dtype=torch.int32, device='cuda') for _ in range(2)]
        rng = random.Random(166)
        rs = b''.join(rng.randrange(ol.R).to_bytes(32, 'little') for _ in range(2 * B))
        alone = pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w[0].data_ptr(), d_st[0].data_ptr(), rs)
        assert d_st[0].cpu().tolist() == [0] * B
        for i in range(B):
            assert ol.verify(vk, alone[1][256 * i:256 * i + 256], alone[0][256 * i:256 * i + 256]), i
        w3 = d_w[0].view(B, nW * 32)[3].cpu().numpy().tobytes()
        rc, op, opub = ol.prove(zk, w3, int.from_bytes(rs[64 * 3:64 * 3 + 32], 'little'), int.from_bytes(rs[64 * 3 + 32:64 * 4], 'little'))
        assert rc == 0 and (op, opub) == (alone[0][256 * 3:256 * 4], alone[1][256 * 3:256 * 4])
        for _ in range(4):
            pk.batch_begin(0, d_in.data_ptr(), B, d_w[0].data_ptr(), d_st[0].data_ptr(), rs)
            pk.batch_begin(1, d_in.data_ptr(), B, d_w[1].data_ptr(), d_st[1].data_ptr(), rs)
            assert pk.batch_finish(0, B) == alone and pk.batch_finish(1, B) == alone
    finally:
        pk.close(); ctx.close()
