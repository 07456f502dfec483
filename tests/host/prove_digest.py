"""Helper of tests/test_00_gpu_switches.py.  It runs as a child process, so that process-wide ZKC_* switches, which the library reads once, take effect.
It proves a fixed batch of nLevels-10 voters, inputs -> witness -> proof: 70 voters (two passes with ZKC_INFLIGHT=40: full-pass code paths from 32 proofs on), then
the first 1, 2 and 40 of them, then voters 3 and 3..4 as a lone proof and a pair.  All (r, s) are fixed.  The first three voters blind with (0, 0), (0, k) and
(R - 1, R - 1); the others, the second lone proof and pair among them, with random scalars.  Prints the SHA-256 of all proof and public-signal bytes."""
import hashlib, json, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup
from census_gen import random_voter
import synth_voter

nl, B = 10, 70
_, zp, vp = setup.ensure_test_artifacts(nl)
zk = open(zp, 'rb').read()
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
rng = random.Random(20261004)
H = lambda xs: synth_voter.H(*xs)
voters = [random_voter(rng, H, nLevels=nl, depth_c=rng.randint(0, nl), depth_s=rng.randint(0, nl)) for _ in range(B)]
flat = b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in voters)
rs = b''.join(rng.randrange(1 << 250).to_bytes(32, 'little') for _ in range(2 * B))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
edge = [(0, 0), (0, rng.randrange(1, R)), (R - 1, R - 1)]          # the first three proofs of every batch blind with a zero r, a zero s and the largest scalars
rs = b''.join(x.to_bytes(32, 'little') for p in edge for x in p) + rs[64 * len(edge):]
d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
d_w = torch.empty(B * ctx.n_wires(nl) * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(B, dtype=torch.int32, device='cuda')
h = hashlib.sha256()
ctx.witness_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_st.data_ptr(), nLevels=nl)
assert int(d_st.abs().sum().item()) == 0
nofold_key = os.environ.get('ZKC_NO_FOLD') is not None           # such a key is not recognised as a census key: the witnesses are given (groth16.prove shape)
nW, nIn = ctx.n_wires(nl), ctx.n_inputs(nl)
for b, first in ((B, 0), (1, 0), (2, 0), (40, 0), (1, 3), (2, 3)):          # the last two: passes of one and two proofs with non-zero random r and s
    rs_b = rs[64 * first:64 * (first + b)]
    p, u = pk.prove_batch_dev(d_w.data_ptr() + first * nW * 32, b, rs_b)
    h.update(p); h.update(u)
    if not nofold_key:                                          # inputs -> witness -> proof in one call: the same bytes
        d_w2 = torch.empty(b * nW * 32, dtype=torch.uint8, device='cuda')
        assert pk.fullprove_batch_dev(d_in.data_ptr() + first * nIn * 32, b, d_w2.data_ptr(), d_st.data_ptr(), rs_b) == (p, u)
print(json.dumps({'sha256': h.hexdigest()}))
pk.close(); ctx.close()
