"""Helper of tests/test_00_gpu_switches.py (a child process, so that the process-wide ZKC_FINALIZE_WAVES takes effect): proves the batches of 5 and of 65 proofs of
tests/blinding_cases.py -- edge (r, s) pairs; once with the foreign witness (an unfolded pass, keys "5" and "65") and once with voters only (a folded pass, "5f" and "65f") --
through a key loaded with ZKC_INFLIGHT=128, so that each batch is ONE pass, and prints the proof bytes as hex in one JSON line.  The witnesses are given (the groth16.prove shape); they come from the CPU oracle, the same bytes the parent proves on the CPU."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup
import blinding_cases as bc

_, zp, vp = setup.ensure_test_artifacts(bc.NL)
zk = open(zp, 'rb').read()
os.environ['ZKC_INFLIGHT'] = '128'
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
assert pk.pass_size == 128
out = {}
for n, foreign in ((5, True), (65, True), (5, False), (65, False)):
    wl, pairs, fi = bc.batch(n, with_foreign=foreign)
    d_w = torch.from_numpy(np.frombuffer(b''.join(wl), dtype=np.uint8).copy()).cuda()
    proofs, pubs = pk.prove_batch_dev(d_w.data_ptr(), n, bc.rs_bytes(pairs))
    out[str(n) + ('' if foreign else 'f')] = proofs.hex()
print(json.dumps(out))
pk.close(); ctx.close()
