"""Helper of tests/test_gpu_abc_rows.py.  It runs as a child process, so that the process-wide switch ZKC_ABC_FOLD (and ZKC_TRACE_HOST, which names the row lists a pass
takes on stderr) take effect.  It proves the batches of tests/abc_rows_cases.py, witnesses given and inputs given, then three voters and the foreign witness in one batch,
and prints the SHA-256 of each batch's proof and public-signal bytes."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup
import oracle_lib as ol
import abc_rows_cases as cases

nl = cases.NL
_, zp, vp = setup.ensure_test_artifacts(nl)
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read())
pool, rs, foreign = cases.build(ctx, ol.poseidon)
ws, st = ctx.witness(pool, nLevels=nl)
assert st == [0] * len(pool)
dev = lambda b: torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
nW = ctx.n_wires(nl)
out = []
for first, b in cases.BATCHES:
    rs_b = b''.join(rs[first:first + b])
    d_w = dev(b''.join(ws[first:first + b]))
    p, u = pk.prove_batch_dev(d_w.data_ptr(), b, rs_b)
    d_in = dev(b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in pool[first:first + b]))
    d_w2 = torch.empty(b * nW * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(b, dtype=torch.int32, device='cuda')
    assert pk.fullprove_batch_dev(d_in.data_ptr(), b, d_w2.data_ptr(), d_st.data_ptr(), rs_b) == (p, u)
    out.append(hashlib.sha256(p + u).hexdigest())
d_w = dev(b''.join(ws[5:8]) + foreign)
p, u = pk.prove_batch_dev(d_w.data_ptr(), 4, b''.join(rs[5:8]) + rs[cases.POOL])
out.append(hashlib.sha256(p + u).hexdigest())
print(json.dumps({'sha256': out}))
pk.close(); ctx.close()
