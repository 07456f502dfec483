"""Helper of tests/test_00_gpu_msm_forms.py.  It runs as a child process, so that the process-wide ZKC_G2_* switches, which the library reads once, choose the form of the
G2 bucket accumulation.  It loads the nLevels-10 test key and runs zkc_msm_debug on sections A (G1) and B2 (G2) over the scalar sets of tests/msm_cases.py, in the order of
msm_cases.forms_scalars, and prints the result bytes as hex in one JSON line: {"0": [...], "2": [...]}.  With a directory as argv[1] it then does the same, after closing
the first key, for the generic key whose bases have coordinates at the edges of the field (msm_cases.edge_key, kept in that directory; its sets are
msm_cases.edge_forms_scalars): {"edge0": [...], "edge2": [...]} in the same line."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup
import oracle_lib as ol
import msm_cases as mc

_, zp, _ = setup.ensure_test_artifacts(mc.FORMS_NL)
zk = open(zp, 'rb').read()
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
z = ol.zkey_parse(zk)
out = {}
for which in mc.FORMS_SECTIONS:
    _, sets = mc.forms_scalars(z, which)
    out[str(which)] = []
    for scb in sets:
        d = torch.from_numpy(np.frombuffer(scb, dtype=np.uint8).copy()).cuda()
        out[str(which)].append(pk.msm_debug(which, d.data_ptr(), pk.n_vars).hex())
pk.close()
if len(sys.argv) > 1:
    zk = mc.edge_key(sys.argv[1])
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    z = ol.zkey_parse(zk)
    for which in mc.FORMS_SECTIONS:
        _, sets = mc.edge_forms_scalars(z, which)
        out['edge%d' % which] = []
        for scb in sets:
            d = torch.from_numpy(np.frombuffer(scb, dtype=np.uint8).copy()).cuda()
            out['edge%d' % which].append(pk.msm_debug(which, d.data_ptr(), pk.n_vars).hex())
    pk.close()
print(json.dumps(out))
ctx.close()
