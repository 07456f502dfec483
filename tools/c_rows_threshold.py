#!/usr/bin/env python3
"""Up to how many listed C rows does a pass gain from leaving out the transform pair of C (ZKC_C_ROWS, DESIGN.md "Constant folding")?  Voters whose leaves sit d levels
down both trees, for several d, proved 256 at a time (four passes of 64) through the census key: proofs/s and G1 additions per proof.  Run as fresh processes with
ZKC_C_ROWS=2 (every legal pass takes the path) and ZKC_C_ROWS=0 (none) alternating on ONE box and compare; a pass of depths (d, d) lists k = 6 283 + 238 x 2 d C rows at
nLevels = 160 (DESIGN.md "buildABC over the voter rows").  With the switch unset the rule decides, and a run from another checkout (--root) measures that checkout's library.
    python tools/c_rows_threshold.py [depths=14,18,24,28,32,36,44,160] [--root DIR]   -> one JSON line"""
import ctypes, json, os, sys, time
args = [a for a in sys.argv[1:]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--root' in args:
    i = args.index('--root'); ROOT = os.path.abspath(args[i + 1]); del args[i:i + 2]
sys.path.insert(0, ROOT)
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import census, setup, groth16

depths = [int(x) for x in (args[0] if args else '14,18,24,28,32,36,44,160').split(',')]
nl, B, REPS = 160, 256, 4
_, zp, vp = setup.ensure_test_artifacts(nl)
zk = open(zp, 'rb').read(); vk = json.load(open(vp))
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
nW = ctx.n_wires(nl); lib = ctx._lib
import random
rng = random.Random(5)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
rs = b''.join(rng.randrange(R).to_bytes(32, 'little') for _ in range(2 * B))
out = {'ZKC_C_ROWS': os.environ.get('ZKC_C_ROWS'), 'root': os.path.basename(ROOT), 'voters_per_call': B, 'calls_timed': REPS, 'rows': []}
for d in depths:
    voters = census.deep_voters(ctx, B, nl, depth=d)
    flat = b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in voters)
    d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    d_w = torch.empty(B * nW * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(B, dtype=torch.int32, device='cuda')
    for _ in range(2):                                   # the first call makes the key's tables and lists, the second seeds nothing any more
        pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_st.data_ptr(), rs)
    assert int(d_st.abs().sum().item()) == 0
    lib.zkc_profile_enable(ctx._h, 0x10); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(REPS):
        p, u = pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_st.data_ptr(), rs)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    ms, n, by = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.zkc_profile_read(ctx._h, 7, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by)); lib.zkc_profile_enable(ctx._h, 0)
    row = {'depth': d, 'c_rows_listed': 6283 + 238 * 2 * d, 'proofs_per_s': round(REPS * B / dt, 1), 'g1_additions_per_proof': round(n.value / (REPS * B)),
           'all_valid': bool(groth16.verify_batch(ctx, vk, u, p))}
    if hasattr(lib, 'zkc_debug_c_rows'):
        info = ctypes.create_string_buffer(32); lib.zkc_debug_c_rows(pk._h, 2, 0, 0, info)
        row['passes_without_c_pair_so_far'] = int.from_bytes(info.raw[8:16], 'little')
    out['rows'].append(row)
print(json.dumps(out))
pk.close(); ctx.close()
