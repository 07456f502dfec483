#!/usr/bin/env python3
"""A fixed workload for comparing the prover's kernel launches between two trees (profiles/pass_plan_kernel_calls.json): the first 1, 2, 3, 65 and 130 of 130 seeded
voters at nLevels = 10 (tools/synth_voter.py, leaves 1 .. 9 levels down either tree), each size as one fullProve call on a fresh key.  Run it under `rocprofv3 --kernel-trace --stats` with ZKC_TOP_FOLD=0: with the
top-of-tree table off nothing the prover launches depends on host timing, so the table of kernel name -> calls of a refactor equals its parent's.
The sizes take the small-pass (tree) form, the lane-per-product blinding below and above four proofs, and calls of two and three passes over the key's lanes."""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, numpy as np
import zkcensus_amd
from zkcensus_amd import setup
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from synth_voter import make_voter

NL, SIZES = 10, (1, 2, 3, 65, 130)


def main():
    _, zp, _ = setup.ensure_test_artifacts(NL)
    ctx = zkcensus_amd.Context(0)
    rng = random.Random(10)
    flat = b''.join(zkcensus_amd.flatten_inputs(make_voter(rng, nLevels=NL, depth_c=1 + i % 9, depth_s=1 + (3 * i) % 9), NL) for i in range(max(SIZES)))
    nIn, nW = ctx.n_inputs(NL), ctx.n_wires(NL)
    d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    d_w = torch.empty(max(SIZES) * nW * 32, dtype=torch.uint8, device='cuda'); d_s = torch.zeros(max(SIZES), dtype=torch.int32, device='cuda')
    assert d_in.numel() == max(SIZES) * nIn * 32
    for B in SIZES:
        pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read())
        rs = b''.join((11 + i).to_bytes(32, 'little') + (17 + i).to_bytes(32, 'little') for i in range(B))
        proofs, _ = pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_s.data_ptr(), rs)
        torch.cuda.synchronize()
        assert d_s[:B].cpu().tolist() == [0] * B and len(proofs) == 256 * B
        pk.close()
    ctx.close()
    print('proved', SIZES, 'voters at nLevels', NL)


if __name__ == '__main__':
    main()
