#!/usr/bin/env python
"""snarkjs `wtns check` on the GPU (include/zkcensus_r1cs.h).

    tools/wtns_check.py <circuit.r1cs> <witness.wtns>            prints the verdict; exit status 0 = every constraint holds, 1 = not
    tools/wtns_check.py --bench --nlevels 160 --batch 1024        builds the census .r1cs (r1cs.build), makes the witnesses on the device (zkc_witness_dev), checks them in
                                                                  place (zkc_r1cs_check_dev) and prints one JSON line: witnesses/s and the zkc_r1cs_check_stats split
"""
import argparse, json, os, random, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))


def check_files(r1cs_path, wtns_path, device):
    import zkcensus_amd
    from zkcensus_amd import groth16, r1cs
    ctx = zkcensus_amd.Context(device)
    payload = groth16._wtns_payload(wtns_path)
    with r1cs.Device(ctx, r1cs_path) as dev:
        if len(payload) != 32 * dev.info[0]:
            print('Invalid witness length. Circuit: %d, witness: %d' % (dev.info[0], len(payload) // 32)); return 1
        first, count = dev.check(payload, 1)
    ctx.close()
    if first[0] == r1cs.SATISFIED:
        print('WITNESS IS CORRECT'); return 0
    print('WITNESS CHECKING FAILED: ' + ('wire 0 is not 1' if first[0] == r1cs.NOT_ONE else "a wire is not below the field's prime" if first[0] == r1cs.WIRE_RANGE
                                         else 'constraint %d is not satisfied (%d violated in all)' % (first[0], count[0])))
    return 1


def bench(nlevels, batch, reps, device):
    import numpy as np, torch
    import zkcensus_amd
    import oracle_lib as ol
    from zkcensus_amd import r1cs, flatten_inputs
    from census_gen import random_voter
    L, cs = r1cs.build(nlevels)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, 'census.r1cs'); cs.write(p); img = open(p, 'rb').read()
    ctx = zkcensus_amd.Context(device)
    rng = random.Random(nlevels)
    distinct = [flatten_inputs(random_voter(rng, ol.poseidon, nLevels=nlevels, depth_c=rng.randrange(1, min(nlevels, 24)), depth_s=rng.randrange(1, min(nlevels, 24))), nlevels)
                for _ in range(min(batch, 32))]
    flat = b''.join(distinct[i % len(distinct)] for i in range(batch))
    torch.cuda.set_device(device)
    d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    d_w = torch.empty(batch * L.nWires * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(batch, dtype=torch.int32, device='cuda')
    ctx.witness_dev(d_in.data_ptr(), batch, d_w.data_ptr(), d_st.data_ptr(), nlevels)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    t0 = time.perf_counter(); dev = r1cs.Device(ctx, img); load_ms = (time.perf_counter() - t0) * 1e3; load_split = dev.stats()
    first, count = dev.check_dev(d_w, batch)                        # warm-up: work space, first launches
    assert first == [-1] * batch and count == [0] * batch, 'a generated witness violates the constraint system'
    best, split = None, None
    for _ in range(reps):
        t0 = time.perf_counter(); dev.check_dev(d_w, batch); ms = (time.perf_counter() - t0) * 1e3
        if best is None or ms < best:
            best, split = ms, dev.stats()
    # one witness with a broken wire among the good ones: the verdict names the row, the others stay satisfied
    k = L.off_nullifier + 7
    d_w[32 * L.nWires * (batch // 2) + 32 * k] ^= 1
    f2, c2 = dev.check_dev(d_w, batch)
    assert f2[batch // 2] >= 0 and c2[batch // 2] >= 1 and sum(1 for x in f2 if x != -1) == 1
    out = {'tool': 'wtns_check', 'nLevels': nlevels, 'batch': batch, 'nWires': dev.info[0], 'nConstraints': dev.info[2], 'check_ms': round(best, 3),
           'witnesses_per_s': round(batch / best * 1e3, 1), 'stats_ms': {'host': round(split[0], 3), 'copies': round(split[1], 3), 'kernels': round(split[2], 3)},
           'load_ms': round(load_ms, 1), 'load_stats_ms': {'host_layout': round(load_split[0], 1), 'copies': round(load_split[1], 1)}, 'reps': reps}
    dev.close(); ctx.close()
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('r1cs', nargs='?'); ap.add_argument('wtns', nargs='?')
    ap.add_argument('--bench', action='store_true'); ap.add_argument('--nlevels', type=int, default=160); ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5); ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args()
    if a.bench:
        return bench(a.nlevels, a.batch, a.reps, a.device)
    if not a.r1cs or not a.wtns:
        ap.error('give <circuit.r1cs> <witness.wtns>, or --bench')
    return check_files(a.r1cs, a.wtns, a.device)


if __name__ == '__main__':
    sys.exit(main())
