"""Where key generation spends its time, on the host and on the GPU (zkc_setup_from_r1cs against zkc_setup_from_r1cs_dev, include/zkcensus_setup.h).

Per key -- the census circuit at the given nLevels, and circuit-shaped random instances (tests/big_circuit.py chain_instance, the circuits of tools/generic_bench.py) at
the given domain sizes -- the same .r1cs and seed go through both generators.  Reported per generator: the whole call and its split (zkc_setup_stats): stage 1 read the
.r1cs and compute the scalars, the two window tables, stage 2 scalars -> points without the tables, stage 3 write the .zkey and the JSON; beside them the time Python needs
to state the circuit (r1cs.build + write, or chain_instance), which every caller of setup.ensure_test_artifacts pays as well; whether the two keys' SHA-256 agree; and
whole_call_ratio = host call / device call.  The device generator runs twice: `device_first` includes what a process pays once (module load, first launches).

    python tools/setup_bench.py [--nlevels 10,160] [--logn 14,16] [--out profiles/setup_device.json]

Prints one JSON line and writes it to --out.  The host generator uses the host's threads (zkc_fixedbase.h parallel_for: at most 32)."""
import argparse, ctypes, hashlib, json, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
STAGES = ('stage1_scalars_ms', 'tables_ms', 'stage2_points_ms', 'stage3_write_ms')


def sha(path):
    with open(path, 'rb') as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def run(lib, ctx, r1, seed, out_stem):
    """one call of either generator -> (call ms, split, zkey sha, vkey sha)"""
    err = ctypes.create_string_buffer(512); z, v = out_stem + '.zkey', out_stem + '_vkey.json'
    t0 = time.perf_counter()
    if ctx is None:
        rc = lib.zkc_setup_from_r1cs(r1.encode(), seed, z.encode(), v.encode(), err, 512)
    else:
        rc = lib.zkc_setup_from_r1cs_dev(ctx._h, r1.encode(), seed, z.encode(), v.encode(), err, 512)
    ms = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise RuntimeError('setup failed (%d): %s' % (rc, err.value.decode()))
    st = (ctypes.c_double * 4)(); lib.zkc_setup_stats(st)
    row = {'call_ms': round(ms, 1)}; row.update({k: round(x, 1) for k, x in zip(STAGES, st)})
    return row, sha(z), sha(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlevels', default='10,160')
    ap.add_argument('--logn', default='14,16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'setup_device.json'))
    args = ap.parse_args()
    import zkcensus_amd
    from zkcensus_amd import r1cs, setup
    import big_circuit as bc
    ctx = zkcensus_amd.Context(0); lib = ctx._lib
    tmp = tempfile.mkdtemp(prefix='zkc_setup_bench_')
    jobs = [('nLevels %d' % nl, 'census', nl) for nl in [int(x) for x in args.nlevels.split(',') if x]]
    jobs += [('generic 2^%d' % ln, 'generic', ln) for ln in [int(x) for x in args.logn.split(',') if x]]
    rows = []
    for name, kind, size in jobs:
        r1 = os.path.join(tmp, '%s_%d.r1cs' % (kind, size))
        t0 = time.perf_counter()
        if kind == 'census':
            _, cs = r1cs.build(size); cs.write(r1); seed = setup.DEFAULT_SEED
        else:
            n = 1 << size; n_cons = n - n // 16
            bc.chain_instance(r1, n_cons, 64, 8, seed=size); seed = 2024 + size
        t_build = (time.perf_counter() - t0) * 1e3
        host, hz, hv = run(lib, None, r1, seed, os.path.join(tmp, 'host'))
        dev1, dz, dv = run(lib, ctx, r1, seed, os.path.join(tmp, 'dev'))
        dev, dz2, dv2 = run(lib, ctx, r1, seed, os.path.join(tmp, 'dev'))
        rows.append({'key': name, 'python_r1cs_build_ms': round(t_build, 1), 'host': host, 'device_first': dev1, 'device': dev,
                     'sha256_equal': hz == dz == dz2 and hv == dv == dv2, 'zkey_sha256': hz,
                     'stage2_ratio_with_tables': round((host['tables_ms'] + host['stage2_points_ms']) / (dev['tables_ms'] + dev['stage2_points_ms']), 2),
                     'stage2_ratio_without_tables': round(host['stage2_points_ms'] / dev['stage2_points_ms'], 2),
                     'whole_call_ratio': round(host['call_ms'] / dev['call_ms'], 2)})
    ctx.close()
    import torch
    line = json.dumps({'tool': 'tools/setup_bench.py', 'device': torch.cuda.get_device_name(0), 'host_threads': min(32, os.cpu_count() or 4),
                       'cpus_allowed': len(os.sched_getaffinity(0)), 'keys': rows})
    print(line)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
