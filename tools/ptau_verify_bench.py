"""Where the check that a powers-of-tau file holds the powers of one tau spends its time (zkc_ptau_verify, include/zkcensus_ptau_verify.h), on the device and on the host
threads of the same entry point, and how the kernel's shape -- one doubling chain shared by a segment of points -- compares with a doubling chain per point.

    python tools/ptau_verify_bench.py --power 17,20 [--host-up-to 17] [--variants seg16=/path/libzkcensus_seg16.so,..]      writes profiles/ptau_verify_2p<power>.json per power

The file is made for the run, on the GPU, from known waste (tests/ptau_prep_lib.monomial_image: the fixed-base engines; nothing is fetched).  One warm-up call on the device
at the first power (module load, first launches), then --reps measured ones with the split of zkc_ptau_verify_stats, every run reported; then the same entry point with
ctx = None -- the sums on 16 host threads of the same box -- once, with the same seed, its verdict compared with the device's.  The host run takes about 2^(power - 15)
seconds: above --host-up-to it is not made and the record gives the count of products it would take.  A weighted point is one weight x point product: a section of n
points has n - 1 terms and each term enters two sums, so the file has 8 (N - 1) of them in G1 and 2 (N - 1) in G2.
The engine on its own: zkc_g1_wsum_pair_dev / zkc_g2_wsum_pair_dev over the points of sections 2 and 3 resident on the device, host clock around the call (it ends in a
synchronise), one warm-up and --reps runs.  The yardstick of the kernel's shape, in the same run: zkc_g1_scale_dev over the same points with ONE 128-bit scalar -- all
its lanes walk one chain in lockstep, the best a double-and-add per point can do; its call includes the conversion of every product to affine, which the sums do not
need, so the kernel-only rate of profiles/phase2_2p20.json is given beside it.
--variants: other builds of the library (say, with another segment length), each run in a process of its own with ZKCENSUS_LIB pointing at it, engine part only; --note: a
line kept in the record that says what they are."""
import argparse, json, os, random, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
SEED = bytes(range(32))


def timed(fn, reps):
    fn()                                                        # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(round((time.perf_counter() - t0) * 1e3, 2))
    return out


def engine_part(ctx, img, power, reps):
    """the two engines and the yardstick over the file's own sections 2 and 3, resident on the device"""
    import numpy as np, torch
    from zkcensus_amd import engines
    import ptau_prep_lib as pp
    _, body = pp.parse(img)
    N = 1 << power; rng = random.Random(power)
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    d_t, d_u = dev(body[2]), dev(body[3])
    d_w = dev(b''.join(rng.getrandbits(128).to_bytes(16, 'little') for _ in range(2 * N - 2)))
    d_o = torch.zeros(64 * (2 * N - 1), dtype=torch.uint8, device='cuda')
    k = rng.getrandbits(128) | (1 << 127)
    g1 = timed(lambda: engines.g1_wsum_pair(ctx, d_t.data_ptr(), 2 * N - 1, d_w.data_ptr(), mont=True), reps)
    g2 = timed(lambda: engines.g2_wsum_pair(ctx, d_u.data_ptr(), N, d_w.data_ptr(), mont=True), reps)
    sc = timed(lambda: engines.g1_scale(ctx, d_t.data_ptr(), 2 * N - 1, k, d_o.data_ptr(), mont=True), reps)
    return {'g1_wsum_pair_ms': g1, 'g1_weighted_points': 2 * (2 * N - 2), 'g1_weighted_points_per_s': round(2 * (2 * N - 2) / (min(g1) / 1e3)),
            'g2_wsum_pair_ms': g2, 'g2_weighted_points': 2 * (N - 1), 'g2_weighted_points_per_s': round(2 * (N - 1) / (min(g2) / 1e3)),
            'g1_scale_128bit_ms': sc, 'g1_scale_points': 2 * N - 1, 'g1_scale_products_per_s': round((2 * N - 1) / (min(sc) / 1e3)),
            'what': 'host clock around each call, point check included (and for g1_scale the conversion of every product to affine); best of the runs for the rates'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--power', default='17,20')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-up-to', type=int, default=17)
    ap.add_argument('--variants', default='')
    ap.add_argument('--note', default='', help='kept in the record: what the variants are and which was chosen')
    ap.add_argument('--engine-only', default=None, help='(used by --variants) the file to run the engine part over; prints one JSON line')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    import torch, zkcensus_amd
    from zkcensus_amd import setup
    import ptau_prep_lib as pp
    ctx = zkcensus_amd.Context(0)
    if args.engine_only:
        print(json.dumps(engine_part(ctx, open(args.engine_only, 'rb').read(), int(args.power), args.reps)), flush=True)
        ctx.close()
        return
    tmp = tempfile.mkdtemp(prefix='zkc_verify_bench_')
    ref = json.load(open(os.path.join(ROOT, 'profiles', 'phase2_2p20.json'))) if os.path.exists(os.path.join(ROOT, 'profiles', 'phase2_2p20.json')) else None
    warm = False
    for power in [int(x) for x in args.power.split(',')]:
        N = 1 << power; g1, g2 = 8 * (N - 1), 2 * (N - 1)
        src = os.path.join(tmp, 'u%d.ptau' % power)
        t0 = time.perf_counter()
        img = pp.monomial_image(power, pp.PLAIN, ctx)
        open(src, 'wb').write(img)
        t_make = time.perf_counter() - t0
        print('2^%d: %d bytes (%.1f s), %d G1 and %d G2 weighted points' % (power, len(img), t_make, g1, g2), file=sys.stderr, flush=True)
        if not warm:
            setup.verify_ptau(src, ctx=ctx, seed=SEED); warm = True
        runs = []
        for i in range(args.reps):
            t0 = time.perf_counter()
            verdict = setup.verify_ptau(src, ctx=ctx, seed=SEED)
            row = {'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'valid': verdict[0]}; row.update({k: round(v, 2) for k, v in setup.ptau_verify_stats().items()})
            row['g1_weighted_points_per_s'] = round(g1 / (row['sums_g1'] / 1e3)); row['g2_weighted_points_per_s'] = round(g2 / (row['sums_g2'] / 1e3))
            assert verdict[0], verdict
            runs.append(row)
            print('device %d: %s' % (i, json.dumps(row)), file=sys.stderr, flush=True)
        hrow = None
        if power <= args.host_up_to:
            t0 = time.perf_counter()
            hv = setup.verify_ptau(src, seed=SEED)
            hrow = {'threads': 16, 'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'valid': hv[0], 'same_verdict_as_the_device': hv == verdict}
            hrow.update({k: round(v, 2) for k, v in setup.ptau_verify_stats().items()})
            hrow['call_times_the_device'] = round(hrow['call_ms'] / min(r['call_ms'] for r in runs), 1)
            assert hv == verdict, (hv, verdict)
            print('host: %s' % json.dumps(hrow), file=sys.stderr, flush=True)
        eng = engine_part(ctx, img, power, args.reps)
        print('engines: %s' % json.dumps(eng), file=sys.stderr, flush=True)
        variants = {}
        for item in [v for v in args.variants.split(',') if v]:
            label, lib = item.split('=', 1)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--power', str(power), '--reps', str(args.reps), '--engine-only', src], capture_output=True, text=True,
                               env=dict(os.environ, ZKCENSUS_LIB=os.path.abspath(lib)))
            variants[label] = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 and p.stdout.strip() else {'failed': p.returncode, 'stderr': p.stderr[-300:]}
            print('variant %s: %s' % (label, json.dumps(variants[label])), file=sys.stderr, flush=True)
        line = json.dumps({'tool': 'tools/ptau_verify_bench.py', 'device': torch.cuda.get_device_name(0), 'power': power, 'file_bytes': len(img),
                           'g1_weighted_points': g1, 'g2_weighted_points': g2,
                           'what': 'stage ms of zkc_ptau_verify_stats: read, upload_check, g2_membership, sums_g1, sums_g2, pairings; weighted points per second = the weight x '
                                   'point products of a group (two per term) over the sums stage of that group, upload of the weights and reduction included',
                           'device_runs': runs,
                           'host_threads': hrow if hrow is not None else 'not run at this power (--host-up-to %d): %d G1 and %d G2 weighted points on 16 threads' % (args.host_up_to, g1, g2),
                           'engines_on_resident_points': eng,
                           'shared_doubling_over_per_point_chain': round(eng['g1_weighted_points_per_s'] / eng['g1_scale_products_per_s'], 2),
                           'zkc_g1_scale_dev_kernel_only_products_per_s_phase2_2p20_full_scalar': None if ref is None else max(r['products_per_s_scale_kernel'] for r in ref['contribute']),
                           'variants': variants, 'note': args.note, 'make_file_s': round(t_make, 1)})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, 'ptau_verify_2p%d.json' % power), 'w') as fh:
            fh.write(line + '\n')
        os.remove(src)
    ctx.close()


if __name__ == '__main__':
    main()
