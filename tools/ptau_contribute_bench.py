"""Where a contribution to a powers-of-tau file spends its time (zkc_ptau_contribute, include/zkcensus_ptau_contribute.h), on the device and on the host threads of the
same entry point, and how the two forms of the kernel -- signed 4-bit windows over a per-lane table, and bit-serial double-and-add -- compare on random full-width scalars.

    python tools/ptau_contribute_bench.py --power 17,20 [--host-up-to 17] [--reps 3] [--kernel-only]      writes profiles/ptau_contribute_2p<power>.json per power

The file is made for the run, on the GPU, from known waste (tests/ptau_prep_lib.monomial_image: the fixed-base engines; nothing is fetched).  One warm-up call on the
device at the first power (module load, first launches), then --reps measured ones with the split of zkc_ptau_contribute_stats, every run reported, in both kernel forms
through the hook; then the same entry point with ctx = None -- 16 host threads of the same box -- once, with the same secrets, its bytes compared with the device's.  Above
--host-up-to the host run is not made and the record gives the count of products it would take.  A contribution at power p is 5 N - 1 products in G1 and N + 1 in G2, N = 2^p.
The kernel on its own: 2^21 random points of G1 and 2^20 of G2 (random multiples of the generators from the fixed-base engines) under random scalars below 2^253, resident
on the device; the shipped form, the bit-serial form and, for G1, zkc_g1_scale_dev on the same points under ONE full-width scalar -- a chain that pays for no per-lane
digit -- alternate in one process, one warm-up round and --reps measured ones.  The kernel's time is the library's own clock around launch and synchronise
(zkc_debug_scale_each_stats), the call's is the host clock around the call, conversion to affine included."""
import argparse, json, os, random, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
SECRETS = (0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100a1b2, 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef,
           0x2b7e151628aed2a6abf7158809cf4f3c2b7e151628aed2a6abf7158809cf4f3c)
FORMS = {0: 'windowed', 1: 'bit_serial'}


def spread(xs):
    return round((max(xs) - min(xs)) / min(xs), 4)


def kernel_part(ctx, reps, log_g1=21, log_g2=20):
    import numpy as np, torch
    from zkcensus_amd import engines
    rng = np.random.default_rng(7)

    def scalars(n):
        k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); k[:, 31] &= 0x1f            # below 2^253 < r
        return torch.from_numpy(k.reshape(-1)).cuda()
    out = {}
    for g2, logn in ((False, log_g1), (True, log_g2)):
        n, w = 1 << logn, 128 if g2 else 64
        d_pts = torch.zeros(w * n, dtype=torch.uint8, device='cuda')
        d_a = scalars(n)
        (engines.g2_fixed_mul if g2 else engines.g1_fixed_mul)(ctx, engines.G2_GENERATOR if g2 else engines.G1_GENERATOR, d_a.data_ptr(), n, d_pts.data_ptr())
        d_k = scalars(n); d_o = torch.zeros(w * n, dtype=torch.uint8, device='cuda')
        one = random.Random(3).getrandbits(253) | (1 << 252)
        rows = {name: {'kernel_ms': [], 'call_ms': []} for name in FORMS.values()}
        if not g2:
            rows['one_scalar_zkc_g1_scale_dev'] = {'call_ms': []}
        for rep in range(reps + 1):                             # round 0 is the warm-up
            for form, name in FORMS.items():
                t0 = time.perf_counter()
                engines.debug_scale_each(ctx, g2, d_pts.data_ptr(), n, d_k.data_ptr(), d_o.data_ptr(), form=form)
                call = (time.perf_counter() - t0) * 1e3
                if rep:
                    rows[name]['kernel_ms'].append(round(engines.scale_each_stats()['scale_kernel'], 2)); rows[name]['call_ms'].append(round(call, 2))
            if not g2:
                t0 = time.perf_counter()
                engines.g1_scale(ctx, d_pts.data_ptr(), n, one, d_o.data_ptr())
                if rep:
                    rows['one_scalar_zkc_g1_scale_dev']['call_ms'].append(round((time.perf_counter() - t0) * 1e3, 2))
        for name, r in rows.items():
            key = 'kernel_ms' if 'kernel_ms' in r else 'call_ms'
            r['products_per_s'] = round(n / (min(r[key]) / 1e3)); r['run_to_run_spread'] = spread(r[key]); r['rate_from'] = key
        ratio = min(rows['bit_serial']['kernel_ms']) / min(rows['windowed']['kernel_ms'])
        out['g2' if g2 else 'g1'] = {'points': n, 'forms': rows, 'windowed_over_bit_serial': round(ratio, 3),
                                     'windowed_ahead_by_more_than_the_spread': ratio - 1 > max(rows['windowed']['run_to_run_spread'], rows['bit_serial']['run_to_run_spread']),
                                     'work_space_bytes_per_point': {name: ctx._lib.zkc_debug_scale_each_work_bytes(1 if g2 else 0, n, form) // n for form, name in FORMS.items()}}
        del d_pts, d_a, d_k, d_o
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--power', default='17,20')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-up-to', type=int, default=17)
    ap.add_argument('--kernel-only', action='store_true', help='the kernel part alone: one JSON line, no profile written')
    ap.add_argument('--kernel-logs', default='21,20', help='log2 of the points of the kernel part, G1 and G2')
    ap.add_argument('--note', default='')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    import torch, zkcensus_amd
    from zkcensus_amd import setup
    import ptau_prep_lib as pp
    ctx = zkcensus_amd.Context(0)
    lg1, lg2 = (int(x) for x in args.kernel_logs.split(','))
    kern = kernel_part(ctx, args.reps, lg1, lg2)
    print('kernel: %s' % json.dumps(kern), file=sys.stderr, flush=True)
    if args.kernel_only:
        print(json.dumps(kern), flush=True)
        ctx.close()
        return
    tmp = tempfile.mkdtemp(prefix='zkc_contribute_bench_')
    warm = False
    for power in [int(x) for x in args.power.split(',')]:
        N = 1 << power; g1, g2 = 5 * N - 1, N + 1
        src, dst, hdst = (os.path.join(tmp, '%s%d.ptau' % (s, power)) for s in 'udh')
        t0 = time.perf_counter()
        img = pp.monomial_image(power, pp.PLAIN, ctx)
        open(src, 'wb').write(img)
        t_make = time.perf_counter() - t0
        print('2^%d: %d bytes (%.1f s), %d G1 and %d G2 products' % (power, len(img), t_make, g1, g2), file=sys.stderr, flush=True)
        if not warm:
            setup.contribute_ptau(src, dst, ctx=ctx, secrets=SECRETS); warm = True
        runs = {name: [] for name in FORMS.values()}
        for i in range(args.reps):
            for form, name in FORMS.items():                    # alternating
                t0 = time.perf_counter()
                h = setup.debug_contribute_ptau(src, dst, ctx=ctx, secrets=SECRETS, form=form)
                row = {'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}; row.update({k: round(v, 2) for k, v in setup.ptau_contribute_stats().items()})
                row['g1_products_per_s'] = round(g1 / (row['scale_g1'] / 1e3)); row['g2_products_per_s'] = round(g2 / (row['scale_g2'] / 1e3))
                runs[name].append(row)
                print('device %s %d: %s' % (name, i, json.dumps(row)), file=sys.stderr, flush=True)
        setup.contribute_ptau(src, dst, ctx=ctx, secrets=SECRETS)
        chunk = min(1 << 20, 2 * N - 1)
        resident = {'g1_chunk_points': chunk, 'g2_chunk_points': min(1 << 20, N),
                    'g1_bytes': chunk * (64 + 32) + ctx._lib.zkc_debug_scale_each_work_bytes(0, chunk, 0),
                    'g2_bytes': min(1 << 20, N) * 128 + chunk * 32 + ctx._lib.zkc_debug_scale_each_work_bytes(1, min(1 << 20, N), 0),
                    'what': 'points, scalars (sized once for the largest chunk of the file), sums and the windowed form\'s table, for the largest chunk of each group'}
        hrow = None
        if power <= args.host_up_to:
            t0 = time.perf_counter()
            hh = setup.contribute_ptau(src, hdst, secrets=SECRETS)
            hrow = {'threads': 16, 'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'same_bytes_as_the_device': open(hdst, 'rb').read() == open(dst, 'rb').read() and hh == h}
            hrow.update({k: round(v, 2) for k, v in setup.ptau_contribute_stats().items()})
            hrow['call_times_the_device'] = round(hrow['call_ms'] / min(r['call_ms'] for r in runs['windowed']), 1)
            assert hrow['same_bytes_as_the_device']
            os.remove(hdst)
            print('host: %s' % json.dumps(hrow), file=sys.stderr, flush=True)
        line = json.dumps({'tool': 'tools/ptau_contribute_bench.py', 'device': torch.cuda.get_device_name(0), 'power': power, 'file_bytes': len(img), 'g1_products': g1, 'g2_products': g2,
                           'what': 'stage ms of zkc_ptau_contribute_stats: read, upload_scalars_check, scale_g1, scale_g2 (the scale kernel with the point checks fused in), '
                                   'affine_download, hashes_write; products per second of a group = its products over its scale stage',
                           'device_runs': runs, 'resident_device_bytes_per_chunk': resident,
                           'host_threads': hrow if hrow is not None else 'not run at this power (--host-up-to %d): by count, %d G1 and %d G2 products of 254 doublings and about 127 '
                                                                         'additions each on 16 threads' % (args.host_up_to, g1, g2),
                           'kernel_alone_random_points_and_scalars': kern, 'window_widths_tried': [4], 'note': args.note, 'make_file_s': round(t_make, 1)})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, 'ptau_contribute_2p%d.json' % power), 'w') as fh:
            fh.write(line + '\n')
        for p in (src, dst):
            os.remove(p)
    ctx.close()


if __name__ == '__main__':
    main()
