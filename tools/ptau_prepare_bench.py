"""Where `powersoftau prepare phase2` spends its time (zkc_ptau_prepare, include/zkcensus_ptau_prepare.h), on the device and on the host threads of the same entry point.

    python tools/ptau_prepare_bench.py --power 14,17,20 [--host-up-to 17] [--setup]      writes profiles/ptau_prepare_2p<power>.json per power

The unprepared file is made for the run, on the GPU, from known waste (tests/ptau_prep_lib.py: the fixed-base engines; nothing is fetched).  One warm-up call on the device at
the first power (module load, first launches), then --reps measured ones with the split of zkc_ptau_prepare_stats, every run reported; check_prepared on the file just
written, next to it; then the same entry point with ctx = None -- the transforms on 16 host threads of the same box -- once, its output compared byte for byte with the
device's.  The host run takes about 2^(power - 10) seconds: above --host-up-to it is not made, and the record says so instead of giving a ratio.  The scalar products are
counted here from the sizes: a block of n = 2^p points takes n at the input (the 1/n factor) and n/2 - 2^(p-1-s) per stage s (the butterflies whose twiddle is not 1).
--setup: tools/ptau_setup.py's call on the prepared file at the file's own power (a circuit-shaped instance of that domain), to show that it is accepted."""
import argparse, json, os, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))


def products(power):
    """(G1, G2) scalar products of one preparation"""
    block = lambda p: (1 << p) + sum((1 << (p - 1)) - (1 << (p - 1 - s)) for s in range(p))
    upto = lambda last: sum(block(p) for p in range(last + 1))
    return upto(power + 1) + 2 * upto(power), upto(power)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--power', default='14,17,20')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--host-up-to', type=int, default=17)
    ap.add_argument('--setup', action='store_true')
    ap.add_argument('--out-dir', default=os.path.join(ROOT, 'profiles'))
    args = ap.parse_args()
    import torch, zkcensus_amd
    from zkcensus_amd import setup
    import ptau_prep_lib as pp
    ctx = zkcensus_amd.Context(0)
    tmp = tempfile.mkdtemp(prefix='zkc_prep_bench_')
    ref = json.load(open(os.path.join(ROOT, 'profiles', 'phase2_2p20.json'))) if os.path.exists(os.path.join(ROOT, 'profiles', 'phase2_2p20.json')) else None
    warm = False
    for power in [int(x) for x in args.power.split(',')]:
        src, dst, host = [os.path.join(tmp, '%s%d.ptau' % (x, power)) for x in 'udh']
        t0 = time.perf_counter()
        open(src, 'wb').write(pp.monomial_image(power, pp.PLAIN, ctx))
        t_make = time.perf_counter() - t0
        g1, g2 = products(power)
        print('2^%d: %d bytes unprepared (%.1f s), %d G1 and %d G2 scalar products' % (power, os.path.getsize(src), t_make, g1, g2), file=sys.stderr, flush=True)
        if not warm:
            setup.prepare_ptau(src, dst, ctx=ctx); warm = True
        runs = []
        for i in range(args.reps):
            t0 = time.perf_counter()
            setup.prepare_ptau(src, dst, ctx=ctx)
            row = {'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}; row.update({k: round(v, 2) for k, v in setup.ptau_prepare_stats().items()})
            row['g1_products_per_s'] = round(g1 / (row['transforms_g1'] / 1e3)); row['g2_products_per_s'] = round(g2 / (row['transforms_g2'] / 1e3))
            runs.append(row)
            print('device %d: %s' % (i, json.dumps(row)), file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        verdict = setup.check_prepared(dst, ctx=ctx)
        check = {'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'valid': verdict[0]}; check.update({k: round(v, 2) for k, v in setup.ptau_prepare_stats().items()})
        assert verdict[0], verdict
        print('check_prepared: %s' % json.dumps(check), file=sys.stderr, flush=True)
        hrow = None
        if power <= args.host_up_to:
            t0 = time.perf_counter()
            setup.prepare_ptau(src, host)
            hrow = {'threads': 16, 'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}; hrow.update({k: round(v, 2) for k, v in setup.ptau_prepare_stats().items()})
            hrow['equals_the_device_output'] = open(host, 'rb').read() == open(dst, 'rb').read()
            hrow['call_times_the_device'] = round(hrow['call_ms'] / min(r['call_ms'] for r in runs), 1)
            assert hrow['equals_the_device_output'], 'the host file differs from the device file'
            os.remove(host)
            print('host: %s' % json.dumps(hrow), file=sys.stderr, flush=True)
        accepted = None
        if args.setup:
            import big_circuit as bc
            n = 1 << power; r1 = os.path.join(tmp, 'c%d.r1cs' % power)
            bc.chain_instance(r1, n - n // 16, 64, 8, seed=power)
            p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'ptau_setup.py'), r1, dst, os.path.join(tmp, 'k%d.zkey' % power)], capture_output=True, text=True)
            accepted = {'exit_status': p.returncode, 'line': (p.stdout.strip().splitlines() or [p.stderr.strip()[-300:]])[-1]}
            print('tools/ptau_setup.py: %s' % json.dumps(accepted), file=sys.stderr, flush=True)
        line = json.dumps({'tool': 'tools/ptau_prepare_bench.py', 'device': torch.cuda.get_device_name(0), 'power': power, 'unprepared_bytes': os.path.getsize(src),
                           'prepared_bytes': os.path.getsize(dst), 'g1_scalar_products': g1, 'g2_scalar_products': g2,
                           'what': 'stage ms of zkc_ptau_prepare_stats: read, upload_check, transforms_g1, transforms_g2, affine_download, write_or_compare; products per '
                                   'second = the scalar products counted from the block sizes over the transform stage of their group',
                           'device_runs': runs, 'check_prepared': check, 'host_threads': hrow if hrow is not None else 'not run at this power (--host-up-to %d)' % args.host_up_to,
                           'zkc_g1_scale_dev_products_per_s_phase2_2p20': None if ref is None else max(r['products_per_s_scale_kernel'] for r in ref['contribute']),
                           'ptau_setup_on_the_prepared_file': accepted, 'make_unprepared_s': round(t_make, 1)})
        print(line, flush=True)
        with open(os.path.join(args.out_dir, 'ptau_prepare_2p%d.json' % power), 'w') as fh:
            fh.write(line + '\n')
        for f in (src, dst):
            os.remove(f)
    ctx.close()


if __name__ == '__main__':
    main()
