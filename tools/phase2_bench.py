"""Where a phase-2 contribution and its verification spend their time (zkc_zkey_contribute / zkc_zkey_verify_contributions, include/zkcensus_phase2.h), and how far the
scale kernel is from two yardsticks measured in the same run.

    python tools/phase2_bench.py --nlevels 160 [--out profiles/phase2_nl160.json]      the census circuit's test key
    python tools/phase2_bench.py --logn 20     [--out profiles/phase2_2p20.json]       a circuit-shaped random instance of that domain size (tests/big_circuit.py)

The key comes from the test-only device generator.  One warm-up contribution (module load, first launches), then --reps measured ones, each with a fresh random secret on
top of the previous key; per contribution the split of zkc_phase2_stats: parse and host points, upload, scale kernel, to affine, download, hashes and output image.  Then
one verification of the whole chain against the initial key, split into table loads (upload, conversion, window tables), the four MSMs and the pairings.  Every run's
figures are reported, not a mean: their spread is the run-to-run spread.  Beside the scale kernel's time:
  (a) the same products -- the first measured contribution's points and scalar -- on --threads host threads with the variable-base multiplication of csrc/zkc_curve.h
      (zkc_debug_phase2_host_scale; one inversion per point included), its output compared byte for byte with the GPU's;
  (b) the field products of the kernel's addition chain (9 per doubling, 10 per mixed addition, counted from the recoded scalar of that run) times the number of points,
      divided by the field-product rate of the G1 bucket accumulation kernel (zkc_msm_accumulate29, 10 products per mixed addition): that rate is measured here, in a
      second verification under the library's event brackets (zkc_profile_enable), from the mixed additions the four MSMs really made and the kernel's summed time.
      It is a rate of the whole chip, quoted per CU as well; the quotient is the time the chain would take at the accumulation kernel's pace.
Prints one JSON line and writes it to --out."""
import argparse, ctypes, json, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DBL_PRODUCTS, MADD_PRODUCTS = 9, 10          # f29_acc_dbl and f29_madd (csrc/zkc_f29_g1.h): squarings counted as products, a two-term sum with one reduction as two


def naf_chain(k):
    """the addition chain zkc_p2_scale_g1 walks for the scalar k (G1Ops::dbl and add_point, csrc/zkc_point_ops.h): doublings (the index of the leading digit) and mixed additions (non-zero digits below it)"""
    top, nz, j = -1, 0, 0
    while k:
        if k & 1:
            k -= 2 - (k & 3); nz += 1; top = j
        k >>= 1; j += 1
    return {'doublings': top, 'additions': nz - 1, 'field_products_per_point': DBL_PRODUCTS * top + MADD_PRODUCTS * (nz - 1)}


def sections(z):
    out, p = {}, 12
    for _ in range(int.from_bytes(z[8:12], 'little')):
        i, sz = int.from_bytes(z[p:p + 4], 'little'), int.from_bytes(z[p + 4:p + 12], 'little')
        out[i] = (p + 12, sz); p += 12 + sz
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlevels', type=int, default=None)
    ap.add_argument('--logn', type=int, default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if (args.nlevels is None) == (args.logn is None):
        ap.error('give exactly one of --nlevels and --logn')
    import torch, zkcensus_amd
    from zkcensus_amd import phase2, r1cs, setup
    ctx = zkcensus_amd.Context(0)
    lib = ctx._lib
    tmp = tempfile.mkdtemp(prefix='zkc_phase2_bench_')
    r1, zp = os.path.join(tmp, 'c.r1cs'), os.path.join(tmp, 'c.zkey')
    if args.nlevels is not None:
        _, cs = r1cs.build(args.nlevels); cs.write(r1); seed, name = setup.DEFAULT_SEED, 'nLevels %d' % args.nlevels
        out = args.out or os.path.join(ROOT, 'profiles', 'phase2_nl%d.json' % args.nlevels)
    else:
        import big_circuit as bc
        n = 1 << args.logn
        bc.chain_instance(r1, n - n // 16, 64, 8, seed=args.logn); seed, name = 2024 + args.logn, 'generic 2^%d' % args.logn
        out = args.out or os.path.join(ROOT, 'profiles', 'phase2_2p%d.json' % args.logn)
    err = ctypes.create_string_buffer(512)
    rc = lib.zkc_setup_from_r1cs_dev(ctx._h, r1.encode(), seed, zp.encode(), None, err, 512)
    if rc:
        raise RuntimeError('setup failed (%d): %s' % (rc, err.value.decode()))
    init = open(zp, 'rb').read()
    si = sections(init)
    products = (si[8][1] + si[9][1]) // 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print('key %s: %d bytes, %d products per contribution' % (name, len(init), products), file=sys.stderr, flush=True)
    phase2.contribute(ctx, init, name='warm-up')
    key, runs, first = init, [], None
    for i in range(args.reps):
        delta = int.from_bytes(os.urandom(40), 'little') % (R - 1) + 1
        t0 = time.perf_counter()
        nxt, _ = phase2.contribute(ctx, key, delta, name='bench %d' % i)
        ms = (time.perf_counter() - t0) * 1e3
        st = phase2.stats()
        row = {'call_ms': round(ms, 2)}; row.update({k: round(st[k], 3) for k in ('parse', 'upload', 'scale_kernel', 'to_affine', 'download', 'hash_write')})
        row['chain'] = naf_chain(pow(delta, -1, R))
        row['products_per_s_scale_kernel'] = round(products / (st['scale_kernel'] * 1e-3))
        row['field_products_per_s_scale_kernel'] = round(products * row['chain']['field_products_per_point'] / (st['scale_kernel'] * 1e-3))
        runs.append(row)
        if first is None:
            first = (key, nxt, pow(delta, -1, R))
        key = nxt
        print('contribution %d: %s' % (i, json.dumps(row)), file=sys.stderr, flush=True)
    # (a) the first measured contribution's products on host threads
    src, dst, dinv = first
    ss, sd = sections(src), sections(dst)
    pts = src[ss[8][0]:ss[8][0] + ss[8][1]] + src[ss[9][0]:ss[9][0] + ss[9][1]]
    want = dst[sd[8][0]:sd[8][0] + sd[8][1]] + dst[sd[9][0]:sd[9][0] + sd[9][1]]
    hout, hms = ctypes.create_string_buffer(len(pts)), ctypes.c_double(0)
    rc = lib.zkc_debug_phase2_host_scale(pts, products, dinv.to_bytes(32, 'little'), args.threads, hout, ctypes.byref(hms))
    if rc:
        raise RuntimeError('zkc_debug_phase2_host_scale failed (%d)' % rc)
    host = {'threads': args.threads, 'ms': round(hms.value, 1), 'products_per_s': round(products / (hms.value * 1e-3)), 'equals_the_gpu_output': hout.raw == want,
            'what': 'xyzz_mul + xyzz_to_affine of csrc/zkc_curve.h per point; compare with scale_kernel + to_affine of contribution 0',
            'times_the_gpu': round(hms.value / (runs[0]['scale_kernel'] + runs[0]['to_affine']), 1)}
    assert host['equals_the_gpu_output'], 'the host products differ from the GPU\'s'
    print('host: %s' % json.dumps(host), file=sys.stderr, flush=True)
    # the verification, timed
    t0 = time.perf_counter()
    ok, n_new, why = phase2.verify(ctx, init, key)
    vms = (time.perf_counter() - t0) * 1e3
    st = phase2.stats()
    assert ok and n_new == args.reps, why
    verify = {'call_ms': round(vms, 2), 'contributions': n_new, 'table_load_ms': round(st['verify_table_load'], 2), 'four_msm_ms': round(st['verify_msm'], 2),
              'pairings_ms': round(st['verify_pairings'], 2)}
    # (b) the same verification under the event brackets: the G1 accumulation kernel's field-product rate
    lib.zkc_profile_enable(ctx._h, 0x10)
    ok, _, why = phase2.verify(ctx, init, key)
    assert ok, why
    ams, an, by, madds = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.zkc_profile_read(ctx._h, 4, ctypes.byref(ams), ctypes.byref(an), ctypes.byref(by))
    lib.zkc_profile_read(ctx._h, 7, None, ctypes.byref(madds), None)
    lib.zkc_profile_enable(ctx._h, 0)
    rate = madds.value * MADD_PRODUCTS / (ams.value * 1e-3)
    acc = {'kernel': 'zkc_msm_accumulate29', 'launches': an.value, 'ms': round(ams.value, 3), 'mixed_additions': madds.value, 'field_products_per_s': round(rate),
           'compute_units': cus, 'field_products_per_s_per_cu': round(rate / cus)}
    for row in runs:
        bound = products * row['chain']['field_products_per_point'] / rate * 1e3
        row['ms_at_accumulation_rate'] = round(bound, 3); row['scale_kernel_over_that'] = round(row['scale_kernel'] / bound, 3)
    line = json.dumps({'tool': 'tools/phase2_bench.py', 'device': torch.cuda.get_device_name(0), 'key': name, 'zkey_bytes': len(init), 'products_per_contribution': products,
                       'contribute': runs, 'host_threads': host, 'accumulation_rate': acc, 'verify': verify})
    ctx.close()
    print(line)
    with open(out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
