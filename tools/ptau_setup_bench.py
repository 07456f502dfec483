"""Where a key from a powers-of-tau file spends its time (zkc_setup_from_ptau, include/zkcensus_ptau.h), on the device and on the host threads of the same entry point.

    python tools/ptau_setup_bench.py --nlevels 160 [--out profiles/setup_ptau_nl160.json]      the census circuit
    python tools/ptau_setup_bench.py --logn 20     [--out profiles/setup_ptau_2p20.json]       a circuit-shaped random instance of that domain size (tests/big_circuit.py)

The .ptau is made for the run, on the GPU, from known waste (tests/ptau_lib.py: the fixed-base engines; its power is the circuit's).  One warm-up call on the device
(module load, first launches), then --reps measured ones with the split of zkc_setup_ptau_stats, every run reported; then the same call with ctx = None -- the sums on 16
host threads of the same box -- once, its output compared byte for byte with the device's.  The counts of unit (+-1) and general coefficient x point products of the
two groups are recounted here from the circuit (what the scale pass and the accumulation pass are given).  zkc_setup_from_r1cs_dev is not comparable: it multiplies one
fixed base.  Prints one JSON line and writes it to --out."""
import argparse, json, os, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU, ALPHA, BETA = 0x3c6ef372fe94f82ba54ff53a5f1d36f1510e527fade682d19b05688c2b3e6c1f % R, 0x1f83d9abfb41bd6b5be0cd19137e2179cbbb9d5dc1059ed8629a292a367cd507 % R, 0x9159015a3070dd17152fecd8f70e593967332667ffc00b318eb44a8768581511 % R


def count(sides, n_pub, n):
    """sides: an iterable of (A coefficients, B coefficients, C coefficients) per constraint -> the products of the two groups as the library classifies them"""
    unit = {'A': 0, 'B': 0, 'C': 0}; gen = {'A': 0, 'B': 0, 'C': 0}
    for abc in sides:
        for m, cs in zip('ABC', abc):
            for c in cs:
                c %= R
                if c in (1, R - 1): unit[m] += 1
                elif c: gen[m] += 1
    # G1: A and B terms feed two rows each (A | K, B1 | K), C terms one; the extra rows 2 (nPub + 1) unit terms; the three partition-of-unity sums 3 n.  G2: B terms, and one sum
    return {'g1_unit': 2 * unit['A'] + 2 * unit['B'] + unit['C'] + 2 * (n_pub + 1) + 3 * n, 'g1_general': 2 * gen['A'] + 2 * gen['B'] + gen['C'],
            'g2_unit': unit['B'] + n, 'g2_general': gen['B'], 'matrix_unit': unit, 'matrix_general': gen}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nlevels', type=int, default=None)
    ap.add_argument('--logn', type=int, default=None)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--no-host', action='store_true', help='skip the host-thread run')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if (args.nlevels is None) == (args.logn is None):
        ap.error('give exactly one of --nlevels and --logn')
    import torch, zkcensus_amd
    from zkcensus_amd import r1cs, setup
    import ptau_lib as pl
    ctx = zkcensus_amd.Context(0)
    tmp = tempfile.mkdtemp(prefix='zkc_ptau_bench_')
    r1 = os.path.join(tmp, 'c.r1cs')
    t0 = time.perf_counter()
    if args.nlevels is not None:
        import closed_form as cf
        _, cs = r1cs.build(args.nlevels); cs.write(r1); name = 'nLevels %d' % args.nlevels
        n_wires, n_pub, cons = cf.read_r1cs(r1)
        n_cons = len(cons); sides = ([[c for _, c in s] for s in abc] for abc in cons)
        out = args.out or os.path.join(ROOT, 'profiles', 'setup_ptau_nl%d.json' % args.nlevels)
    else:
        import big_circuit as bc
        n = 1 << args.logn; n_cons, n_in, n_pub = n - n // 16, 64, 8
        n_wires = bc.chain_instance(r1, n_cons, n_in, n_pub, seed=args.logn); name = 'generic 2^%d' % args.logn
        sides = (([c for _, c in a], [c for _, c in b], [1]) for a, b in bc._chain_rows(n_cons, n_in, args.logn))
        out = args.out or os.path.join(ROOT, 'profiles', 'setup_ptau_2p%d.json' % args.logn)
    power = (n_cons + n_pub).bit_length(); n = 1 << power
    counts = count(sides, n_pub, n)
    t_circuit = time.perf_counter() - t0
    print('%s: %d wires, %d constraints, domain 2^%d, %s (%.1f s)' % (name, n_wires, n_cons, power, json.dumps(counts), t_circuit), file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    ptau = pl.write(os.path.join(tmp, 'pot.ptau'), power, TAU, ALPHA, BETA, ctx=ctx)
    t_ptau = time.perf_counter() - t0
    print('ptau: %d bytes (%.1f s)' % (os.path.getsize(ptau), t_ptau), file=sys.stderr, flush=True)
    dz, dv, hz, hv = [os.path.join(tmp, x) for x in ('d.zkey', 'd.json', 'h.zkey', 'h.json')]
    setup.from_ptau(r1, ptau, dz, dv, ctx=ctx)                  # warm-up
    runs = []
    for i in range(args.reps):
        t0 = time.perf_counter()
        setup.from_ptau(r1, ptau, dz, dv, ctx=ctx)
        row = {'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}; row.update({k: round(v, 2) for k, v in setup.ptau_stats().items()})
        row['points_stage_ms'] = round(row['upload'] + row['scale'] + row['accumulate_reduce'], 2)
        runs.append(row)
        print('device %d: %s' % (i, json.dumps(row)), file=sys.stderr, flush=True)
    host = None
    if not args.no_host:
        t0 = time.perf_counter()
        setup.from_ptau(r1, ptau, hz, hv)
        host = {'threads': 16, 'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}; host.update({k: round(v, 2) for k, v in setup.ptau_stats().items()})
        host['points_stage_ms'] = round(host['scale'] + host['accumulate_reduce'], 2)
        host['equals_the_device_output'] = open(hz, 'rb').read() == open(dz, 'rb').read() and open(hv, 'rb').read() == open(dv, 'rb').read()
        host['points_stage_times_the_device'] = round(host['points_stage_ms'] / min(r['points_stage_ms'] for r in runs), 1)
        assert host['equals_the_device_output'], 'the host key differs from the device key'
        print('host: %s' % json.dumps(host), file=sys.stderr, flush=True)
    line = json.dumps({'tool': 'tools/ptau_setup_bench.py', 'device': torch.cuda.get_device_name(0), 'circuit': name, 'wires': n_wires, 'constraints': n_cons, 'public': n_pub,
                       'domain_log2': power, 'ptau_bytes': os.path.getsize(ptau), 'zkey_bytes': os.path.getsize(dz), 'products': counts,
                       'what': 'stage ms of zkc_setup_ptau_stats: read_parse, transpose, upload, scale (general coefficients, to affine included), accumulate_reduce (to affine and '
                               'download included), checks_write; points_stage_ms = upload + scale + accumulate_reduce (host: scale + accumulate_reduce)',
                       'device_runs': runs, 'host_threads': host, 'make_circuit_s': round(t_circuit, 1), 'make_ptau_s': round(t_ptau, 1)})
    ctx.close()
    print(line)
    with open(out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
