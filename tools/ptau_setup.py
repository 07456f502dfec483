"""`snarkjs groth16 setup circuit.r1cs pot_final.ptau circuit_0000.zkey` on the GPU (include/zkcensus_ptau.h):

    python tools/ptau_setup.py circuit.r1cs pot.ptau out.zkey [vkey.json] [--host] [--device N]

The .ptau must be prepared (`powersoftau prepare phase2`; public files are).  Writes the initial key (gamma = delta = 1, no contributions; follow with phase2.contribute)
and, when named, its verification_key.json; prints where the time went.  --host: the sums run on host threads and no GPU is touched; the bytes are the same."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('r1cs'); ap.add_argument('ptau'); ap.add_argument('zkey'); ap.add_argument('vkey', nargs='?', default=None)
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--device', type=int, default=0)
    args = ap.parse_args()
    from zkcensus_amd import setup, _native
    ctx = None
    if not args.host:
        import zkcensus_amd
        ctx = zkcensus_amd.Context(args.device)
    t0 = time.perf_counter()
    try:
        setup.from_ptau(args.r1cs, args.ptau, args.zkey, args.vkey, ctx=ctx)
    except _native.ZkcError as e:
        print('refused: %s' % e, file=sys.stderr)
        return 1
    finally:
        if ctx is not None:
            ctx.close()
    print(json.dumps({'zkey': args.zkey, 'vkey': args.vkey, 'bytes': os.path.getsize(args.zkey), 'path': 'host threads' if args.host else 'device',
                      'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'stages_ms': {k: round(v, 2) for k, v in setup.ptau_stats().items()}}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
