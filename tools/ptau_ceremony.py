"""Phase 1 of the ceremony on the GPU (include/zkcensus_ptau_contribute.h): `snarkjs powersoftau new`, `contribute` and the transcript part of `verify`.

    python tools/ptau_ceremony.py new POWER out.ptau
    python tools/ptau_ceremony.py contribute in.ptau out.ptau [--name NAME] [--verify] [--host] [--device N]
    python tools/ptau_ceremony.py verify [prev.ptau] next.ptau [--host] [--device N] [--seed HEX64]

new: tau = alpha = beta = 1, every point its group's generator, no contribution.  contribute: secrets from the OS, used once and cleared; prints the contribution hash.
--verify checks the input's points first (setup.verify_ptau).  verify: is next.ptau what prev.ptau becomes under the contributions its section 7 adds -- without
prev.ptau, what a `new` file of its power becomes -- and is it the powers of one tau, alpha and beta?  --host: host threads, no GPU is touched; bytes and verdicts are the
same.  Exit status 0: done / valid; 1: not valid (the line names the failing check) or refused.  Prints one JSON line with where the time went.  The record format is
this library's own: snarkjs does not accept it, nor this tool snarkjs' (the header says exactly what is shared)."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('new'); p.add_argument('power', type=int); p.add_argument('out')
    p = sub.add_parser('contribute'); p.add_argument('src'); p.add_argument('dst'); p.add_argument('--name', default=''); p.add_argument('--verify', action='store_true')
    p.add_argument('--host', action='store_true'); p.add_argument('--device', type=int, default=0)
    p = sub.add_parser('verify'); p.add_argument('files', nargs='+'); p.add_argument('--host', action='store_true'); p.add_argument('--device', type=int, default=0)
    p.add_argument('--seed', default=None)
    args = ap.parse_args()
    from zkcensus_amd import setup, _native
    ctx = None
    try:
        t0 = time.perf_counter()
        if args.cmd == 'new':
            setup.new_ptau(args.out, args.power)
            print(json.dumps({'new': args.out, 'power': args.power, 'bytes': os.path.getsize(args.out), 'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}))
            return 0
        if not args.host:
            import zkcensus_amd
            ctx = zkcensus_amd.Context(args.device)
        where = 'host threads' if args.host else 'device'
        t0 = time.perf_counter()
        if args.cmd == 'contribute':
            h = setup.contribute_ptau(args.src, args.dst, ctx=ctx, name=args.name, verify=args.verify)
            print(json.dumps({'contributed': args.dst, 'hash': h.hex(), 'contributions': len(setup.ptau_contributions(args.dst)), 'path': where,
                              'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'stages_ms': {k: round(v, 2) for k, v in setup.ptau_contribute_stats().items()}}))
            return 0
        if len(args.files) > 2:
            ap.error('verify takes [prev.ptau] next.ptau')
        seed = None if args.seed is None else bytes.fromhex(args.seed)
        if seed is not None and len(seed) != 32:
            ap.error('--seed takes 64 hex digits')
        prev, nxt = (None, args.files[0]) if len(args.files) == 1 else args.files
        ok, n_new, why = setup.verify_ptau_contributions(prev, nxt, ctx=ctx, seed=seed)
        print(json.dumps({'verified': nxt, 'against': prev or 'a new file of its power', 'valid': ok, 'new_contributions': n_new, 'reason': why, 'path': where,
                          'call_ms': round((time.perf_counter() - t0) * 1e3, 1)}))
        return 0 if ok else 1
    except _native.ZkcError as e:
        print('refused: %s' % e, file=sys.stderr)
        return 1
    finally:
        if ctx is not None:
            ctx.close()


if __name__ == '__main__':
    sys.exit(main())
