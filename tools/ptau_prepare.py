"""`snarkjs powersoftau prepare phase2 in.ptau out.ptau` on the GPU (include/zkcensus_ptau_prepare.h):

    python tools/ptau_prepare.py in.ptau out.ptau [--check] [--host] [--device N]      out.ptau = in.ptau's sections, then the Lagrange sections 12 .. 15
    python tools/ptau_prepare.py prepared.ptau --check [--host]                         only check: are sections 12 .. 15 the transforms of sections 2 .. 5?

--check after a preparation checks the file just written.  --host: the transforms run on host threads and no GPU is touched; the bytes are the same.  Exit status 0: written
(and, with --check, confirmed); 1: refused, or the check names a point that differs.  Prints one JSON line per step with where the time went."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('src'); ap.add_argument('dst', nargs='?', default=None)
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--device', type=int, default=0)
    args = ap.parse_args()
    if args.dst is None and not args.check:
        ap.error('give an output file, or --check for a prepared one')
    from zkcensus_amd import setup, _native
    ctx = None
    if not args.host:
        import zkcensus_amd
        ctx = zkcensus_amd.Context(args.device)
    where = 'host threads' if args.host else 'device'
    try:
        target = args.src
        if args.dst is not None:
            t0 = time.perf_counter()
            setup.prepare_ptau(args.src, args.dst, ctx=ctx)
            print(json.dumps({'prepared': args.dst, 'bytes': os.path.getsize(args.dst), 'path': where, 'call_ms': round((time.perf_counter() - t0) * 1e3, 1),
                              'stages_ms': {k: round(v, 2) for k, v in setup.ptau_prepare_stats().items()}}))
            target = args.dst
        if args.check:
            t0 = time.perf_counter()
            ok, section, index, why = setup.check_prepared(target, ctx=ctx)
            print(json.dumps({'checked': target, 'valid': ok, 'section': section, 'index': index, 'reason': why, 'path': where,
                              'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'stages_ms': {k: round(v, 2) for k, v in setup.ptau_prepare_stats().items()}}))
            if not ok:
                return 1
    except _native.ZkcError as e:
        print('refused: %s' % e, file=sys.stderr)
        return 1
    finally:
        if ctx is not None:
            ctx.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
