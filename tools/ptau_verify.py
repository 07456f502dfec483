"""The point checks of `snarkjs powersoftau verify` on the GPU (include/zkcensus_ptau_verify.h): is the file the powers of one tau, one alpha and one beta?

    python tools/ptau_verify.py file.ptau [--prepared] [--host] [--device N] [--seed HEX64]

Sections 2 .. 6 of a prepared or unprepared file are checked (setup.verify_ptau); --prepared also checks that sections 12 .. 15 are the transforms of sections 2 .. 5
(setup.check_prepared): the two together are `powersoftau verify` without the contribution transcript of section 7.  --host: the sums run on host threads and no GPU is
touched; the verdict is the same.  --seed: 32 bytes in hex make the weights reproducible; without it they come from the OS, which is what a verifier wants.  Exit status
0: valid; 1: not valid (the line names the check) or refused.  Prints one JSON line per step with the verdict and where the time went."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('ptau')
    ap.add_argument('--prepared', action='store_true')
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--seed', default=None)
    args = ap.parse_args()
    seed = None if args.seed is None else bytes.fromhex(args.seed)
    if seed is not None and len(seed) != 32:
        ap.error('--seed takes 64 hex digits')
    from zkcensus_amd import setup, _native
    ctx = None
    if not args.host:
        import zkcensus_amd
        ctx = zkcensus_amd.Context(args.device)
    where = 'host threads' if args.host else 'device'
    try:
        t0 = time.perf_counter()
        ok, check, section, index, why = setup.verify_ptau(args.ptau, ctx=ctx, seed=seed)
        print(json.dumps({'verified': args.ptau, 'valid': ok, 'check': setup.PTAU_CHECKS[check], 'section': section, 'index': index, 'reason': why, 'path': where,
                          'call_ms': round((time.perf_counter() - t0) * 1e3, 1), 'stages_ms': {k: round(v, 2) for k, v in setup.ptau_verify_stats().items()}}))
        if not ok:
            return 1
        if args.prepared:
            t0 = time.perf_counter()
            ok, section, index, why = setup.check_prepared(args.ptau, ctx=ctx)
            print(json.dumps({'checked': args.ptau, 'valid': ok, 'section': section, 'index': index, 'reason': why, 'path': where,
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
