"""Check every voter's census proof of a --n voter tree in one batch (census.check_proofs, zkc_smt_check_proofs, csrc/zkc_smt_check.hip) and time it.

Builds the tree with zkc_smt_build (random 160-bit addresses, weights 1..100), takes every voter's zero-padded proof, then times zkc_smt_check_proofs over all of
them against the tree's root.  Prints one JSON line: host-to-host proofs/s (host buffers in, verdicts in host memory; median of --reps calls), the split of the last call
into host work (checks, depth sort, compaction), host-to-device copies and kernels, the bytes uploaded against the zero-padded layout, the depth histogram, the kernels'
Poseidons per second, and a labelled CPU baseline: the oracle's Poseidon climb (C, one ctypes call per hash) on the host's threads over --cpu-sample proofs.
--ab also times small batches in the wave-per-proof form against the lane-per-proof form (ZKC_SMT_WAVE_MAX), alternating the two."""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import zkcensus_amd
from zkcensus_amd import census


def words(a):
    """(n, k) uint8 little-endian rows -> (n, 32) uint8"""
    out = np.zeros((a.shape[0], 32), dtype=np.uint8); out[:, :a.shape[1]] = a
    return out


def ptr(a):
    return ctypes.c_char_p(a.ctypes.data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--nlevels', type=int, default=160)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-sample', type=int, default=4096, help='proofs in the CPU baseline (0: skip it)')
    ap.add_argument('--ab', default='1,8,64,256,1024,4096', help='batch sizes of the wave / lane A/B (empty: skip it)')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    n, nl = a.n, a.nlevels
    rng = np.random.default_rng(a.seed)
    keys = words(rng.integers(0, 256, size=(n, 20), dtype=np.uint8))
    vals = words(rng.integers(1, 101, size=(n, 1), dtype=np.uint8))
    ctx = zkcensus_amd.Context(0)
    L = ctx._lib
    sib = np.empty(n * (nl + 1) * 32, dtype=np.uint8)
    dep = np.empty(n, dtype=np.int32)
    root = ctypes.create_string_buffer(32)
    ctx._check(L.zkc_smt_build(ctx._h, ptr(keys), ptr(vals), n, nl, root, ptr(sib), dep.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    st = np.empty(n, dtype=np.int32)

    def check(m, per=0, roots=root):
        ctx._check(L.zkc_smt_check_proofs(ctx._h, nl, m, ptr(keys), ptr(vals), ptr(sib), roots, per, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    res = {'tool': 'census_check', 'n': n, 'nLevels': nl}
    check(n)                                                  # warm-up: code objects, pinned buffers
    assert not st.any(), 'a valid proof was refused'
    ts = []
    for _ in range(a.reps):
        st[:] = -1
        t0 = time.perf_counter(); check(n); ts.append(time.perf_counter() - t0)
        assert not st.any(), 'a valid proof was refused'
    host, up, kern = census.check_stats(ctx)
    med = statistics.median(ts)
    hashes = int(dep.sum()) + n
    hist = np.bincount(dep)
    res['call_ms'] = {'median': round(1e3 * med, 2), 'min': round(1e3 * min(ts), 2), 'max': round(1e3 * max(ts), 2)}
    res['proofs_per_s_host_to_host'] = round(n / med)
    res['last_call_ms'] = {'host_checks_sort_compaction': round(host, 2), 'h2d': round(up, 2), 'kernels': round(kern, 2)}
    res['bytes_uploaded'] = n * 3 * 32 + 4 * n + 32 * int(dep.sum())        # keys, values, offsets, compacted siblings (the shared root and alignment left out)
    res['bytes_zero_padded_layout'] = n * 2 * 32 + n * (nl + 1) * 32
    res['depth_histogram'] = {str(d): int(c) for d, c in enumerate(hist) if c}
    res['depth_mean'] = round(float(dep.mean()), 2)
    res['poseidons'] = hashes
    res['kernel_poseidons_per_s'] = round(hashes / (kern / 1e3)) if kern else None
    res['h2d_GB_per_s'] = round(res['bytes_uploaded'] / (up / 1e3) / 1e9, 1) if up else None
    # the CPU baseline
    if a.cpu_sample:
        import oracle_lib as ol
        pick = rng.choice(n, size=min(a.cpu_sample, n), replace=False)
        r = int.from_bytes(root.raw, 'little')
        blk = 32 * (nl + 1)

        def climb(i):
            k = int.from_bytes(keys[i].tobytes(), 'little'); v = int.from_bytes(vals[i].tobytes(), 'little')
            s = sib[blk * i:blk * (i + 1)].tobytes()
            cur = ol.poseidon([k, v, 1])
            for l in range(int(dep[i]) - 1, -1, -1):
                x = int.from_bytes(s[32 * l:32 * l + 32], 'little')
                cur = ol.poseidon([x, cur]) if (k >> l) & 1 else ol.poseidon([cur, x])
            return cur == r
        ol.lib()
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
        t0 = time.perf_counter(); ok = ol.pmap(climb, pick.tolist(), threads); dt = time.perf_counter() - t0
        assert all(ok)
        res['cpu_baseline'] = {'what': 'oracle Poseidon climb (C via ctypes, one call per hash) on host threads', 'threads': threads, 'proofs': len(pick),
                               'proofs_per_s': round(len(pick) / dt), 'gpu_speedup_host_to_host': round((n / med) / (len(pick) / dt), 1)}
    # wave-per-proof (the default for <= 64 proofs; forced here for every size measured) against lane-per-proof (ZKC_SMT_WAVE_MAX=0), alternating, 21 calls each after a warm-up
    sizes = [int(x) for x in a.ab.split(',') if x]
    if sizes:
        ab = {}
        for m in sizes:
            t = {'wave': [], 'lane': []}
            for rep in range(22):
                for form in ('wave', 'lane'):
                    os.environ['ZKC_SMT_WAVE_MAX'] = str(m) if form == 'wave' else '0'
                    t0 = time.perf_counter(); check(m); dt = time.perf_counter() - t0
                    assert not st[:m].any()
                    if rep:
                        t[form].append(dt)
            ab[str(m)] = {f: round(1e3 * statistics.median(x), 3) for f, x in t.items()}
            ab[str(m)]['depths'] = [int(dep[:m].min()), int(dep[:m].max())]
        os.environ.pop('ZKC_SMT_WAVE_MAX')
        res['small_batch_call_ms_wave_vs_lane'] = ab
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
