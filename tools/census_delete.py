"""Remove voters from a resident census tree and prove keys absent (census.CensusTree.delete / gen_absence_proof, csrc/zkc_tree.hip; census.check_absence,
csrc/zkc_smt_check.hip) and time it against the static rebuild (zkc_smt_build).

Builds an --n voter tree in one add (random 160-bit addresses, weights 1..100), then:
- deletes --batches batches of --batch voters, each call timed and split into host trie time and device time, and rebuilds the remaining set once with zkc_smt_build
  (the roots are asserted equal);
- takes one gen_absence_proof over --absent random addresses the tree does not hold, and checks them all in one check_absence call against the tree's root (--reps calls;
  every verdict asserted VALID), with the last call's host / copy / kernel split.
Prints one JSON line."""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import zkcensus_amd
from zkcensus_amd import census


def words(a):
    """(n, k) uint8 little-endian rows -> (n, 32) uint8"""
    out = np.zeros((a.shape[0], 32), dtype=np.uint8); out[:, :a.shape[1]] = a
    return out


def ptr(a):
    return ctypes.c_char_p(a.ctypes.data)


def i32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--batches', type=int, default=32)
    ap.add_argument('--absent', type=int, default=1 << 20)
    ap.add_argument('--nlevels', type=int, default=160)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    n, nl, m = a.n, a.nlevels, a.absent
    rng = np.random.default_rng(a.seed)
    addr = words(rng.integers(0, 256, size=(n + m, 20), dtype=np.uint8))
    weight = words(rng.integers(1, 101, size=(n, 1), dtype=np.uint8))
    absent = addr[n:]; addr = addr[:n]                 # 2^-160 per pair to collide: the absent keys are absent
    ctx = zkcensus_amd.Context(0)
    L = ctx._lib
    res = {'tool': 'census_delete', 'n': n, 'batch': a.batch, 'nLevels': nl}
    tree = census.CensusTree(ctx, nl)
    t0 = time.perf_counter()
    assert not any(tree.add(addr.tobytes(), weight.tobytes()))
    res['build_by_one_add_ms'] = round(1e3 * (time.perf_counter() - t0), 3)
    res['refs_full'] = list(tree.refs())
    # deletes: batches of random voters, every call timed
    order = rng.permutation(n)[:a.batch * a.batches]
    xs = []
    for b in range(a.batches):
        q = order[a.batch * b:a.batch * (b + 1)]
        t0 = time.perf_counter(); st = tree.delete(addr[q].tobytes()); ms = 1e3 * (time.perf_counter() - t0)
        assert not any(st), 'delete refused entries'
        xs.append((ms, *tree.stats()))
    med = lambda k: round(statistics.median(x[k] for x in xs), 3)
    res['delete_ms_median'] = {'call': med(0), 'host_trie': med(1), 'device': med(2)}
    res['delete_ms_min_max'] = [round(min(x[0] for x in xs), 3), round(max(x[0] for x in xs), 3)]
    res['refs_after_deletes'] = list(tree.refs())
    keep = np.ones(n, dtype=bool); keep[order] = False
    rk, rw = addr[keep], weight[keep]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); root, _, _ = census.smt_build(ctx, rk.tobytes(), rw.tobytes(), nl, siblings=False); ts.append(1e3 * (time.perf_counter() - t0))
    res['rebuild_smt_build_ms'] = round(statistics.median(ts), 3)
    res['remaining'] = int(keep.sum())
    res['roots_equal'] = tree.root == root and len(tree) == res['remaining']
    assert res['roots_equal'], 'the tree after deletes and the rebuild differ'
    res['rebuild_over_delete'] = round(res['rebuild_smt_build_ms'] / res['delete_ms_median']['call'], 1)
    # absence proofs: one gen_absence_proof over every absent key, then check_absence over all of them
    sib = np.empty(m * (nl + 1) * 32, dtype=np.uint8)
    dep = np.empty(m, dtype=np.int32); o0 = np.empty(m, dtype=np.int32); st = np.empty(m, dtype=np.int32)
    ok = np.empty((m, 32), dtype=np.uint8); ov = np.empty((m, 32), dtype=np.uint8)
    rb = ctypes.create_string_buffer(32)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx._check(L.zkc_tree_gen_absence_proof(tree._h, ptr(absent), m, rb, sib.ctypes.data, i32(dep), ok.ctypes.data, ov.ctypes.data, i32(o0), i32(st)))
        ts.append(1e3 * (time.perf_counter() - t0))
    assert not st.any() and rb.raw == tree.root.to_bytes(32, 'little')
    res['gen_absence_proof_ms'] = round(statistics.median(ts), 3)
    res['gen_absence_proofs_per_s'] = round(m / (statistics.median(ts) / 1e3))
    res['absent'] = m
    res['is_old0_share'] = round(float(o0.mean()), 4)
    res['absence_depth_mean'] = round(float(dep.mean()), 2)

    def check():
        ctx._check(L.zkc_smt_check_absence(ctx._h, nl, m, ptr(absent), ptr(ok), ptr(ov), i32(o0), ptr(sib), rb, 0, i32(st)))
    check()                                                   # warm-up: code objects, pinned buffers
    assert not st.any(), 'a valid absence proof was refused'
    ts = []
    for _ in range(a.reps):
        st[:] = -1
        t0 = time.perf_counter(); check(); ts.append(time.perf_counter() - t0)
        assert not st.any(), 'a valid absence proof was refused'
    host, up, kern = census.check_stats(ctx)
    medc = statistics.median(ts)
    hashes = int(dep.sum()) + int((o0 == 0).sum())
    res['check_absence_ms'] = {'median': round(1e3 * medc, 2), 'min': round(1e3 * min(ts), 2), 'max': round(1e3 * max(ts), 2)}
    res['check_absence_proofs_per_s_host_to_host'] = round(m / medc)
    res['check_absence_last_call_ms'] = {'host_checks_sort_compaction': round(host, 2), 'h2d': round(up, 2), 'kernels': round(kern, 2)}
    res['check_absence_poseidons'] = hashes
    res['check_absence_kernel_poseidons_per_s'] = round(hashes / (kern / 1e3)) if kern else None
    tree.close(); ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
