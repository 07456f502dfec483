"""Grow a census tree in place (census.CensusTree, csrc/zkc_tree.hip) to --n voters in --batch-sized adds and time it against the static rebuild (zkc_smt_build).

Prints one JSON line: per batch size the median ms of an add call, split into host trie time and device time (upload, kernels, synchronise); the ms of gen_proof and
of census_inputs_from_trees over one batch; the ms of one whole-census add and of one zkc_smt_build over the final set; and whether the roots agree (asserted).
Keys are random 160-bit addresses, weights 1..100; the SIK tree is filled with one whole-census add."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--probe', default='1,64,1024,16384', help='batch sizes timed again on the full tree (5 adds each)')
    ap.add_argument('--nlevels', type=int, default=160)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    probes = [int(x) for x in a.probe.split(',') if x]
    extra = 5 * sum(probes)
    total = a.n + extra
    addr = words(rng.integers(0, 256, size=(total, 20), dtype=np.uint8))
    weight = words(rng.integers(1, 101, size=(total, 1), dtype=np.uint8))
    pw = words(rng.integers(0, 256, size=(total, 11), dtype=np.uint8))
    sig = words(rng.integers(0, 256, size=(total, 31), dtype=np.uint8))
    ctx = zkcensus_amd.Context(0)
    tree = census.CensusTree(ctx, a.nlevels)
    res = {'tool': 'census_grow', 'n': a.n, 'batch': a.batch, 'nLevels': a.nlevels}

    def add(t, lo, hi):
        t0 = time.perf_counter()
        st = t.add(addr[lo:hi].tobytes(), weight[lo:hi].tobytes())
        ms = 1e3 * (time.perf_counter() - t0)
        assert not any(st), 'add refused entries'
        h, d = t.stats()
        return ms, h, d
    # growth: every add timed; the medians over the whole growth and over the last 64 adds (tree within 64 batches of --n)
    grow = [add(tree, lo, min(a.n, lo + a.batch)) for lo in range(0, a.n, a.batch)]
    med = lambda xs, k: round(statistics.median(x[k] for x in xs), 3)
    res['grow_total_s'] = round(sum(x[0] for x in grow) / 1e3, 3)
    res['grow_add_ms_median'] = {'call': med(grow, 0), 'host_trie': med(grow, 1), 'device': med(grow, 2)}
    res['grow_add_ms_median_last64'] = {'call': med(grow[-64:], 0), 'host_trie': med(grow[-64:], 1), 'device': med(grow[-64:], 2)}
    # batch sizes on the full tree
    lo = a.n
    res['add_ms_median_by_batch'] = {}
    for b in probes:
        xs = []
        for _ in range(5):
            xs.append(add(tree, lo, lo + b)); lo += b
        res['add_ms_median_by_batch'][str(b)] = {'call': med(xs, 0), 'host_trie': med(xs, 1), 'device': med(xs, 2)}
    assert lo == total and len(tree) == total
    # gen_proof over one batch of voters already in the tree
    q = rng.choice(total, size=a.batch, replace=False)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); r, sib, dep, ex = tree.gen_proof(addr[q].tobytes()); ts.append(1e3 * (time.perf_counter() - t0))
        assert all(ex)
    res['gen_proof_ms'] = round(statistics.median(ts), 3)
    res['gen_proof_max_depth'] = max(dep)
    # the SIK tree in one whole-census add, then the circuit inputs of one batch from both trees
    flat = np.concatenate([addr, pw, sig], axis=1).tobytes()
    sikb = ctypes.create_string_buffer(32 * total)
    ctx._check(ctx._lib.zkc_poseidon_batch(ctx._h, 3, flat, total, sikb))
    sik = np.frombuffer(sikb.raw, dtype=np.uint8).reshape(total, 32)
    stree = census.CensusTree(ctx, a.nlevels)
    t0 = time.perf_counter()
    assert not any(stree.add(addr.tobytes(), sik.tobytes()))
    res['whole_census_add_ms'] = {'call': round(1e3 * (time.perf_counter() - t0), 3), 'host_trie': round(stree.stats()[0], 3), 'device': round(stree.stats()[1], 3)}
    eid = [int(x) for x in census.bytes_to_arbo(bytes.fromhex(census.ELECTION_ID_HEX))]
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        blocks, cr, sr, st = census.census_inputs_from_trees(ctx, tree, stree, eid, addr[q].tobytes(), pw[q].tobytes(), sig[q].tobytes(), [1] * a.batch, [(1, 2)] * a.batch)
        ts.append(1e3 * (time.perf_counter() - t0))
        assert not any(st)
    res['census_inputs_from_trees_ms'] = round(statistics.median(ts), 3)
    # the static rebuild over the final set, and the roots
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); root, _, _ = census.smt_build(ctx, addr.tobytes(), weight.tobytes(), a.nlevels, siblings=False); ts.append(1e3 * (time.perf_counter() - t0))
    res['rebuild_smt_build_ms'] = round(statistics.median(ts), 3)
    sroot, _, _ = census.smt_build(ctx, addr.tobytes(), sik.tobytes(), a.nlevels, siblings=False)
    res['roots_equal'] = tree.root == root == cr and stree.root == sroot == sr
    assert res['roots_equal'], 'incremental and rebuilt roots differ'
    probe = res['add_ms_median_by_batch'].get('1024')
    res['rebuild_over_add_1024'] = round(res['rebuild_smt_build_ms'] / probe['call'], 1) if probe else None
    stree.close(); tree.close(); ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
