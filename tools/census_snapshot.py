"""Snapshots of a resident census tree (census.CensusTree.snapshot, zkc_tree_snapshot in csrc/zkc_tree.hip): what freezing a census costs while it goes on changing.

Builds an --n voter tree in one add (random 160-bit addresses, weights 1..100) and a SIK tree over the same addresses, then:
- times taking and releasing a snapshot of the untouched tree;
- with 0, 1 and 8 live snapshots, --rounds rounds of one add, one update and one delete of --batch voters each, every call timed and split into host trie time and
  device time.  A fresh snapshot is taken before every round and the oldest released beyond the count, so every measured change is the first after a snapshot:
  it copies the most paths.  Per call also the growth of refs()[0] (live node references), and the snapshot take / release times;
- holds one snapshot through 32 more change calls, then times gen_proof of --batch voters and census_inputs_from_trees(tree, SIK tree) for them on the snapshot and
  on the live tree, alternating; checks the snapshot's root against zkc_smt_build over its recorded set (asserted) and the live root against the live set.
Prints one JSON line."""
import argparse, collections, ctypes, json, os, statistics, sys, time
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
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--nlevels', type=int, default=160)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    n, nl, B = a.n, a.nlevels, a.batch
    held_calls = 32
    total = n + B * (3 * a.rounds + held_calls // 3 + 1)
    rng = np.random.default_rng(a.seed)
    addr = words(rng.integers(0, 256, size=(total, 20), dtype=np.uint8))
    weight = words(rng.integers(1, 101, size=(total, 1), dtype=np.uint8))
    pw = words(rng.integers(0, 256, size=(total, 11), dtype=np.uint8))
    sig = words(rng.integers(0, 256, size=(total, 31), dtype=np.uint8))
    ctx = zkcensus_amd.Context(0)
    L = ctx._lib
    res = {'tool': 'census_snapshot', 'n': n, 'batch': B, 'nLevels': nl, 'rounds': a.rounds}
    tree = census.CensusTree(ctx, nl)
    assert not any(tree.add(addr[:n].tobytes(), weight[:n].tobytes()))
    alive = np.zeros(total, dtype=bool); alive[:n] = True
    nxt = n                                                    # next fresh address
    res['refs_full'] = list(tree.refs())
    # take / release on the untouched tree: O(1), no device work
    take, rel = [], []
    for _ in range(201):
        h = ctypes.c_void_p()
        t0 = time.perf_counter(); ctx._check(L.zkc_tree_snapshot(tree._h, ctypes.byref(h))); t1 = time.perf_counter()
        L.zkc_tree_free(h); t2 = time.perf_counter()
        take.append(1e6 * (t1 - t0)); rel.append(1e6 * (t2 - t1))
    res['snapshot_take_us_median'] = round(statistics.median(take), 2)
    res['snapshot_release_untouched_us_median'] = round(statistics.median(rel), 2)

    def change(op):
        """one timed change call of B voters: (call ms, host trie ms, device ms, refs()[0] growth)"""
        nonlocal nxt
        r0 = tree.refs()[0]
        if op == 'add':
            q = np.arange(nxt, nxt + B); nxt += B
            t0 = time.perf_counter(); st = tree.add(addr[q].tobytes(), weight[q].tobytes()); ms = 1e3 * (time.perf_counter() - t0)
            alive[q] = True
        else:
            q = rng.choice(np.flatnonzero(alive), size=B, replace=False)
            if op == 'update':
                weight[q] = words(rng.integers(1, 101, size=(B, 1), dtype=np.uint8))
                t0 = time.perf_counter(); st = tree.update(addr[q].tobytes(), weight[q].tobytes()); ms = 1e3 * (time.perf_counter() - t0)
            else:
                t0 = time.perf_counter(); st = tree.delete(addr[q].tobytes()); ms = 1e3 * (time.perf_counter() - t0)
                alive[q] = False
        assert not any(st), op + ' refused entries'
        return (ms, *tree.stats(), tree.refs()[0] - r0)
    med = lambda xs, k: round(statistics.median(x[k] for x in xs), 3)
    res['by_live_snapshots'] = {}
    for k in (0, 1, 8):
        held = collections.deque()
        rows = {'add': [], 'update': [], 'delete': []}
        take, rel = [], []
        for _ in range(a.rounds):
            if k:
                t0 = time.perf_counter(); held.append(tree.snapshot()); take.append(1e3 * (time.perf_counter() - t0))
                while len(held) > k:
                    t0 = time.perf_counter(); held.popleft().close(); rel.append(1e3 * (time.perf_counter() - t0))
                assert tree.snapshot_count() == len(held)
            for op in rows:
                rows[op].append(change(op))
        refs_held = list(tree.refs())
        while held:
            t0 = time.perf_counter(); held.popleft().close(); rel.append(1e3 * (time.perf_counter() - t0))
        out = {}
        for op, xs in rows.items():
            out[op] = {'call_ms': med(xs, 0), 'call_ms_max': round(max(x[0] for x in xs), 3), 'host_trie_ms': med(xs, 1), 'device_ms': med(xs, 2),
                       'refs_growth': int(statistics.median(x[3] for x in xs))}
        if k:
            out['take_ms_median'] = round(statistics.median(take), 4)
            out['release_ms_median'] = round(statistics.median(rel), 3)
            out['release_ms_max'] = round(max(rel), 3)
        out['refs_with_snapshots_held'] = refs_held
        out['refs_after_release'] = list(tree.refs())
        res['by_live_snapshots'][str(k)] = out
    base = res['by_live_snapshots']['0']
    for k in ('1', '8'):
        cur = res['by_live_snapshots'][k]
        res['by_live_snapshots'][k]['refs_held_per_batch'] = {op: cur[op]['refs_growth'] - base[op]['refs_growth'] for op in ('add', 'update', 'delete')}
        res['by_live_snapshots'][k]['add_over_no_snapshot'] = round(cur['add']['call_ms'] / base['add']['call_ms'], 3)
    # one snapshot held through 32 change calls: proofs and circuit inputs against its frozen root
    flat = np.concatenate([addr, pw, sig], axis=1).tobytes()
    sikb = ctypes.create_string_buffer(32 * total)
    ctx._check(L.zkc_poseidon_batch(ctx._h, 3, flat, total, sikb))
    sik = np.frombuffer(sikb.raw, dtype=np.uint8).reshape(total, 32)
    stree = census.CensusTree(ctx, nl)
    assert not any(stree.add(addr.tobytes(), sik.tobytes()))
    snap = tree.snapshot()
    frozen_alive, frozen_weight = alive.copy(), weight.copy()
    r0 = tree.refs()[0]
    for c in range(held_calls):
        change(('add', 'update', 'delete')[c % 3])
    res['held_calls'] = held_calls
    res['refs_growth_over_held_calls'] = tree.refs()[0] - r0
    q = rng.choice(np.flatnonzero(frozen_alive & alive), size=B, replace=False)
    kb = addr[q].tobytes()
    eid = [int(x) for x in census.bytes_to_arbo(bytes.fromhex(census.ELECTION_ID_HEX))]

    def proofs(t):
        r, sib, dep, ex = t.gen_proof(kb)
        assert all(ex)

    def inputs(t):
        blocks, cr, sr, st = census.census_inputs_from_trees(ctx, t, stree, eid, kb, pw[q].tobytes(), sig[q].tobytes(), [1] * B, [(1, 2)] * B)
        assert not any(st) and cr == t.root
    for what, fn in (('gen_proof', proofs), ('census_inputs_from_trees', inputs)):
        fn(snap); fn(tree)                                     # warm-up: output buffers
        ts = {'snapshot': [], 'live': []}
        for _ in range(7):                                     # snapshot and live tree alternating
            for name, t in (('snapshot', snap), ('live', tree)):
                t0 = time.perf_counter(); fn(t); ts[name].append(1e3 * (time.perf_counter() - t0))
        for name in ts:
            res['%s_ms_%s' % (what, name)] = round(statistics.median(ts[name]), 3)
    froot, _, _ = census.smt_build(ctx, addr[frozen_alive].tobytes(), frozen_weight[frozen_alive].tobytes(), nl, siblings=False)
    lroot, _, _ = census.smt_build(ctx, addr[alive].tobytes(), weight[alive].tobytes(), nl, siblings=False)
    res['snapshot_root_equals_rebuild'] = snap.root == froot and len(snap) == int(frozen_alive.sum())
    res['live_root_equals_rebuild'] = tree.root == lroot and len(tree) == int(alive.sum())
    assert res['snapshot_root_equals_rebuild'] and res['live_root_equals_rebuild'], 'a root differs from its rebuild'
    t0 = time.perf_counter(); snap.close(); res['release_after_held_calls_ms'] = round(1e3 * (time.perf_counter() - t0), 3)
    res['refs_after_release'] = list(tree.refs())
    stree.close(); tree.close(); ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
