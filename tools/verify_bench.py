"""Batch verifier timing: N proofs of the nLevels=160 circuit, one zkc_verify_batch call against N zkc_verify_bin calls.
`--bad k[,k...]` (N defaults to 8192): for each k, k randomly placed members get another proof's C and verify_each is timed next to verify_batch on the same inputs
(alternating, 10 repetitions each) and, for k > 0, next to N single verifications on 16 host threads; one JSON goes to profiles/verify_each_<N>.json."""
import json, os, random, statistics, sys, threading, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup, census, groth16, _native

def each_bench(ctx, vkb, pubs, proofs, N, ks, reps=10):
    lib = _native.load()
    ms = lambda f: (lambda t0: (f(), 1e3 * (time.perf_counter() - t0))[1])(time.perf_counter())
    out = {'N': N, 'nLevels': 160, 'repetitions': reps, 'cases': []}
    for k in ks:
        bad = sorted(random.Random(1000 + k).sample(range(N), k))
        buf = bytearray(proofs)
        for i in bad:
            j = (i + 1) % N; buf[256 * i + 192:256 * i + 256] = proofs[256 * j + 192:256 * j + 256]      # another proof's C: only the pairing equation can tell
        P = bytes(buf); seed = os.urandom(32)
        got = groth16.verify_each(ctx, vkb, pubs, P, seed); stats = groth16.verify_each_stats(ctx)
        assert [i for i, v in enumerate(got) if v] == bad and all(got[i] == groth16.PROOF_INVALID for i in bad)
        assert groth16.verify_batch(ctx, vkb, pubs, P, seed) is (k == 0)
        tb, te = [], []
        for _ in range(reps):                                            # alternating, same inputs, same process
            tb.append(ms(lambda: groth16.verify_batch(ctx, vkb, pubs, P, seed)))
            te.append(ms(lambda: groth16.verify_each(ctx, vkb, pubs, P, seed)))
        case = {'bad': k, 'verify_batch_ms': {'median': round(statistics.median(tb), 3), 'min': round(min(tb), 3), 'max': round(max(tb), 3)},
                'verify_each_ms': {'median': round(statistics.median(te), 3), 'min': round(min(te), 3), 'max': round(max(te), 3)},
                'stats': {'range_checks': stats[0], 'singles': stats[1], 'rounds_rebuilt': stats[2], 'budget_hit': stats[3]}}
        if k == 0:
            case['median_difference_ms'] = round(abs(statistics.median(te) - statistics.median(tb)), 3)
            case['verify_batch_spread_ms'] = round(max(tb) - min(tb), 3)
            case['within_spread'] = case['median_difference_ms'] <= case['verify_batch_spread_ms']
        else:
            one = lambda i: lib.zkc_verify_bin(vkb, 8, pubs[256 * i:256 * i + 256], P[256 * i:256 * i + 256])
            with ThreadPoolExecutor(16) as ex:
                t0 = time.perf_counter(); single = list(ex.map(one, range(N))); case['singles_16_threads_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
            assert [i for i, v in enumerate(single) if v != 1] == bad
            case['speedup_vs_singles'] = round(case['singles_16_threads_ms'] / case['verify_each_ms']['median'], 1)
        if k == 1:                                                       # peak device memory of a locating pass: free memory sampled while the call runs, against free memory after it
            low = [torch.cuda.mem_get_info()[0]]; stop = threading.Event()
            def sample():
                while not stop.is_set(): low[0] = min(low[0], torch.cuda.mem_get_info()[0]); time.sleep(0.0002)
            th = threading.Thread(target=sample); th.start()
            for _ in range(3): groth16.verify_each(ctx, vkb, pubs, P, seed)
            stop.set(); th.join()
            peak = torch.cuda.mem_get_info()[0] - low[0]
            case['locating_pass_peak_work_space_MB'] = round(peak / 2**20, 1); case['locating_pass_peak_KB_per_proof'] = round(peak / 1024 / N, 1)
        out['cases'].append(case)
    path = os.path.join(ROOT, 'profiles', 'verify_each_%d.json' % N)
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1); fh.write('\n')
    print(json.dumps(out))


def main():
    ks = None
    if '--bad' in sys.argv:
        at = sys.argv.index('--bad'); ks = [int(x) for x in sys.argv[at + 1].split(',')]; del sys.argv[at:at + 2]
    N = int(sys.argv[1]) if len(sys.argv) > 1 else (8192 if ks is not None else 1024)
    nl = 160
    _, zp, vp = setup.ensure_test_artifacts(nl)
    ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, open(zp, 'rb').read()); vk = json.load(open(vp))
    voters = census.synthetic_census(ctx, max(N, 64), nl)[:N]
    flat = b''.join(zkcensus_amd.flatten_inputs(v, nl) for v in voters)
    d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    nW = ctx.n_wires(nl)
    d_w = torch.empty(N * nW * 32, dtype=torch.uint8, device='cuda'); d_s = torch.zeros(N, dtype=torch.int32, device='cuda')
    rs = np.random.default_rng(3).integers(0, 256, size=(2 * N, 32), dtype=np.uint8); rs[:, 31] = 0
    proofs, pubs = pk.fullprove_batch_dev(d_in.data_ptr(), N, d_w.data_ptr(), d_s.data_ptr(), rs.tobytes())
    assert int(d_s.abs().sum().item()) == 0
    vkb = groth16.vk_to_bytes(vk)
    if ks is not None:
        return each_bench(ctx, vkb, pubs, proofs, N, ks)
    t0 = time.perf_counter(); groth16.verify_batch(ctx, vkb, pubs, proofs, os.urandom(32)); first = time.perf_counter() - t0      # the key is made ready, the kernels load, the work space is allocated
    cpu0 = time.process_time(); t0 = time.perf_counter(); ok = groth16.verify_batch(ctx, vkb, pubs, proofs, os.urandom(32)); t1 = time.perf_counter(); cpu1 = time.process_time()
    lib = _native.load(); k = min(N, 64)
    t2 = time.perf_counter()
    for i in range(k):
        assert lib.zkc_verify_bin(vkb, 8, pubs[256 * i:256 * i + 256], proofs[256 * i:256 * i + 256]) == 1
    t3 = time.perf_counter()
    bad = bytearray(proofs); bad[256 * (N // 2) + 192:256 * (N // 2) + 256] = proofs[192:256]       # one proof gets another proof's C
    rej = groth16.verify_batch(ctx, vkb, pubs, bytes(bad), os.urandom(32))
    print(json.dumps({'N': N, 'batch_valid': ok, 'tampered_batch_rejected': not rej, 'batch_verify_s': round(t1 - t0, 4), 'first_call_s': round(first, 3), 'proofs_per_s_batch': round(N / (t1 - t0), 1),
                      'single_verify_ms': round(1e3 * (t3 - t2) / k, 2), 'speedup_vs_single': round((t3 - t2) / k * N / (t1 - t0), 1), 'host_threads': min(32, os.cpu_count()), 'host_cpu_s_batch': round(cpu1 - cpu0, 3)}))

if __name__ == '__main__':
    main()
