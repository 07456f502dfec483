"""Helper of tests/test_gpu_lane_streams.py.  It runs as a child process, because ZKC_LANE_STREAMS, ZKC_LANES, ZKC_INFLIGHT and ZKC_SERIAL_STREAMS are read when a key is
loaded and every other test keeps the defaults.  argv[1] names a scenario; each proves fixed nLevels-10 voters, inputs -> witness -> proof, with fixed (r, s) and prints one
JSON line: the bytes of every call (proofs, then public signals, as hex), the number of streams each call was enqueued on (zkc_zkey_call_streams), the key's pass size and
lanes, and -- with argv[2] == 'oracle' -- for a sample of proofs whether the CPU oracle gives the same bytes."""
import json, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import setup
from census_gen import random_voter
import synth_voter
import oracle_lib as ol

NL = 10
scenario, with_oracle = sys.argv[1], sys.argv[2:] == ['oracle']
_, zp, _ = setup.ensure_test_artifacts(NL)
zk = open(zp, 'rb').read()
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
nW, nIn = ctx.n_wires(NL), ctx.n_inputs(NL)
rng = random.Random(20261021)
H = lambda xs: synth_voter.H(*xs)


class Voters:
    """B voters of random depths, their input blocks on the device, a witness buffer and fixed (r, s)"""
    def __init__(self, B):
        self.B = B
        vs = [random_voter(rng, H, nLevels=NL, depth_c=rng.randint(0, NL), depth_s=rng.randint(0, NL)) for _ in range(B)]
        flat = b''.join(zkcensus_amd.flatten_inputs(v, NL) for v in vs)
        self.rs_int = [(rng.randrange(1, ol.R), rng.randrange(1, ol.R)) for _ in range(B)]
        self.rs = b''.join(x.to_bytes(32, 'little') for p in self.rs_int for x in p)
        self.d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
        self.d_w = torch.empty(B * nW * 32, dtype=torch.uint8, device='cuda'); self.d_st = torch.zeros(B, dtype=torch.int32, device='cuda')

    def args(self, first=0, b=None):
        b = self.B - first if b is None else b
        return self.d_in.data_ptr() + first * nIn * 32, b, self.d_w.data_ptr() + first * nW * 32, self.d_st.data_ptr() + first * 4, self.rs[64 * first:64 * (first + b)]

    def accepted(self):
        return int(self.d_st.abs().sum().item()) == 0

    def oracle_equal(self, proofs, pubs, sample, first=0):
        """for proof q of a call that began at voter `first`: the oracle's proof and public signals from the witness the call left on the device"""
        npub = len(pubs) // (len(proofs) // 256)
        def one(q):
            w = bytes(self.d_w[(first + q) * nW * 32:(first + q + 1) * nW * 32].cpu().numpy())
            return w, self.rs_int[first + q]
        jobs = [one(q) for q in sample]
        got = ol.pmap(lambda j: ol.prove(zk, j[0], *j[1]), jobs)
        return [bool(rc == 0 and p == proofs[256 * q:256 * q + 256] and u == pubs[npub * q:npub * q + npub]) for q, (rc, p, u) in zip(sample, got)]


out = {'pass_size': pk.pass_size, 'lanes': pk.lanes, 'calls': [], 'streams': []}


def record(p, u):
    out['calls'].append((p + u).hex()); out['streams'].append(pk.call_streams())


if scenario == 'plan':
    # one call of 163 voters: with ZKC_INFLIGHT=32 six passes, so the rotation wraps past lane 3, the last of them short
    v = Voters(163)
    p, u = pk.fullprove_batch_dev(*v.args())
    assert v.accepted()
    record(p, u)
    per = -(-v.B // -(-v.B // pk.pass_size))                  # proofs per pass (plan::call_split)
    sample = sorted({0, v.B - 1} | {q for k in range(per, v.B, per) for q in (k - 1, k)})
    out['per'] = per; out['sample'] = sample
    if with_oracle:
        out['oracle_equal'] = v.oracle_equal(p, u, sample)
elif scenario == 'pipelined':
    # two calls in flight, eight times: begin(0), begin(1), finish(0), finish(1); 65 voters per call (two passes of a key loaded with ZKC_INFLIGHT=64)
    a, b = Voters(65), Voters(65)
    for rnd in range(8):
        pk.batch_begin(0, *a.args()); pk.batch_begin(1, *b.args())
        streams = pk.call_streams()
        pa, ua = pk.batch_finish(0, a.B); pb, ub = pk.batch_finish(1, b.B)
        assert a.accepted() and b.accepted()
        out['calls'].append((pa + ua).hex()); out['calls'].append((pb + ub).hex()); out['streams'].append(streams)
    if with_oracle:
        out['oracle_equal'] = a.oracle_equal(pa, ua, [0, 32, 33, 64]) + b.oracle_equal(pb, ub, [0, 32, 33, 64])
elif scenario == 'tree':
    # a call of one voter and a call of two (the tree shape of a pass: its blinding's variable-base products ride as MSM jobs) between calls that rotate over the lanes
    v = Voters(70)
    for first, b in ((0, 70), (3, 1), (0, 70), (5, 2), (0, 70)):
        p, u = pk.fullprove_batch_dev(*v.args(first, b))
        assert v.accepted()
        record(p, u)
        if with_oracle and b <= 2:
            out.setdefault('oracle_equal', []).extend(v.oracle_equal(p, u, list(range(b)), first))
elif scenario == 'mixed':
    # two calls in flight on one key whose plans differ: a rotating call (163 voters, six passes: lane 0 carries passes 0 and 4 with the G2 MSM on its st) and a call of one
    # pass (20 voters, or 2: the tree shape), which lands on lane 0 with the G2 MSM on st2 -- the lane has ONE G2 work space.  Both orders, three times each, after the
    # synchronous calls whose bytes every pipelined call has to repeat
    big, mid, two = Voters(163), Voters(20), Voters(2)
    for v in (big, mid, two):
        p, u = pk.fullprove_batch_dev(*v.args())
        assert v.accepted()
        record(p, u)
    out['pipelined'] = []
    for small in (mid, two):
        for first, second in ((big, small), (small, big)):
            for rnd in range(3):
                pk.batch_begin(0, *first.args()); s0 = pk.call_streams()
                pk.batch_begin(1, *second.args()); s1 = pk.call_streams()
                r0 = pk.batch_finish(0, first.B); r1 = pk.batch_finish(1, second.B)
                assert first.accepted() and second.accepted()
                out['pipelined'].append({'sizes': [first.B, second.B], 'streams': [s0, s1], 'calls': [(r0[0] + r0[1]).hex(), (r1[0] + r1[1]).hex()]})
elif scenario == 'tiny':
    # three voters through a key loaded with ZKC_INFLIGHT=2: passes of 2 and 1 proofs on lanes 0 and 1 -- tree-shaped passes INSIDE a rotating call (plan::call_split
    # equalises passes, so a larger pass size never leaves such a stub) -- each proof against the oracle
    v = Voters(3)
    for rnd in range(2):
        p, u = pk.fullprove_batch_dev(*v.args())
        assert v.accepted()
        record(p, u)
    out['oracle_equal'] = v.oracle_equal(p, u, [0, 1, 2])
else:
    raise SystemExit('unknown scenario')
print(json.dumps(out))
pk.close(); ctx.close()
