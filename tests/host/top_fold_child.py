"""Helper of tests/test_gpu_top_fold.py.  It runs as a child process, because ZKC_TOP_FOLD and ZKC_TEST_TOP_SLOTS are read when a key is loaded and every other test keeps
the default.  argv[1] names a scenario; each proves nLevels-10 voters through the public prove calls with fixed (r, s), compares every proof and public-signal block with
the CPU oracle's, reads the G1 additions of each call (zkc_profile_read, category 7) and prints one JSON line: per call its name, whether every proof equalled the oracle's
and the additions; plus what the scenario needs to predict them (the non-zero window digits of the wires a slot stands for, per voter and tree)."""
import ctypes, json, os, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import census, setup
from zkcensus_amd.r1cs import Layout
import oracle_lib as ol

NL = 10
C_SEC, NW_SEC = 12, 22                                  # window bits and windows of a census key's witness sections (zkc_prover.h: MSM_C_SMALL; zkc_pass_plan.h: msm_nw)
K = int(os.environ.get('ZKC_TOP_FOLD', '8'))
_, zp, _ = setup.ensure_test_artifacts(NL)
zk = open(zp, 'rb').read()
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
lib = ctx._lib
L = Layout(NL); n = L.n
nW, nIn = ctx.n_wires(NL), ctx.n_inputs(NL)
BASE = 1 << 20                                          # addresses BASE + i: a voter's path is the low bits of i


def sections(zkey):
    nsec = struct.unpack_from('<I', zkey, 8)[0]
    at, out = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from('<IQ', zkey, at)
        out[typ] = zkey[at + 12:at + 12 + size]
        at += 12 + size
    return out


def live_sections():
    """per wire: in how many of the G1 sections A, B1, C it has a base that is not the point at infinity (C from wire nPub + 1)"""
    sec = sections(zk); npub = 8
    nz = lambda s, cnt: np.frombuffer(s, dtype=np.uint8, count=64 * cnt).reshape(cnt, 64).any(axis=1)
    live = nz(sec[5], nW).astype(int) + nz(sec[6], nW).astype(int)
    live[npub + 1:] += nz(sec[8], nW - npub - 1).astype(int)
    return live


LIVE = live_sections()


def group(tree, g):
    blk = (L.off_census, L.off_sikver)[tree]
    nctrl = (g == n - 3) + (0 < g < n - 2) + 1
    return blk + L.lvl_off(g) + nctrl, blk + (L.lvl_off(g + 1) if g + 1 < n - 1 else L.lvl_off(n - 1))


def nz_digits(x):
    """non-zero signed window digits of a scalar as the bucketing forms them (zkc_msm_sort.hip: d = bits + carry; above half it becomes 2^c - d with a carry)"""
    half, mask, carry, cnt = 1 << (C_SEC - 1), (1 << C_SEC) - 1, 0, 0
    for i in range(NW_SEC):
        d = ((x >> (C_SEC * i)) & mask) + carry
        if d > half:
            d, carry = (1 << C_SEC) - d, 1
        else:
            carry = 0
        cnt += d != 0
    return cnt


def top_adds(w, tree):
    """the G1 additions a proof saves when the groups 0 .. K-1 of `tree` come from a slot"""
    t = 0
    for g in range(K):
        a, e = group(tree, g)
        for i in range(a, e):
            if LIVE[i]:
                t += int(LIVE[i]) * nz_digits(int.from_bytes(w[32 * i:32 * i + 32], 'little'))
    return t


def subtrees(ws, tree):
    """per witness: the first witness that carries the same wires in the groups 0 .. K-1 of `tree` (voters below one depth-K node)"""
    first, ids = {}, []
    for i, w in enumerate(ws):
        key = b''.join(w[32 * a:32 * e] for a, e in (group(tree, g) for g in range(K)))
        ids.append(first.setdefault(key, i))
    return ids


def depths(flat_block):
    """(census, sik): 1 + the index of the voter's last non-zero sibling"""
    out = []
    for tree in range(2):
        d = 0
        for i in range(NL + 1):
            o = 32 * (12 + tree * (NL + 1) + i)
            if any(flat_block[o:o + 32]):
                d = i + 1
        out.append(d)
    return tuple(out)


def make_census(nv, salt=0):
    eid, _, password, signature, avail = census._voter_data(nv + salt, census.ELECTION_ID_HEX)
    password, signature, avail = password[salt:], signature[salt:], avail[salt:]
    address = [BASE + i for i in range(nv)]
    vh = [census.bytes_to_arbo(a.to_bytes((a.bit_length() + 7) // 8 or 1, 'big')) for a in avail]
    flat, cr, sr = census.census_inputs(ctx, eid, address, password, signature, avail, [1] * nv, vh, NL)
    blocks = [flat[32 * nIn * i:32 * nIn * (i + 1)] for i in range(nv)]
    ws, st = ctx.witness(blocks, NL)
    assert st == [0] * nv, st
    return blocks, ws, (cr, sr)


def rs_of(i):
    import hashlib
    h = lambda tag: int.from_bytes(hashlib.sha256(b'%s%d' % (tag, i)).digest(), 'little') % ol.R
    return h(b'r'), h(b's')


_oracle = {}


def oracle(items):
    """items: (witness bytes, rs index) -> (proof, publics) of the CPU oracle, each pair proved once"""
    todo = [it for it in dict.fromkeys(items) if it not in _oracle]
    for it, (rc, p, u) in zip(todo, ol.pmap(lambda a: ol.prove(zk, a[0], *rs_of(a[1])), todo)):
        assert rc == 0
        _oracle[it] = (p, u)
    return [_oracle[it] for it in items]


calls = []


def adds_of(fn):
    lib.zkc_profile_enable(ctx._h, 0x10)
    out = fn()
    ms, cnt, by = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.zkc_profile_read(ctx._h, 7, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by))
    lib.zkc_profile_enable(ctx._h, 0)
    return out, cnt.value


def prove(name, ws, idx, rs_idx=None, inputs=None):
    """one prove_batch_dev call over the witnesses ws[i], i in idx (inputs: the voters' input blocks instead -- fullprove_batch_dev)"""
    rs_idx = list(idx) if rs_idx is None else rs_idx
    rsb = b''.join(ol.le32(x) for k in rs_idx for x in rs_of(k))
    b = len(idx)
    if inputs is None:
        d_w = torch.from_numpy(np.frombuffer(b''.join(ws[i] for i in idx), dtype=np.uint8).copy()).cuda()
        (p, u), adds = adds_of(lambda: pk.prove_batch_dev(d_w.data_ptr(), b, rsb))
    else:
        d_in = torch.from_numpy(np.frombuffer(b''.join(inputs[i] for i in idx), dtype=np.uint8).copy()).cuda()
        d_w = torch.empty(b * nW * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(b, dtype=torch.int32, device='cuda')
        (p, u), adds = adds_of(lambda: pk.fullprove_batch_dev(d_in.data_ptr(), b, d_w.data_ptr(), d_st.data_ptr(), rsb))
        assert int(d_st.abs().sum().item()) == 0
    want = oracle([(ws[i], k) for i, k in zip(idx, rs_idx)])
    equal = all((p[256 * q:256 * q + 256], u[256 * q:256 * q + 256]) == want[q] for q in range(b))
    calls.append({'name': name, 'equal': bool(equal), 'adds': adds, 'proofs': b})


out = {'K': K}
scenario = sys.argv[1]
if scenario == 'census64':
    # 64 voters, all six levels down: 2^K subtrees per tree.  Twice the whole census (misses that seed, then hits), then what never folds its top: a lone proof, a pair, a
    # one-pass call that brings its inputs (laid out early), and a call whose first witness has one word changed inside a top group
    blocks, ws, _ = make_census(64)
    assert all(depths(b) == (6, 6) for b in blocks)
    prove('first', ws, range(64)); prove('second', ws, range(64))
    prove('one', ws, [5]); prove('two', ws, [6, 7]); prove('early', ws, range(8, 16), inputs=blocks)
    a, _ = group(0, 0)
    alt = bytearray(ws[0]); alt[32 * (a + 1) + 12] ^= 1            # the second wire of the census tree's first group (not one the slot index is hashed from), word 3
    ws2 = list(ws) + [bytes(alt)]
    prove('altered', ws2, [64, 1, 2, 3], rs_idx=[0, 1, 2, 3]); prove('unaltered', ws2, [0, 1, 2, 3])
    out['top'] = [[top_adds(w, 0), top_adds(w, 1)] for w in ws2]
    out['subtree'] = [subtrees(ws, 0), subtrees(ws, 1)]
elif scenario == 'mixed65':
    # the prover's own split of 65 proofs, 33 + 32: first the voters of half the subtrees (their slots are seeded), then everyone -- both passes hold hits and misses, the
    # misses seed, and pass 1 may find the slots pass 0 wrote --, then everyone again: all hits
    blocks, ws, _ = make_census(65)
    sub = subtrees(ws, 0)
    assert sub == subtrees(ws, 1) and len(set(sub)) == 1 << K
    half = [i for i in range(65) if sorted(set(sub)).index(sub[i]) < (1 << K) // 2]
    prove('half', ws, half); prove('all', ws, range(65)); prove('again', ws, range(65))
    out['top'] = [[top_adds(w, 0), top_adds(w, 1)] for w in ws]
    out['half'] = half
elif scenario == 'two_roots':
    # two censuses with different roots, alternating on one key: the entries of both stay
    _, wa, ra = make_census(16); _, wb, rb = make_census(16, salt=37)
    assert ra[0] != rb[0] and ra[1] != rb[1]
    for rnd in range(3):
        prove('a%d' % rnd, wa, range(16)); prove('b%d' % rnd, wb, range(16))
    out['top_a'] = [[top_adds(w, 0), top_adds(w, 1)] for w in wa]; out['top_b'] = [[top_adds(w, 0), top_adds(w, 1)] for w in wb]
elif scenario == 'shallow3':
    # three voters; the census tree holds them alone, the sik tree one more entry next to voter 1: voter 1 sits one level down the census tree and five down the sik tree,
    # voters 0 and 2 five down both (they part at bit 4)
    eid, _, password, signature, avail = census._voter_data(3, census.ELECTION_ID_HEX)
    address = [BASE, BASE + 1, BASE + 16]
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    vh = [census.bytes_to_arbo(a.to_bytes((a.bit_length() + 7) // 8 or 1, 'big')) for a in avail]
    with census.CensusTree(ctx, NL) as ct, census.CensusTree(ctx, NL) as stree:
        assert ct.add(address, avail) == [0] * 3 and stree.add(address + [BASE + 17], sik + [12345]) == [0] * 4
        flat, _, _, st = census.census_inputs_from_trees(ctx, ct, stree, eid, address, password, signature, [1] * 3, vh)
    assert st == [0] * 3
    blocks = [flat[32 * nIn * i:32 * nIn * (i + 1)] for i in range(3)]
    ws, wst = ctx.witness(blocks, NL)
    assert wst == [0] * 3
    out['depths'] = [depths(b) for b in blocks]
    prove('first', ws, range(3)); prove('second', ws, range(3))
    out['top'] = [[top_adds(w, 0), top_adds(w, 1)] for w in ws]
else:
    raise SystemExit('unknown scenario')
out['calls'] = calls
print(json.dumps(out))
pk.close(); ctx.close()
