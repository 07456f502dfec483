"""Helper of tests/test_gpu_c_rows.py.  It runs as a child process, because ZKC_C_ROWS is read when a key is loaded and every other test keeps the default.  argv[1] names
a scenario, argv[2] a file in which the CPU oracle's proofs are kept from one child to the next (they do not depend on the switch).  Each scenario proves nLevels-10 voters
through the public prove calls with fixed (r, s) and prints one JSON line.
  calls  3, 33 and 65 voters of one census, 5 voters at different depths of another, 4 voters with a foreign witness among them: per call whether every proof and
         public-signal block equalled the oracle's, a digest of the proof bytes, the G1 additions the device counted (zkc_profile_read, category 7), how many passes left out
         C's transform pair and how many vectors went through the pair (zkc_debug_c_rows), and -- argv[3] = digits -- the non-zero signed window digits of C_dom - C_T
         over the call's voters, computed here from zkc_debug_stage's domain vectors and the template's (delta_c_stats)
  slots  a 33-voter call and a 2-voter call kept in flight together on call slots 0 and 1, three times: the bytes of each against the bytes it gives alone
  bases  -H'_j at rows 0, 1, the last constraint row and n - 1 against the H section's MSM over -pair(e_j), the pair by the oracle's transform"""
import ctypes, hashlib, json, os, pickle, struct, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import zkcensus_amd
from zkcensus_amd import census, setup
import oracle_lib as ol

NL = 10
C_H, NW_H = 17, 15                                      # window bits and windows of a census key's H section (zkc_prover.h: MSM_C_BIG; zkc_pass_plan.h: msm_nw)
R = ol.R
RINV = pow(1 << 256, -1, R)
_, zp, _ = setup.ensure_test_artifacts(NL)
zk = open(zp, 'rb').read()
ctx = zkcensus_amd.Context(0); pk = zkcensus_amd.ProvingKey(ctx, zk)
lib = ctx._lib
nW, nIn, n = ctx.n_wires(NL), ctx.n_inputs(NL), pk.domain_size
BASE = 1 << 20
CACHE = sys.argv[2] if len(sys.argv) > 2 else None
_oracle = pickle.load(open(CACHE, 'rb')) if CACHE and os.path.exists(CACHE) else {}


def dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def rs_of(i):
    h = lambda tag: int.from_bytes(hashlib.sha256(b'%s%d' % (tag, i)).digest(), 'little') % R
    return h(b'r'), h(b's')


def oracle(items):
    """items: (witness bytes, rs index) -> (proof, publics) of the CPU oracle, each pair proved once (and kept in the cache file)"""
    key = lambda it: hashlib.sha256(it[0]).hexdigest() + ':%d' % it[1]
    todo = [it for it in dict.fromkeys(items) if key(it) not in _oracle]
    for it, (rc, p, u) in zip(todo, ol.pmap(lambda a: ol.prove(zk, a[0], *rs_of(a[1])), todo)):
        assert rc == 0
        _oracle[key(it)] = (p, u)
    if todo and CACHE:
        pickle.dump(_oracle, open(CACHE + '.tmp%d' % os.getpid(), 'wb')); os.replace(CACHE + '.tmp%d' % os.getpid(), CACHE)
    return [_oracle[key(it)] for it in items]


def census_of(nv):
    eid, _, password, signature, avail = census._voter_data(nv, census.ELECTION_ID_HEX)
    address = [BASE + i for i in range(nv)]
    vh = [census.bytes_to_arbo(a.to_bytes((a.bit_length() + 7) // 8 or 1, 'big')) for a in avail]
    flat, _, _ = census.census_inputs(ctx, eid, address, password, signature, avail, [1] * nv, vh, NL)
    ws, st = ctx.witness([flat[32 * nIn * i:32 * nIn * (i + 1)] for i in range(nv)], NL)
    assert st == [0] * nv, st
    return ws


def uneven5():
    """five voters of one census: BASE + 0 and + 16 part at bit 4 (five levels down), + 2 leaves them at bit 1, + 1 and + 3 part at bit 1 (two levels down)"""
    eid, _, password, signature, avail = census._voter_data(5, census.ELECTION_ID_HEX)
    address = [BASE, BASE + 1, BASE + 16, BASE + 2, BASE + 3]
    sik = census.poseidon_batch(ctx, list(zip(address, password, signature)))
    vh = [census.bytes_to_arbo(a.to_bytes((a.bit_length() + 7) // 8 or 1, 'big')) for a in avail]
    with census.CensusTree(ctx, NL) as ct, census.CensusTree(ctx, NL) as stree:
        assert ct.add(address, avail) == [0] * 5 and stree.add(address, sik) == [0] * 5
        flat, _, _, st = census.census_inputs_from_trees(ctx, ct, stree, eid, address, password, signature, [1] * 5, vh)
    assert st == [0] * 5
    blocks = [flat[32 * nIn * i:32 * nIn * (i + 1)] for i in range(5)]
    depth = lambda b, tree: max([i + 1 for i in range(NL + 1) if any(b[32 * (12 + tree * (NL + 1) + i):32 * (12 + tree * (NL + 1) + i) + 32])] or [0])
    ws, wst = ctx.witness(blocks, NL)
    assert wst == [0] * 5
    return ws, [(depth(b, 0), depth(b, 1)) for b in blocks]


def info():
    out = ctypes.create_string_buffer(32)
    ctx._check(lib.zkc_debug_c_rows(pk._h, 2, 0, 0, out))
    return struct.unpack('<4Q', out.raw)


def adds_of(fn):
    lib.zkc_profile_enable(ctx._h, 0x10)
    out = fn()
    ms, cnt, by = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    lib.zkc_profile_read(ctx._h, 7, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by))
    lib.zkc_profile_enable(ctx._h, 0)
    return out, cnt.value


def nz_digits(scalars):
    """non-zero signed window digits of H scalars (32 B each, standard form) as the bucketing forms them (zkc_msm_sort.hip: d = bits + carry; above half it becomes
    2^c - d with a carry), summed over the scalars"""
    a = np.frombuffer(bytes(scalars), dtype='<u8').reshape(-1, 4)
    half, mask = np.uint64(1 << (C_H - 1)), np.uint64((1 << C_H) - 1)
    carry, cnt = np.zeros(len(a), dtype=np.uint64), 0
    for i in range(NW_H):
        li, sh = (C_H * i) >> 6, (C_H * i) & 63
        d = a[:, li] >> np.uint64(sh)
        if sh + C_H > 64 and li < 3:
            d = d | (a[:, li + 1] << np.uint64(64 - sh))
        d = (d & mask) + carry
        neg = d > half
        d = np.where(neg, np.uint64(1 << C_H) - d, d)
        carry = neg.astype(np.uint64)
        cnt += int(np.count_nonzero(d))
    return cnt


_tmpl_c, _stats = None, {}


def delta_c_stats(w):
    """of one witness: rows with C_dom != C_T; the non-zero digits of those differences; and by how many non-zero digits the proof's n evaluations change when the template's
    transformed C stands in for its own -- h' = h + pair(C_dom - C_T) against h, the pair by the oracle's transform.  (Either is n full-width values of 15 digits, each zero
    with probability 2^-17: a handful per proof, and not the same handful.)"""
    global _tmpl_c
    if w in _stats:
        return _stats[w]
    if _tmpl_c is None:
        out = ctypes.create_string_buffer(96 * n)
        ctx._check(lib.zkc_debug_c_rows(pk._h, 1, 0, 0, out))
        _tmpl_c = out.raw[64 * n:]
    d_w = dev(w)
    c = pk.debug_stage(d_w.data_ptr(), 0)[64 * n:]
    h = pk.debug_stage(d_w.data_ptr(), 1)
    val = lambda b, i: int.from_bytes(b[32 * i:32 * i + 32], 'little')
    dc = [0] * n
    rows = [i for i in range(n) if c[32 * i:32 * i + 32] != _tmpl_c[32 * i:32 * i + 32]]
    for i in rows:
        dc[i] = (val(c, i) - val(_tmpl_c, i)) * RINV % R
    g, f, sc = ol.root_of_unity(n.bit_length()), 1, []
    for x in ol.ntt(dc, inverse=True):
        sc.append(x * f % R); f = f * g % R
    h_new = b''.join(ol.le32((val(h, i) + x) % R) for i, x in enumerate(ol.ntt(sc)))
    _stats[w] = (len(rows), nz_digits(b''.join(ol.le32(x) for x in dc)), nz_digits(h_new) - nz_digits(h))
    return _stats[w]


def prove(name, ws, idx, digits=True):
    idx = list(idx); b = len(idx)
    rsb = b''.join(ol.le32(x) for k in idx for x in rs_of(k))
    d_w = dev(b''.join(ws[i] for i in idx))
    before = info()
    (p, u), adds = adds_of(lambda: pk.prove_batch_dev(d_w.data_ptr(), b, rsb))
    after = info()
    want = oracle([(ws[i], k) for i, k in zip(idx, idx)])
    equal = all((p[256 * q:256 * q + 256], u[256 * q:256 * q + 256]) == want[q] for q in range(b))
    dd = [delta_c_stats(ws[i]) for i in idx] if digits else []
    return {'name': name, 'equal': bool(equal), 'sha': hashlib.sha256(p).hexdigest(), 'adds': adds, 'proofs': b, 'vectors': after[0] - before[0], 'new': after[1] - before[1],
            'old': after[2] - before[2], 'rows': sum(r for r, _, _ in dd), 'digits': sum(d for _, d, _ in dd), 'h_digits': sum(e for _, _, e in dd)}


out = {}
scenario = sys.argv[1]
if scenario == 'calls':
    ws = census_of(65)
    w5, out['depths5'] = uneven5()
    want_digits = len(sys.argv) > 3 and sys.argv[3] == 'digits'
    calls = [prove('three', ws, range(3), want_digits), prove('thirtythree', ws, range(33), want_digits), prove('sixtyfive', ws, range(65), want_digits),
             prove('uneven', w5, range(5), want_digits)]
    import random
    rng = random.Random(99)
    junk = b''.join([(1).to_bytes(32, 'little')] + [rng.randrange(R).to_bytes(32, 'little') for _ in range(nW - 1)])
    calls.append(prove('foreign', list(ws[:3]) + [junk], range(4), False))
    out['calls'] = calls
elif scenario == 'slots':
    ws = census_of(33)
    big, small = list(range(33)), [3, 4]
    rsb = lambda idx: b''.join(ol.le32(x) for k in idx for x in rs_of(k))
    d_big, d_small = dev(b''.join(ws[i] for i in big)), dev(b''.join(ws[i] for i in small))
    before = info()
    alone = [pk.prove_batch_dev(d_big.data_ptr(), 33, rsb(big)), pk.prove_batch_dev(d_small.data_ptr(), 2, rsb(small))]
    mid = info()
    same = []
    for rnd in range(3):
        first, second = (0, 1) if rnd % 2 == 0 else (1, 0)             # which call is begun first alternates
        order = [(first, (d_big, 33, big) if first == 0 else (d_small, 2, small)), (second, (d_big, 33, big) if second == 0 else (d_small, 2, small))]
        for slot, (d, b, idx) in order:
            pk.batch_begin(slot, None, b, d.data_ptr(), None, rsb(idx))
        got = {slot: pk.batch_finish(slot, b) for slot, (d, b, idx) in order}
        same.append(got[0] == alone[0] and got[1] == alone[1])
    want = oracle([(ws[i], i) for i in big + small])
    out.update(same=same, new_alone=mid[1] - before[1], new_together=info()[1] - mid[1],
               equal=all((alone[0][0][256 * q:256 * q + 256], alone[0][1][256 * q:256 * q + 256]) == want[q] for q in range(33)) and
               all((alone[1][0][256 * q:256 * q + 256], alone[1][1][256 * q:256 * q + 256]) == want[33 + q] for q in range(2)))
elif scenario == 'bases':
    # the constraints of the key: the highest row that section 4 names (m, c, s, value: 44 B per coefficient)
    at, sec4 = 12, None
    for _ in range(struct.unpack_from('<I', zk, 8)[0]):
        typ, size = struct.unpack_from('<IQ', zk, at)
        if typ == 4:
            sec4 = zk[at + 12:at + 12 + size]
        at += 12 + size
    ncoef = struct.unpack_from('<I', sec4, 0)[0]
    last_row = int(np.frombuffer(sec4, dtype=np.uint8, count=44 * ncoef, offset=4).reshape(ncoef, 44)[:, 4:8].copy().view('<u4').max())
    logn = n.bit_length() - 1
    g = ol.root_of_unity(logn + 1)
    rows, same = [0, 1, last_row, n - 1], []
    for j in rows:
        e = [0] * n; e[j] = 1
        t = ol.ntt(e, inverse=True)
        f, sc = 1, []
        for x in t:
            sc.append(x * f % R); f = f * g % R
        pair = ol.ntt(sc)
        want = pk.msm_debug(4, dev(b''.join(ol.le32((R - x) % R) for x in pair)).data_ptr(), n)          # sum_i -pair(e_j)_i H_i = -H'_j
        got = ctypes.create_string_buffer(64)
        ctx._check(lib.zkc_debug_c_rows(pk._h, 0, j, 1, got))
        same.append(got.raw == want)
    out.update(rows=rows, same=same, n=n, last_row=last_row, ready=info()[3])
else:
    raise SystemExit('unknown scenario')
print(json.dumps(out))
pk.close(); ctx.close()
