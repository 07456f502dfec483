"""GPU: witnesses checked against a resident constraint system (r1cs.Device, zkc_r1cs_load / zkc_r1cs_check / zkc_r1cs_check_dev; csrc/zkc_r1cs.hip).

Every expected verdict is Python's: r1cs.R1CS.check for the first violated constraint, a count of violated constraints made with lc_eval, and the two wire rules restated
here (wire 0 == 1 before any wire < r before any constraint).  Hand-made systems reach each branch of the kernel (empty rows, constants, a repeated wire, r - 1, rows
around and far above the long-row threshold, sizes around the wave and the block); then the census circuit at nLevels 10 and 160, and a random system of 10^5 constraints."""
import collections, ctypes, json, os, random, re, struct, sys
import pytest
import oracle_lib as ol
from zkcensus_amd import r1cs, _native
from zkcensus_amd.r1cs import R, lc_eval

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
ZKC_ERR_BAD_ARG, ZKC_ERR_FORMAT = 4, 5
LONG = int(re.search(r'R1CS_LONG = (\d+);', open(os.path.join(ol.ROOT, 'zk-franchise-proof-circuit_amd', 'csrc', 'zkc_r1cs.hip')).read()).group(1))
N_IN = 170                                          # input wires of a hand-made system: 1 .. N_IN; wire N_IN is zero


def to_bytes(wit):
    return b''.join(x.to_bytes(32, 'little') for x in wit)


def wires(w):
    return [int.from_bytes(w[32 * i:32 * i + 32], 'little') for i in range(len(w) // 32)]


def violated(cs, wit, rows=None):
    return [k for k in (range(len(cs.cons)) if rows is None else rows) if (lc_eval(cs.cons[k][0], wit) * lc_eval(cs.cons[k][1], wit) - lc_eval(cs.cons[k][2], wit)) % R]


def py_verdict(cs, wit):
    """(first_bad, n_bad) as include/zkcensus_r1cs.h words them, decided by the Python restatement"""
    if wit[0] != 1:
        return r1cs.NOT_ONE, 0
    if any(x >= R for x in wit):
        return r1cs.WIRE_RANGE, 0
    first = cs.check(wit)
    bad = violated(cs, wit)
    assert first == (bad[0] if bad else -1)
    return first, len(bad)


class Repeated(dict):
    """a linear combination that names a wire more than once: R1CS.write and lc_eval both walk items()"""
    def __init__(self, pairs):
        super().__init__(pairs); self.pairs = list(pairs)

    def items(self):
        return self.pairs


def hand_made(n_cons, seed):
    """A satisfiable system of n_cons constraints over N_IN inputs and one output wire per constraint, with its witness.  Row k's C side holds its own output wire
    N_IN + 1 + k (so changing that wire breaks constraint k alone), except for the special rows without one.  Returns (cs, witness, {name: file index of a special row})."""
    rng = random.Random(seed)
    nW = 1 + N_IN + n_cons
    wit = [1] + [rng.randrange(1, R) for _ in range(N_IN - 1)] + [0] + [0] * n_cons
    cs = r1cs.R1CS(nW, 2)
    lc = lambda n: {w: rng.randrange(1, R) for w in rng.sample(range(0, N_IN), n)}
    special = {}
    plan = {}
    if n_cons >= 63:
        names = ['emptyA', 'emptyB', 'emptyC', 'const', 'repeat', 'rm1', 'under', 'at', 'over', 'far']
        for name, k in zip(names, rng.sample(range(1, n_cons - 1), len(names))):
            plan[k] = name; special[name] = k
    for k in range(n_cons):
        out = N_IN + 1 + k
        name = plan.get(k)
        own = True
        if name == 'emptyA':
            a, b, c, own = {}, lc(2), {}, False
        elif name == 'emptyB':
            a, b, c, own = lc(3), {}, {}, False
        elif name == 'emptyC':
            a, b, c, own = {N_IN: 5}, lc(2), {}, False                      # wire N_IN is zero
        elif name == 'const':
            a, b, c, own = {0: 3}, {0: 5}, {0: 15}, False
        elif name == 'repeat':
            x = rng.randrange(1, N_IN)
            a, b = Repeated([(x, 7), (x, R - 3), (x + 1 if x + 1 < N_IN else 1, 2)]), lc(1)
        elif name == 'rm1':
            x, y = rng.sample(range(1, N_IN), 2)
            a, b = {x: R - 1, y: 1}, {0: 1, x: R - 1}
        elif name in ('under', 'at', 'over', 'far'):
            total = {'under': LONG - 1, 'at': LONG, 'over': LONG + 1, 'far': 2 * 64 + 1 + 30}[name]
            nc = 9                                                          # C: the output wire and eight inputs
            na = (total - nc) * 2 // 3; nb = total - nc - na
            a, b = lc(na), lc(nb)
        else:
            a, b = lc(1 + rng.randrange(3)), lc(1 + rng.randrange(2))
        if own:
            rest = lc(8) if name in ('under', 'at', 'over', 'far') else ({} if rng.random() < 0.7 else lc(1))
            coef = rng.choice([1, R - 1, rng.randrange(1, R)])
            wit[out] = (lc_eval(a, wit) * lc_eval(b, wit) - lc_eval(rest, wit)) * pow(coef, -1, R) % R
            c = dict(rest); c[out] = coef
        cs.add(a, b, c)
        if name in ('under', 'at', 'over', 'far'):
            assert len(a) + len(b) + len(c) == total
    assert cs.check(wit) == -1
    return cs, wit, special


def image(cs, tmp_path, name='cs'):
    p = str(tmp_path / (name + '.r1cs'))
    cs.write(p)
    return open(p, 'rb').read()


def expect(dev, cs, wits):
    got = dev.check(b''.join(to_bytes(w) for w in wits))
    want = [py_verdict(cs, w) for w in wits]
    assert list(zip(*got)) == want
    return want


@pytest.fixture(scope='module')
def ctx():
    import zkcensus_amd
    c = zkcensus_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('n_cons', [1, 63, 64, 65, 255, 256, 257])
def test_hand_made_systems(ctx, tmp_path, n_cons):
    cs, wit, special = hand_made(n_cons, 1000 + n_cons)
    out = lambda k: N_IN + 1 + k
    bump = lambda w, k: w[:k] + [(w[k] + 1) % R] + w[k + 1:]
    with r1cs.Device(ctx, image(cs, tmp_path)) as dev:
        assert dev.info == (cs.nWires, 2, n_cons)
        assert expect(dev, cs, [wit]) == [(-1, 0)]                                          # B = 1
        first, last = bump(wit, out(0)), bump(wit, out(n_cons - 1))
        assert expect(dev, cs, [wit, first, last]) == [(-1, 0), (0, 1), (n_cons - 1, 1)]   # B = 3
        if special:
            far = special['far']
            assert expect(dev, cs, [bump(wit, out(far)), wit, bump(wit, out(special['at']))]) == [(far, 1), (-1, 0), (special['at'], 1)]
            # two violations that the device's order (longest row first) holds in different waves and the other way round: a short row earlier in the file than the
            # long one.  The verdict is the file's.
            short = max(k for k in range(far) if k not in special.values())
            assert expect(dev, cs, [bump(bump(wit, out(short)), out(far))]) == [(short, 2)]
        # seeded random mutations of any wire, the inputs (which break many rows at once) and wire 0 included
        rng = random.Random(n_cons)
        muts = []
        for _ in range(50):
            m = list(wit); m[rng.randrange(0, cs.nWires) if rng.random() < 0.5 else rng.randrange(0, N_IN + 1)] = rng.randrange(R)
            muts.append(m)
        want = expect(dev, cs, muts)
        assert n_cons == 1 or len({f for f, _ in want}) > 5


def test_verdict_codes(ctx, tmp_path):
    cs, wit, special = hand_made(65, 7)
    j = next(i for i in range(65) if i not in special.values())
    k = N_IN + 1 + j                                 # constraint j's own output wire
    sub = lambda pairs: [dict(pairs).get(i, x) for i, x in enumerate(wit)]
    cases = [sub([(k, R)]), sub([(k, 2 ** 256 - 1)]), sub([(5, R + 1)]), sub([(cs.nWires - 1, R)]), sub([(0, 2)]), sub([(0, 0)]), sub([(0, 2), (k, R)]),
             sub([(0, 2 ** 256 - 1)]), sub([(0, R + 1)]), sub([(k, R - 1)]), wit]
    with r1cs.Device(ctx, image(cs, tmp_path)) as dev:
        want = expect(dev, cs, cases)
    assert want == [(-2, 0)] * 4 + [(-3, 0)] * 5 + [(j, 1), (-1, 0)]


@pytest.fixture(scope='module')
def census10(ctx, tmp_path_factory):
    from census_gen import random_voter
    L, cs = r1cs.build(10)
    p = str(tmp_path_factory.mktemp('c10') / 'census10.r1cs')
    cs.write(p)
    rng = random.Random(10)
    voters = [random_voter(rng, ol.poseidon, nLevels=10, depth_c=rng.randrange(1, 11), depth_s=rng.randrange(1, 11)) for _ in range(5)]
    ws, st = ctx.witness(voters, nLevels=10)
    assert st == [0] * 5
    return L, cs, p, ws


def touch_index(cs):
    touch = collections.defaultdict(list)
    for idx, (a, b, c) in enumerate(cs.cons):
        for w in set(a) | set(b) | set(c):
            touch[w].append(idx)
    return touch


def test_census_circuit_nlevels_10(ctx, census10):
    import numpy as np, torch
    L, cs, path, ws = census10
    assert L.nWires == 8354
    with r1cs.Device(ctx, path) as dev:
        assert dev.info == (8354, 8, len(cs.cons)) == r1cs.header_info(path)
        assert dev.check(b''.join(ws)) == ([-1] * 5, [0] * 5)
        d = torch.from_numpy(np.frombuffer(b''.join(ws), dtype=np.uint8).copy()).cuda()
        assert dev.check_dev(d, 5) == ([-1] * 5, [0] * 5)
        assert dev.check_dev(d.data_ptr() + 32 * 8354 * 3, 2) == ([-1] * 2, [0] * 2)
        base = [wires(w) for w in ws]
        for w in base:
            assert cs.check(w) == -1
        # the base witnesses satisfy every constraint, so a changed wire can only break constraints that name it (tests/test_r1cs_setup_cpu.py indexes them the same way)
        touch = touch_index(cs)
        rng = random.Random(40)
        muts, want = [], []
        for i in range(40):
            k = rng.randrange(1, L.nWires) if i >= 4 else (4, 5, L.off_checknull, L.off_census + 2)[i]      # four of the wires no constraint pins
            m = list(base[i % 5]); m[k] = (m[k] + 1 + rng.randrange(5)) % R
            bad = violated(cs, m, touch[k])
            muts.append(to_bytes(m)); want.append((bad[0] if bad else -1, len(bad)))
        assert want[:4] == [(-1, 0)] * 4 and sum(1 for f, _ in want if f >= 0) >= 30
        got = dev.check(b''.join(muts))
        assert list(zip(*got)) == want
        dm = torch.from_numpy(np.frombuffer(b''.join(muts), dtype=np.uint8).copy()).cuda()
        assert list(zip(*dev.check_dev(dm, 40))) == want
        ms = dev.stats()
        assert len(ms) == 3 and ms[2] > 0


def test_census_circuit_nlevels_160(ctx, tmp_path):
    L, cs = r1cs.build(160)
    vec = ol.load_json('witness_vectors.json')['vectors']
    ws, st = ctx.witness([vec[0]['inputs'], vec[1]['inputs']], nLevels=160)
    assert st == [0, 0]
    with r1cs.Device(ctx, image(cs, tmp_path, 'census160')) as dev:
        assert dev.info == (82754, 8, len(cs.cons))
        assert dev.check(b''.join(ws)) == ([-1, -1], [0, 0])
        base = wires(ws[1])
        touch = touch_index(cs)
        rng = random.Random(160)
        muts, want = [], []
        for k in rng.sample(range(1, L.nWires), 10):
            m = list(base); m[k] = (m[k] + 1 + rng.randrange(5)) % R
            bad = violated(cs, m, touch[k])
            muts.append(to_bytes(m)); want.append((bad[0] if bad else -1, len(bad)))
        assert list(zip(*dev.check(b''.join(muts)))) == want and any(f >= 0 for f, _ in want)


def parse_r1cs(img):
    """an .r1cs image -> r1cs.R1CS, in Python (tests/big_circuit.py writes its files directly)"""
    secs, p = {}, 12
    for _ in range(struct.unpack_from('<I', img, 8)[0]):
        sid, sz = struct.unpack_from('<IQ', img, p); secs[sid] = (p + 12, sz); p += 12 + sz
    h = secs[1][0]
    nW, nOut, nIn = struct.unpack_from('<III', img, h + 36); nC = struct.unpack_from('<I', img, h + 60)[0]
    cs = r1cs.R1CS(nW, nOut + nIn); q = secs[2][0]
    for _ in range(nC):
        row = []
        for _m in range(3):
            n = struct.unpack_from('<I', img, q)[0]; q += 4; a = {}
            for _t in range(n):
                w = struct.unpack_from('<I', img, q)[0]; a[w] = (a.get(w, 0) + int.from_bytes(img[q + 4:q + 36], 'little')) % R; q += 36
            row.append(a)
        cs.add(*row)
    return cs


def test_random_system_and_its_proofs(ctx, tmp_path):
    import big_circuit as bc
    import zkcensus_amd
    n_cons, n_wires, n_pub = 100000, 3000, 2                       # the smallest size big_circuit is written for (10^5 rows); few wires keep the key cheap
    r1 = str(tmp_path / 'big.r1cs')
    w = bc.big_instance(r1, n_cons, n_wires, n_pub, seed=99)
    img = open(r1, 'rb').read()
    cs = parse_r1cs(img)
    lib = _native.load()
    z, v = str(tmp_path / 'big.zkey'), str(tmp_path / 'big_vkey.json')
    err = ctypes.create_string_buffer(512)
    assert lib.zkc_setup_from_r1cs_dev(ctx._h, r1.encode(), 4711, z.encode(), v.encode(), err, 512) == 0, err.value
    vk = json.load(open(v))
    pk = zkcensus_amd.ProvingKey(ctx, open(z, 'rb').read())
    with r1cs.Device(ctx, img) as dev:
        assert dev.info == (n_wires, n_pub, n_cons)
        assert dev.check(w) == ([-1], [0]) and cs.check(wires(w)) == -1
        proof, pub = pk.prove(w, 3, 5)
        assert ol.verify(vk, pub, proof)
        m = wires(w); k = 1234; m[k] = (m[k] + 1) % R
        want = py_verdict(cs, m)
        assert list(zip(*dev.check(to_bytes(m)))) == [want]
        assert want[0] >= 0                                          # wire 1234 is in some row of the 10^5
        proof2, pub2 = pk.prove(to_bytes(m), 3, 5)
        assert not ol.verify(vk, pub2, proof2)
    pk.close()


def test_argument_errors_and_lifetime(ctx, census10, tmp_path):
    import zkcensus_amd
    from zkcensus_amd import setup
    L, cs10, path10, ws = census10
    lib = _native.load()
    small, wit, _ = hand_made(65, 3)
    a = r1cs.Device(ctx, image(small, tmp_path, 'small'))
    b = r1cs.Device(ctx, path10)
    first, count = (ctypes.c_int64 * 1)(77), (ctypes.c_uint32 * 1)(88)
    for n in (L.nWires - 1, L.nWires + 1):
        assert lib.zkc_r1cs_check(b._h, ws[0], n, 1, first, count) == ZKC_ERR_BAD_ARG and (first[0], count[0]) == (77, 88)
    assert 'wires' in lib.zkc_last_error(ctx._h).decode()
    assert lib.zkc_r1cs_check(b._h, ws[0], L.nWires, 0, first, count) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check(b._h, None, L.nWires, 1, first, count) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check(b._h, ws[0], L.nWires, 1, None, count) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check_dev(b._h, None, L.nWires, 1, first, count) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check(b._h, ws[0], L.nWires, 1, first, None) == 0 and first[0] == -1          # n_bad may be NULL
    with pytest.raises(ValueError):
        b.check(ws[0][:-32])
    # a malformed image is the reader's text, through the context
    img = open(path10, 'rb').read()
    h = ctypes.c_void_p()
    assert lib.zkc_r1cs_load(ctx._h, img[:len(img) // 2], len(img) // 2, ctypes.byref(h)) == ZKC_ERR_FORMAT and not h.value
    assert lib.zkc_last_error(ctx._h).decode() == 'r1cs constraints truncated'
    with pytest.raises(zkcensus_amd.ZkcError, match='not an r1cs file'):
        r1cs.Device(ctx, b'zkey' + img[4:])
    # two systems resident; one is freed, the other still answers
    assert a.check(to_bytes(wit)) == ([-1], [0]) and b.check(ws[1]) == ([-1], [0])
    a.close(); a.close()
    assert b.check(ws[2]) == ([-1], [0])
    # a check between two proofs with a key resident on the same context changes nothing in the proof
    _, zkey_path, _ = setup.ensure_test_artifacts(10)
    pk = zkcensus_amd.ProvingKey(ctx, open(zkey_path, 'rb').read())
    before = pk.prove(ws[0], 12345, 67890)
    m = wires(ws[0]); m[L.off_nullifier + 7] = (m[L.off_nullifier + 7] + 1) % R
    f, c = b.check(ws[0] + to_bytes(m))
    assert f[0] == -1 and f[1] >= 0 and c[1] >= 1
    assert pk.prove(ws[0], 12345, 67890) == before
    pk.close(); b.close()


def test_wtns_check_convenience(ctx, census10):
    from zkcensus_amd import groth16
    L, cs, path, ws = census10
    lib = _native.load()
    def wtns_file(payload):
        n = len(payload) // 32
        need = lib.zkc_wtns_write(payload, n, None, 0)
        out = ctypes.create_string_buffer(need)
        lib.zkc_wtns_write(payload, n, out, need)
        return out.raw
    assert groth16.wtns_check(ctx, path, wtns_file(ws[0])) is True
    m = wires(ws[0]); m[3] = (m[3] + 1) % R                          # the nullifier: a public wire pinned by the t = 5 Poseidon
    assert cs.check(m) >= 0 and groth16.wtns_check(ctx, open(path, 'rb').read(), wtns_file(to_bytes(m))) is False
    with pytest.raises(ValueError):
        groth16.wtns_check(ctx, path, wtns_file(ws[0][:-32]))
