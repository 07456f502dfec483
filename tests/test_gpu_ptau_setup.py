"""GPU: Groth16 keys from a prepared powers-of-tau file on the device (include/zkcensus_ptau.h, csrc/zkc_setup_ptau.hip).  The host-thread path of the same entry point is
held against the seeded generator and against every exponent in tests/test_ptau_setup_cpu.py; here the device path must write the host path's bytes -- on the nLevels-10
census circuit and on a crafted circuit whose wire rows sit at, one below and one above every boundary of the kernels (SEG = 32 terms per accumulation lane, RED = 32
partial sums per reduction lane, so 32 x 32 = 1024 terms is where a row starts to need a second reduction step), with every kind of coefficient, under waste that makes
the additions meet equal points, opposite points and infinity.  Then the key is used: a proof under it equals the closed form at (tau, alpha, beta, 1, 1) and verifies,
and a ceremony on top of it passes `zkey verify` against the circuit and fails it for a forged C point and for another circuit.  The .ptau files are made on the GPU by
tests/ptau_lib.py from known waste."""
import json, os, random, struct, sys
import pytest
import oracle_lib as ol
import closed_form as cf
import ptau_lib as pl

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
R, Q = ol.R, ol.Q
NL = 10
TAU, ALPHA, BETA = 0x3c6ef372fe94f82ba54ff53a5f1d36f1510e527fade682d19b05688c2b3e6c1f % R, 0x1f83d9abfb41bd6b5be0cd19137e2179cbbb9d5dc1059ed8629a292a367cd507 % R, 0x9159015a3070dd17152fecd8f70e593967332667ffc00b318eb44a8768581511 % R
SEG, RED = 32, 32
SEED = bytes(range(32))


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    import zkcensus_amd
    from zkcensus_amd import setup
    ctx = zkcensus_amd.Context(0)
    d = tmp_path_factory.mktemp('ptau')
    r1, _, _ = setup.ensure_test_artifacts(NL)
    n_wires, n_pub, cons = cf.read_r1cs(r1)
    power = (len(cons) + n_pub).bit_length()
    assert (1 << power) >= len(cons) + n_pub + 1 > (1 << (power - 1))
    ptau = pl.write(str(d / 'census.ptau'), power, TAU, ALPHA, BETA, ctx=ctx)
    dz, dv = str(d / 'dev.zkey'), str(d / 'dev.json')
    setup.from_ptau(r1, ptau, dz, dv, ctx=ctx)
    dev_ms = setup.ptau_stats()
    yield {'ctx': ctx, 'dir': d, 'r1cs': r1, 'ptau': ptau, 'power': power, 'zkey': dz, 'vkey': dv, 'dev_ms': dev_ms, 'circuit': (n_wires, n_pub, cons)}
    ctx.close()


def same_files(hz, hv, dz, dv):
    a, b = pl.zkey_sections(open(hz, 'rb').read()), pl.zkey_sections(open(dz, 'rb').read())
    for s in range(1, 11):
        assert a[s] == b[s], 'section %d of the device key differs from the host key' % s
    assert open(hz, 'rb').read() == open(dz, 'rb').read() and open(hv, 'rb').read() == open(dv, 'rb').read()


def test_device_key_equals_host_key_census(env):
    from zkcensus_amd import setup
    hz, hv = str(env['dir'] / 'host.zkey'), str(env['dir'] / 'host.json')
    setup.from_ptau(env['r1cs'], env['ptau'], hz, hv)
    same_files(hz, hv, env['zkey'], env['vkey'])
    assert all(v > 0 for v in env['dev_ms'].values()), env['dev_ms']
    s = pl.zkey_sections(open(hz, 'rb').read())
    assert s[2][84:84 + 64] == pl.g1_mont(ALPHA) and s[2][84 + 64 + 64:84 + 256] == pl.g2_mont(BETA) and s[2][84 + 384:84 + 448] == pl.g1_mont(1)


# ---- the crafted circuit ----
LENS = [0, 1, SEG - 1, SEG, SEG + 1, SEG * RED - 1, SEG * RED, SEG * RED + 1]
FULL = 0x2a9e3c1f7b5d08e64c3a1f9d7e5b2c0a8f6e4d2b1a0918273645546372819aaf % R


def crafted():
    """wire 1 + j occurs in the A side and the B side of the first LENS[j] constraints, so its A, B1 and B2 rows have LENS[j] terms (wire 1: none -- every point of it is
    infinity) and its K row the sum; coefficients cycle through 1, r - 1, 2, r - 2, 2^253, a full-width value that repeats within the row, and random full-width ones.
    Wire 9 is squared with coefficient 1, and with FULL, in constraints of its own (alpha = +-beta: P + P and P - P in K), C empty there."""
    rng = random.Random(11)
    kinds = [1, R - 1, 2, R - 2, 1 << 253, FULL, None, (R - 1) // 2, (R + 1) // 2]
    n_cons = max(LENS)
    cons = []
    for c in range(n_cons):
        a, b = [], []
        for j, ln in enumerate(LENS):
            if c < ln:
                k = kinds[(c + 3 * j) % len(kinds)]
                a.append((1 + j, rng.randrange(2, R) if k is None else k))
                k = kinds[(c + 5 * j + 2) % len(kinds)]
                b.append((1 + j, rng.randrange(2, R) if k is None else k))
        cons.append((a, b, [(10 + c % 3, 1 if c % 2 else R - 1)] if c % 5 else []))
    cons += [([(9, 1)], [(9, 1)], []), ([(9, FULL)], [(9, FULL)], [])]
    return 13, 0, cons                                                           # wires 0 .. 12, none public; 1027 constraints + 1: domain 2^11


WASTES = {'plain': (TAU, ALPHA, BETA), 'alpha=beta': (TAU, ALPHA, ALPHA), 'alpha=-beta': (TAU, R - BETA, BETA), 'tau=root': (pow(pl.root_of_unity(11), 1000, R), ALPHA, BETA)}


@pytest.fixture(scope='module')
def crafted_r1cs(env):
    n_wires, n_pub, cons = crafted()
    assert 1024 < len(cons) + n_pub + 1 <= 2048
    return pl.write_r1cs(str(env['dir'] / 'crafted.r1cs'), n_wires, n_pub, cons), (n_wires, n_pub, cons)


@pytest.mark.parametrize('waste', list(WASTES))
def test_device_key_equals_host_key_at_every_boundary(env, crafted_r1cs, waste):
    from zkcensus_amd import setup
    r1, (n_wires, n_pub, cons) = crafted_r1cs
    tau, alpha, beta = WASTES[waste]
    d = env['dir']
    ptau = pl.write(str(d / ('c_%d.ptau' % list(WASTES).index(waste))), 11, tau, alpha, beta, ctx=env['ctx'])
    hz, hv, dz, dv = [str(d / ('c_' + x)) for x in ('h.zkey', 'h.json', 'd.zkey', 'd.json')]
    setup.from_ptau(r1, ptau, hz, hv)
    setup.from_ptau(r1, ptau, dz, dv, ctx=env['ctx'])
    same_files(hz, hv, dz, dv)
    s = pl.zkey_sections(open(dz, 'rb').read())
    a = lambda w: s[5][64 * w:64 * w + 64]
    k = lambda w: s[8][64 * (w - n_pub - 1):64 * (w - n_pub)]
    assert a(1) == bytes(64) and k(1) == bytes(64) and s[6][64:128] == bytes(64) and s[7][128:256] == bytes(128)      # wire 1: in no constraint, four empty rows
    if waste != 'tau=root':
        assert all(any(a(w)) for w in range(2, 10))
    # three rows in the exponent, one at each side of the second reduction step, and the squared wire
    logn, A, B, K, H = pl.key_exponents(n_wires, n_pub, cons, tau, alpha, beta)
    for w in (6, 7, 8, 9):
        assert a(w) == pl.g1_mont(A[w]) and k(w) == pl.g1_mont(K[w]) and s[7][128 * w:128 * w + 128] == pl.g2_mont(B[w]), w
    if waste == 'alpha=-beta':
        assert K[9] == 0 and k(9) == bytes(64)
    if waste == 'tau=root':
        assert s[9] == bytes(64 << 11)


def test_bad_points_are_refused_on_the_device(env):
    from zkcensus_amd import setup, _native
    d = env['dir']; n = 1 << env['power']
    raw = bytearray(open(env['ptau'], 'rb').read())
    off, p = {}, 12
    for _ in range(struct.unpack_from('<I', raw, 8)[0]):
        i, sz = struct.unpack_from('<IQ', raw, p); off[i] = p + 12; p += 12 + sz
    cases = []
    m = bytearray(raw); m[off[12] + 64 * (n - 1 + 77)] ^= 1; cases.append((m, 'section 12 point %d has a coordinate >= q or is not on the curve' % (n - 1 + 77)))
    m = bytearray(raw); at = off[13] + 128 * (n - 1 + 5) + 96; m[at:at + 32] = Q.to_bytes(32, 'little'); cases.append((m, 'section 13 point %d has a coordinate >= q or is not on the twist' % (n - 1 + 5)))
    m = bytearray(raw); m[off[12] + 64 * (2 * n - 1 + 2 * 9 + 1) + 3] ^= 4; m[off[12] + 64 * (n - 1 + 100)] ^= 1          # two bad points: the smaller index is named
    cases.append((m, 'section 12 point %d has' % (n - 1 + 100)))
    for j, (img, text) in enumerate(cases):
        bad = str(d / ('bad%d.ptau' % j)); open(bad, 'wb').write(img)
        out = d / ('bad%d.zkey' % j)
        with pytest.raises(_native.ZkcError) as ei:
            setup.from_ptau(env['r1cs'], bad, out, d / ('bad%d.json' % j), ctx=env['ctx'])
        assert ei.value.code == 5 and text in str(ei.value), str(ei.value)
        assert not out.exists() and not (d / ('bad%d.json' % j)).exists()


def test_proof_under_the_ptau_key_is_the_closed_form_and_verifies(env, monkeypatch):
    import zkcensus_amd
    from zkcensus_amd import groth16
    from census_gen import random_voter
    ctx = env['ctx']
    zk = open(env['zkey'], 'rb').read(); vk = json.load(open(env['vkey']))
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    voter = random_voter(random.Random(21), ol.poseidon, nLevels=NL, depth_c=7, depth_s=3)
    ws, st = ctx.witness([voter], nLevels=NL)
    assert st == [0]
    r, s = 0x1234567, R - 3
    proof, pub = pk.prove(ws[0], r, s)
    pk.close()
    monkeypatch.setattr(cf, 'toxic_waste', lambda seed: [TAU, ALPHA, BETA, 1, 1])
    a, b, c = cf.proof_scalars(env['r1cs'], 0, ws[0], r, s)
    assert proof == cf.proof_from_scalars(ol, a, b, c)
    assert ol.verify(vk, pub, proof)
    out = groth16.fullProve(voter, None, env['zkey'])
    assert groth16.verify(vk, out['publicSignals'], out['proof']) is True
    bad = list(out['publicSignals']); bad[1] = str((int(bad[1]) + 1) % R)
    assert groth16.verify(vk, bad, out['proof']) is False


def test_ceremony_on_the_ptau_key_and_zkey_verify_against_the_circuit(env):
    from zkcensus_amd import phase2, setup
    ctx, d = env['ctx'], env['dir']
    init = open(env['zkey'], 'rb').read()
    k1, _ = phase2.contribute(ctx, init, 0x1234567890abcdef % R, 'first')
    k2, _ = phase2.contribute(ctx, k1, (R - 7) // 5, 'second')
    assert phase2.verify_circuit(ctx, env['r1cs'], env['ptau'], k2, SEED) == (True, 2, '')
    assert phase2.verify_circuit(ctx, env['r1cs'], env['ptau'], init, SEED) == (True, 0, '')
    # one C point replaced by its neighbour
    off, p = {}, 12
    for _ in range(struct.unpack_from('<I', k2, 8)[0]):
        i, sz = struct.unpack_from('<IQ', k2, p); off[i] = p + 12; p += 12 + sz
    forged = bytearray(k2); forged[off[8] + 64 * 40:off[8] + 64 * 41] = k2[off[8] + 64 * 41:off[8] + 64 * 42]
    ok, n_new, why = phase2.verify_circuit(ctx, env['r1cs'], env['ptau'], bytes(forged), SEED)
    assert (ok, n_new) == (False, 2) and why.startswith('check (e): the C points (section 8)'), why
    # another circuit: one coefficient of the first constraint's A side changed
    raw = bytearray(open(env['r1cs'], 'rb').read())
    q, secs = 12, {}
    for _ in range(struct.unpack_from('<I', raw, 8)[0]):
        i, sz = struct.unpack_from('<IQ', raw, q); secs[i] = q + 12; q += 12 + sz
    c0 = secs[2]
    assert struct.unpack_from('<I', raw, c0)[0] >= 1
    coef = int.from_bytes(raw[c0 + 8:c0 + 40], 'little')
    raw[c0 + 8:c0 + 40] = ((coef + 1) % R).to_bytes(32, 'little')
    other = str(d / 'other.r1cs'); open(other, 'wb').write(raw)
    ok, n_new, why = phase2.verify_circuit(ctx, other, env['ptau'], k2, SEED)
    assert not ok and why.startswith('check (a): section '), why
    # the circuit hash binds the transcript to its circuit
    oz = str(d / 'other.zkey'); setup.from_ptau(other, env['ptau'], oz, None, ctx=ctx)
    cs, recs = phase2.contributions(k2)
    cs_other, _ = phase2.contributions(open(oz, 'rb').read())
    assert cs != bytes(64) and cs_other != bytes(64) and cs != cs_other and len(recs) == 2
    assert phase2.contributions(init)[0] == cs
