"""GPU: the phase-2 ceremony (include/zkcensus_phase2.h) on the nLevels-10 test key: a contribution with a known secret held against the CPU oracle and a Python
recomputation of its hashes, a key whose section 10 is not its last section, proofs under the contributed key, chains of contributions, and twelve forgeries, each
refused by the check that is there for it.
The key stays TEST ONLY: its toxic waste is known, which is what lets the test state delta1 = (delta delta') G."""
import hashlib, os, random, struct, sys
import pytest
import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
MONT = 1 << 256
NL = 10
DELTA1 = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % R
DELTA2 = (R - 5) // 3
SEED = bytes(range(32))


def _le(x):
    return x.to_bytes(32, 'little')


def from_mont(b):
    """a point of a .zkey (little-endian Montgomery coordinates) -> the standard form of the C ABI"""
    if not any(b): return bytes(len(b))
    inv = pow(MONT, -1, Q)
    return b''.join(_le(int.from_bytes(b[i:i + 32], 'little') * inv % Q) for i in range(0, len(b), 32))


def to_mont(b):
    if not any(b): return bytes(len(b))
    return b''.join(_le(int.from_bytes(b[i:i + 32], 'little') * MONT % Q) for i in range(0, len(b), 32))


def sections(z):
    """id -> (offset of the payload, size)"""
    out, p = {}, 12
    for _ in range(struct.unpack_from('<I', z, 8)[0]):
        i, sz = struct.unpack_from('<IQ', z, p)
        out[i] = (p + 12, sz); p += 12 + sz
    return out


def unc(pt_mont):
    """the uncompressed form a hash takes: big-endian standard-form coordinates, G2 components c1 before c0"""
    s = from_mont(pt_mont)
    c = [s[i:i + 32][::-1] for i in range(0, len(s), 32)]
    if len(c) == 4: c = [c[1], c[0], c[3], c[2]]
    out = b''.join(c)
    return out if any(s) else bytes([0x40]) + out[1:]


def pubkey(rec):
    return unc(rec['deltaAfter']) + unc(rec['g1_s']) + unc(rec['g1_sx']) + unc(rec['g2_spx']) + rec['transcript']


def seed_delta(seed):
    """the delta zkc_setup_from_r1cs derives from its seed (csrc/zkc_setup.hip): splitmix64, four draws per element, the fifth element"""
    s, M = seed, (1 << 64) - 1
    def nxt():
        nonlocal s
        s = (s + 0x9E3779B97F4A7C15) & M
        z = s; z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M; z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    def fr():
        v = sum(nxt() << (64 * i) for i in range(4)) & ((1 << 253) - 1)
        return v if v & ((1 << 64) - 1) else v | 1
    return [fr() for _ in range(5)][4]


@pytest.fixture(scope='module')
def env():
    import torch, zkcensus_amd
    from zkcensus_amd import setup, phase2
    ctx = zkcensus_amd.Context(0)
    _, zp, _ = setup.ensure_test_artifacts(NL, ctx=ctx)
    init = open(zp, 'rb').read()
    k1, h1 = phase2.contribute(ctx, init, DELTA1, 'first')
    k2, h2 = phase2.contribute(ctx, k1, DELTA2, 'x' * 80)
    yield {'ctx': ctx, 'torch': torch, 'init': init, 'k1': k1, 'h1': h1, 'k2': k2, 'h2': h2}
    ctx.close()


def test_contribution_with_a_known_secret(env):
    from zkcensus_amd import phase2, engines, setup
    init, k1 = env['init'], env['k1']
    si, s1 = sections(init), sections(k1)
    assert [i for i in s1] == [i for i in si] and all(s1[i] == si[i] for i in range(1, 10))          # section 10 is last in a generated key: nothing before it moved
    d1_off, d2_off = si[2][0] + 468, si[2][0] + 532
    changed = [(d1_off, d1_off + 64 + 128), (si[8][0], si[8][0] + si[8][1]), (si[9][0], si[9][0] + si[9][1])]
    mask = bytearray(init)
    for a, b in changed: mask[a:b] = k1[a:b]
    end10 = si[10][0] + si[10][1]
    assert bytes(mask[:si[10][0] - 8]) == k1[:si[10][0] - 8] and init[si[10][0]:si[10][0] + 64] == k1[s1[10][0]:s1[10][0] + 64]      # every byte outside delta1, delta2, sections 8-10
    assert len(k1) == len(init) + s1[10][1] - si[10][1] and init[end10:] == b''
    # delta1 = (delta delta') G, by the fixed-base engine
    ctx, torch = env['ctx'], env['torch']
    import numpy as np
    d_k = torch.from_numpy(np.frombuffer(_le(seed_delta(setup.DEFAULT_SEED) * DELTA1 % R), dtype=np.uint8).copy()).cuda(); d_o = torch.zeros(64, dtype=torch.uint8, device='cuda')
    engines.g1_fixed_mul(ctx, engines.G1_GENERATOR, d_k.data_ptr(), 1, d_o.data_ptr())
    assert from_mont(k1[d1_off:d1_off + 64]) == d_o.cpu().numpy().tobytes()
    assert from_mont(init[d1_off:d1_off + 64]) == ol.g1_mul(engines.G1_GENERATOR, seed_delta(setup.DEFAULT_SEED))
    # C and H points: 32 samples, first and last of each section included, against the oracle's product by 1 / delta'
    dinv = pow(DELTA1, -1, R); rng = random.Random(3)
    for sec in (8, 9):
        n = si[sec][1] // 64
        for i in sorted(set([0, n - 1] + rng.sample(range(n), 14))):
            a = si[sec][0] + 64 * i
            assert from_mont(k1[a:a + 64]) == ol.g1_mul(from_mont(init[a:a + 64]), dinv), (sec, i)
    # the record, its name, the hashes
    cs, recs = phase2.contributions(k1)
    assert cs == init[si[10][0]:si[10][0] + 64] and len(recs) == 1
    r = recs[0]
    assert r['type'] == 0 and r['name'] == b'first' and r['deltaAfter'] == k1[d1_off:d1_off + 64]
    assert r['transcript'] == hashlib.blake2b(cs + unc(r['g1_s']) + unc(r['g1_sx']), digest_size=64).digest()
    assert env['h1'] == hashlib.blake2b(cs + pubkey(r), digest_size=64).digest()
    assert from_mont(r['g1_sx']) == ol.g1_mul(from_mont(r['g1_s']), DELTA1)
    cs2, recs2 = phase2.contributions(env['k2'])
    assert len(recs2) == 2 and recs2[0]['raw'] == r['raw'] and recs2[1]['name'] == b'x' * 64               # the name is cut at 64 bytes
    assert recs2[1]['transcript'] == hashlib.blake2b(cs + pubkey(r) + unc(recs2[1]['g1_s']) + unc(recs2[1]['g1_sx']), digest_size=64).digest()
    assert env['h2'] == hashlib.blake2b(cs + pubkey(r) + pubkey(recs2[1]), digest_size=64).digest()


def test_contribution_to_a_key_whose_section_10_is_not_last(env):
    """A generated key ends with section 10; a .zkey may hold its sections in any order.  Here the log sits between sections 2 and 3 and again at the very front, so the
    appended record moves every later section: each must arrive intact, under an unchanged header, in the order it had."""
    from zkcensus_amd import phase2
    ctx, init, k1 = env['ctx'], env['init'], env['k1']
    si, s1 = sections(init), sections(k1)

    def image(z, sec, order):
        body = b''.join(struct.pack('<IQ', i, sec[i][1]) + z[sec[i][0]:sec[i][0] + sec[i][1]] for i in order)
        return z[:12] + body

    assert image(init, si, list(si)) == init
    for order in ([1, 2, 10, 3, 4, 5, 6, 7, 8, 9], [10, 9, 8, 7, 6, 5, 4, 3, 2, 1]):
        moved = image(init, si, order)
        out, h = phase2.contribute(ctx, moved, DELTA1, 'first')
        so = sections(out)
        assert list(so) == order and len(out) == len(k1)
        end = max(so[i][0] + so[i][1] for i in so)
        assert end == len(out)                                                         # the section headers add up to the whole image
        for i in (1, 3, 4, 5, 6, 7):
            assert out[so[i][0]:so[i][0] + so[i][1]] == init[si[i][0]:si[i][0] + si[i][1]], i
        for i in (2, 8, 9):                                                            # the same secret: the same delta1, delta2, C and H as the contribution to the plain key
            assert out[so[i][0]:so[i][0] + so[i][1]] == k1[s1[i][0]:s1[i][0] + s1[i][1]], i
        assert so[10][1] == s1[10][1]
        cs, recs = phase2.contributions(out)
        assert cs == init[si[10][0]:si[10][0] + 64] and len(recs) == 1 and recs[0]['name'] == b'first' and recs[0]['type'] == 0
        assert recs[0]['deltaAfter'] == k1[s1[2][0] + 468:s1[2][0] + 532]
        assert h == hashlib.blake2b(cs + pubkey(recs[0]), digest_size=64).digest()
        assert phase2.verify(ctx, moved, out, SEED) == (True, 1, '')
        assert phase2.verify(ctx, init, out, SEED) == (True, 1, '')                    # the order of the sections is no part of what a contribution is checked for
        again, _ = phase2.contribute(ctx, out, DELTA2, 'second')                       # and a second record goes behind the first, in the same place
        assert list(sections(again)) == order and phase2.verify(ctx, moved, again, SEED) == (True, 2, '')


def test_proofs_under_the_contributed_key(env):
    import numpy as np, zkcensus_amd
    from census_gen import random_voter
    ctx, torch, init, k1 = env['ctx'], env['torch'], env['init'], env['k1']
    B, rng = 4, random.Random(12)
    voters = [random_voter(rng, ol.poseidon, nLevels=NL, depth_c=rng.randint(1, NL), depth_s=rng.randint(1, NL)) for _ in range(B)]
    flat = b''.join(zkcensus_amd.flatten_inputs(v, NL) for v in voters)
    d_in = torch.from_numpy(np.frombuffer(flat, dtype=np.uint8).copy()).cuda()
    nW = ctx.n_wires(NL)
    d_w = torch.zeros(B * nW * 32, dtype=torch.uint8, device='cuda'); d_st = torch.zeros(B, dtype=torch.int32, device='cuda')
    rs = b''.join(_le(rng.randrange(1 << 248)) for _ in range(2 * B))
    pk = zkcensus_amd.ProvingKey(ctx, k1)
    proofs, pubs = pk.fullprove_batch_dev(d_in.data_ptr(), B, d_w.data_ptr(), d_st.data_ptr(), rs)
    pk.close()
    assert d_st.cpu().tolist() == [0] * B
    ws = d_w.cpu().numpy().tobytes()
    vk1, vk0 = ol.zkey_vk(k1), ol.zkey_vk(init)
    lib = ctx._lib
    for i in range(B):
        r_i, s_i = (int.from_bytes(rs[64 * i + 32 * j:64 * i + 32 * j + 32], 'little') for j in range(2))
        rc, op, opub = ol.prove(k1, ws[i * nW * 32:(i + 1) * nW * 32], r_i, s_i)
        assert rc == 0 and op == proofs[256 * i:256 * i + 256] and opub == pubs[256 * i:256 * i + 256]
        assert lib.zkc_verify_bin(vk1, 8, pubs[256 * i:256 * i + 256], proofs[256 * i:256 * i + 256]) == 1
        assert lib.zkc_verify_bin(vk0, 8, pubs[256 * i:256 * i + 256], proofs[256 * i:256 * i + 256]) == 0
    assert lib.zkc_verify_batch(ctx._h, vk1, 8, pubs, proofs, B, SEED) == 1
    assert lib.zkc_verify_batch(ctx._h, vk0, 8, pubs, proofs, B, SEED) == 0


def test_chains(env):
    from zkcensus_amd import phase2
    ctx, init, k1, k2 = env['ctx'], env['init'], env['k1'], env['k2']
    assert phase2.verify(ctx, init, k2, SEED) == (True, 2, '')
    assert phase2.verify(ctx, k1, k2, SEED) == (True, 1, '')
    assert phase2.verify(ctx, init, init, SEED) == (True, 0, '')
    assert phase2.verify(ctx, init, k1) == (True, 1, '')                             # weights from the OS generator
    ok, _, why = phase2.verify(ctx, k2, k1, SEED)
    assert not ok and 'check (b)' in why
    a, ha = phase2.contribute(ctx, init)
    b, hb = phase2.contribute(ctx, init)
    assert a != b and ha != hb
    assert phase2.verify(ctx, init, a, SEED)[:2] == (True, 1) and phase2.verify(ctx, init, b, SEED)[:2] == (True, 1)
    import zkcensus_amd
    for bad in (0, R, (1 << 256) - 1):
        with pytest.raises(zkcensus_amd.ZkcError) as ei:
            phase2.contribute(ctx, init, bad)
        assert ei.value.code == 4


def g1_add_std(p, q):
    """p + q for two different finite points in standard form (Python integers)"""
    x1, y1, x2, y2 = (int.from_bytes(b[i:i + 32], 'little') for b in (p, q) for i in (0, 32))
    lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return _le(x3) + _le((lam * (x1 - x3) - y1) % Q)


def g1_neg_std(p):
    return p[:32] + _le(-int.from_bytes(p[32:], 'little') % Q)


def test_forgeries_are_refused_by_the_check_that_is_there_for_them(env):
    from zkcensus_amd import phase2, engines
    ctx, init, k1, k2 = env['ctx'], env['init'], env['k1'], env['k2']
    s = sections(k1)
    G = engines.G1_GENERATOR

    def put(img, off, b):
        return img[:off] + b + img[off + len(b):]

    def pt(img, sec, i):
        return img[s[sec][0] + 64 * i:s[sec][0] + 64 * i + 64]

    def refused(forged, check, base=init, seed=SEED):
        ok, _, why = phase2.verify(ctx, base, forged, seed)
        assert not ok and check in why, why
    c8, h9 = s[8][0], s[9][0]
    # (i) one C point doubled
    refused(put(k1, c8 + 64 * 5, to_mont(ol.g1_mul(from_mont(pt(k1, 8, 5)), 2))), 'check (e): the C points')
    # (ii) two neighbouring H points swapped
    refused(put(k1, h9 + 64 * 7, pt(k1, 9, 8) + pt(k1, 9, 7)), 'check (e): the H points')
    # (iii) C0 += G, C1 -= G: the unweighted sum is unchanged; three seeds
    f3 = put(k1, c8, to_mont(g1_add_std(from_mont(pt(k1, 8, 0)), G)) + to_mont(g1_add_std(from_mont(pt(k1, 8, 1)), g1_neg_std(G))))
    for seed in (SEED, bytes([7]) * 32, hashlib.sha256(b'three').digest()):
        refused(f3, 'check (e): the C points', seed=seed)
    # (iv) H scaled by another scalar than C: the H section of a contribution with another secret
    other, _ = phase2.contribute(ctx, init, DELTA1 + 1, 'first')
    refused(put(k1, h9, other[h9:h9 + s[9][1]]), 'check (e): the H points')
    # (v) delta2 from another secret
    d1_off, d2_off = s[2][0] + 468, s[2][0] + 532
    refused(put(k1, d2_off, other[d2_off:d2_off + 128]), 'check (d): sameRatio(G1, delta1; G2, delta2)')
    # (vi) deltaAfter altered (to another point of the curve), (vii) g1_sx altered, (viii) a transcript byte flipped
    rec = s[10][0] + 68
    refused(put(k1, rec, other[d1_off:d1_off + 64]), 'sameRatio(delta, deltaAfter; g2_sp, g2_spx)')
    refused(put(k1, rec + 128, to_mont(ol.g1_mul(from_mont(k1[rec + 128:rec + 192]), 2))), 'check (c), contribution 0: the stored transcript')
    refused(put(k1, rec + 320 + 9, bytes([k1[rec + 320 + 9] ^ 1])), 'check (c), contribution 0: the stored transcript')
    # (xii) g1_sx from another secret (twice the honest one) under a transcript recomputed for it: the stored transcript is then the right one, the challenge follows
    # it, and only the proof of knowledge itself, sameRatio(g1_s, g1_sx; g2_sp, g2_spx), is left to refuse the record
    cs = k1[s[10][0]:s[10][0] + 64]
    sx2 = to_mont(ol.g1_mul(from_mont(k1[rec + 128:rec + 192]), 2))
    f12 = put(k1, rec + 128, sx2)
    f12 = put(f12, rec + 320, hashlib.blake2b(cs + unc(k1[rec + 64:rec + 128]) + unc(sx2), digest_size=64).digest())
    refused(f12, 'check (c), contribution 0: sameRatio(g1_s, g1_sx; g2_sp, g2_spx)')
    # (ix) one byte of section 5 flipped
    refused(put(k1, s[5][0] + 100, bytes([k1[s[5][0] + 100] ^ 0x10])), 'check (a): section 5')
    # (x) the last record dropped while delta1 is kept: k2 with its second record cut out
    s2 = sections(k2)
    recs = phase2.contributions(k2)[1]
    cut = len(recs[1]['raw'])
    f10 = k2[:len(k2) - cut]
    f10 = put(f10, s2[10][0] - 8, struct.pack('<Q', s2[10][1] - cut)); f10 = put(f10, s2[10][0] + 64, struct.pack('<I', 1))
    assert len(phase2.contributions(f10)[1]) == 1
    refused(f10, 'check (d): the final key\'s delta1')
    refused(f10, 'check (d): the final key\'s delta1', base=k1)
    # (xi) a type-1 record in the chain
    refused(put(k1, rec + 384, struct.pack('<I', 1)), 'a beacon contribution (type 1)')
    # and the untouched key still passes
    assert phase2.verify(ctx, init, k1, SEED) == (True, 1, '')
