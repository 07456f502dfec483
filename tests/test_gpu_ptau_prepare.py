"""GPU: a powers-of-tau file prepared for phase 2 on the device (include/zkcensus_ptau_prepare.h, csrc/zkc_ecntt.hip, csrc/zkc_ptau_prepare.hip).  The transform on its own
is held against the exponents: inputs are k_i G from the fixed-base engines, outputs must be the fixed-base product of (1/n) sum_i w^(-c i) k_i, which Python computes
(tests/ptau_prep_lib.py).  The kernels have no workgroup-resident group of stages and no tile, so the sizes are 0, 1, 2 (the first non-unit twiddle), 6 and 7 (one wave of
butterflies and one past it), 10 and 11, every input vector in place and out of place, with mont 0 and 1.  Then the file: the device must write the host path's bytes (tests/test_ptau_prepare_cpu.py holds that path against the expected
image; here both are), the prepared file must serve as a key source at its own power -- section 9 is the odd half of the padded top block, and a proof under the key equals
the closed form at (tau, alpha, beta, 1, 1) -- check_prepared must name every changed point, and a ceremony over such a key must pass `zkey verify` against the circuit."""
import json, os, random, struct, sys
import pytest
import oracle_lib as ol
import closed_form as cf
import big_circuit
import ptau_lib as pl
import ptau_prep_lib as pp

pytestmark = pytest.mark.gpu
R, Q = ol.R, ol.Q
SEED = bytes(range(32))
TAU, ALPHA, BETA = pp.PLAIN


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    import zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield {'ctx': ctx, 'dir': tmp_path_factory.mktemp('prep')}
    ctx.close()


# ---- the engine against the exponents ----
def fixed(ctx, width, ks):
    """[k G] in standard form (the engines' default), all zero for k = 0"""
    return pl._points_gpu(ctx, width, [k % R for k in ks])


def vectors(logn):
    n = 1 << logn
    out = {name: [pow(tau, i, R) for i in range(n)] for name, (tau, _, _) in pp.wastes(logn).items()}
    rng = random.Random(100 + logn)
    ks = [rng.randrange(1, R) for _ in range(n)]
    for i in (0, 1, n - 1):
        ks[i % n] = 0                                           # infinity among the inputs
    out['random-with-infinity'] = ks
    return out


@pytest.mark.parametrize('width', [64, 128])
@pytest.mark.parametrize('logn', [0, 1, 2, 6, 7, 10, 11])
def test_lagrange_engine_is_the_transform_in_the_exponent(env, logn, width):
    import numpy as np, torch
    from zkcensus_amd import engines
    ctx = env['ctx']; n = 1 << logn
    lag = engines.g1_lagrange if width == 64 else engines.g2_lagrange
    modes = [(m, ip) for m in (False, True) for ip in (False, True)]          # (mont, in place)
    for name, ks in vectors(logn).items():
        src = fixed(ctx, width, ks)
        exp = fixed(ctx, width, pp.intt(ks, logn))
        assert [i for i in range(n) if not any(src[width * i:width * i + width])] == [i for i in range(n) if ks[i] % R == 0]
        for mont, inplace in modes:                             # every vector in every mode at every size
            a, e = (pl.to_mont(src), pl.to_mont(exp)) if mont else (src, exp)
            d_in = torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy()).cuda()
            d_out = d_in if inplace else torch.full((width * n,), 0xab, dtype=torch.uint8, device='cuda')
            lag(ctx, d_in.data_ptr(), logn, d_out.data_ptr(), mont=mont)
            got = d_out.cpu().numpy().tobytes()
            bad = [c for c in range(n) if got[width * c:width * c + width] != e[width * c:width * c + width]]
            assert bad == [], '%s, logn %d, mont %s, in place %s: points %r differ' % (name, logn, mont, inplace, bad[:8])
            if not inplace:
                assert d_in.cpu().numpy().tobytes() == a            # the input is left alone


@pytest.mark.parametrize('width', [64, 128])
def test_lagrange_engine_refuses_bad_points_and_arguments(env, width):
    import numpy as np, torch
    from zkcensus_amd import engines, _native
    ctx = env['ctx']; logn = 7; n = 1 << logn
    lag = engines.g1_lagrange if width == 64 else engines.g2_lagrange
    good = fixed(ctx, width, [3 + 5 * i for i in range(n)])
    for mont in (False, True):
        src = bytearray(pl.to_mont(good) if mont else good)
        src[width * 77 + 1] ^= 1                                     # off the curve
        src[width * 40 + width - 32:width * 40 + width] = Q.to_bytes(32, 'little')      # a coordinate = q, at the smaller index
        d_in = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).cuda()
        d_out = torch.full((width * n,), 0xab, dtype=torch.uint8, device='cuda')
        with pytest.raises(_native.ZkcError) as ei:
            lag(ctx, d_in.data_ptr(), logn, d_out.data_ptr(), mont=mont)
        assert ei.value.code == 5 and 'point 40 has a coordinate >= q or is not on the curve' in str(ei.value)
        assert d_out.cpu().numpy().tobytes() == b'\xab' * (width * n)               # nothing written
    d = torch.zeros(width, dtype=torch.uint8, device='cuda')
    # NULL pointers, and sizes above 2^28: Fr has no larger domain (the argument is refused before anything is read, so the small buffer is never touched)
    for args in ((0, 0, d.data_ptr()), (d.data_ptr(), 0, 0), (d.data_ptr(), 29, d.data_ptr()), (d.data_ptr(), 30, d.data_ptr())):
        with pytest.raises(_native.ZkcError) as ei:
            lag(ctx, args[0], args[1], args[2])
        assert ei.value.code == 4


# ---- the file ----
_files = {}


def files(env, power, waste):
    """(unprepared path, device-prepared path, expected image) of (power, waste name); made once"""
    from zkcensus_amd import setup
    key = (power, waste)
    if key not in _files:
        unprepared, expected, _ = pp.images(power, pp.wastes(power)[waste], env['ctx'])
        src = str(env['dir'] / ('u_%d_%s.ptau' % key)); dst = str(env['dir'] / ('d_%d_%s.ptau' % key))
        open(src, 'wb').write(unprepared)
        setup.prepare_ptau(src, dst, ctx=env['ctx'])
        _files[key] = (src, dst, expected, setup.ptau_prepare_stats())
    return _files[key]


@pytest.mark.parametrize('power,waste', [(1, 'plain'), (2, 'plain'), (3, 'plain'), (7, 'plain'), (11, 'plain'), (11, 'on-domain'), (11, 'on-double-domain'), (11, 'minus-one')])
def test_device_file_equals_host_file(env, power, waste):
    from zkcensus_amd import setup
    src, dst, expected, ms = files(env, power, waste)
    host = str(env['dir'] / 'host.ptau')
    setup.prepare_ptau(src, host)
    dev_img, host_img = open(dst, 'rb').read(), open(host, 'rb').read()
    _, db = pp.parse(dev_img); _, hb = pp.parse(host_img)
    for i in (12, 13, 14, 15):
        w = pl.PT_BYTES[i]
        assert len(db[i]) == len(hb[i])
        diff = [k for k in range(len(hb[i]) // w) if db[i][w * k:w * k + w] != hb[i][w * k:w * k + w]]
        assert diff == [], 'section %d: points %r of the device file differ from the host file' % (i, diff[:8])
    assert dev_img == host_img
    assert dev_img == expected                                   # and both are what the exponents say
    assert all(v > 0 for v in ms.values()), ms
    assert not [f for f in os.listdir(env['dir']) if '.tmp' in f]


# the crafted circuit of tests/test_gpu_ptau_setup.py (copied: that file is not imported from): 1027 constraints + 1, no public wire: domain 2^11
SEG, RED = 32, 32
LENS = [0, 1, SEG - 1, SEG, SEG + 1, SEG * RED - 1, SEG * RED, SEG * RED + 1]
FULL = 0x2a9e3c1f7b5d08e64c3a1f9d7e5b2c0a8f6e4d2b1a0918273645546372819aaf % R


def crafted():
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
    return 13, 0, cons


def test_key_at_the_files_power_and_proofs_under_it(env, monkeypatch):
    """power 11 = the crafted circuit's domain: H is read from the padded top block.  Section 9 is L'_(2i+1) G1.  The crafted circuit's only witness is (1, 0, .., 0), whose
    quotient polynomial is zero, so a random satisfiable circuit of the same domain is proved as well: there h is a full polynomial of degree 2N - 2 and the proof must
    still EQUAL the closed form -- the padded basis and the true one contract to the same point."""
    import zkcensus_amd
    from zkcensus_amd import setup
    ctx, d = env['ctx'], env['dir']
    _, ptau, _, _ = files(env, 11, 'plain')
    n_wires, n_pub, cons = crafted()
    assert 1024 < len(cons) + n_pub + 1 <= 2048
    r1 = pl.write_r1cs(str(d / 'crafted.r1cs'), n_wires, n_pub, cons)
    r2 = str(d / 'random11.r1cs')
    w2 = big_circuit.big_instance(r2, 2048 - 3, 700, 2, seed=4)
    top = pp.top_block_exponents(11, TAU)
    h_expected = pp.points([top[2 * i + 1] for i in range(2048)], 64, ctx)
    monkeypatch.setattr(cf, 'toxic_waste', lambda seed: [TAU, ALPHA, BETA, 1, 1])
    for name, r1cs, wtns, npub in (('crafted', r1, b''.join(ol.le32(x) for x in [1] + [0] * (n_wires - 1)), 0), ('random', r2, w2, 2)):
        zk, vk = str(d / (name + '.zkey')), str(d / (name + '.json'))
        setup.from_ptau(r1cs, ptau, zk, vk, ctx=ctx)
        z = open(zk, 'rb').read()
        s = pl.zkey_sections(z)
        assert struct.unpack_from('<I', s[2], 80)[0] == 2048
        assert s[9] == h_expected, name
        pk = zkcensus_amd.ProvingKey(ctx, z)
        proof, pub = pk.prove(wtns, 0x1234567, R - 3)
        pk.close()
        assert pub == wtns[32:32 * (1 + npub)]
        assert proof == cf.proof_from_scalars(ol, *cf.proof_scalars(r1cs, 0, wtns, 0x1234567, R - 3)), name
        assert ol.verify(json.load(open(vk)), pub, proof), name


def changed(env, img, edits, name):
    m = bytearray(img); off = pp.offsets(img)
    for sec, at, val in edits:
        m[off[sec] + at:off[sec] + at + len(val)] = val
    p = str(env['dir'] / name); open(p, 'wb').write(bytes(m))
    return p


def test_check_prepared_on_the_device(env):
    from zkcensus_amd import setup, _native
    ctx = env['ctx']; power = 7; n = 1 << power
    _, dst, _, _ = files(env, power, 'plain')
    assert setup.check_prepared(dst, ctx=ctx) == (True, 0, 0, '')
    ms = setup.ptau_prepare_stats()
    assert all(v > 0 for v in ms.values()), ms
    img = open(dst, 'rb').read(); _, body = pp.parse(img)
    flip = lambda sec, pt, byte: (sec, pl.PT_BYTES[sec] * pt + byte, bytes([body[sec][pl.PT_BYTES[sec] * pt + byte] ^ 4]))
    for sec, pt in ((12, 2 * n - 1 + 200), (12, 0), (13, n - 1 + 64), (14, 70), (15, 2 * n - 2)):
        ok, s, i, why = setup.check_prepared(changed(env, img, [flip(sec, pt, 33)], 'one.ptau'), ctx=ctx)
        assert (ok, s, i) == (False, sec, pt) and why == 'ptau: section %d point %d is not the transform of section %d' % (sec, pt, sec - 10)
    assert setup.check_prepared(changed(env, img, [flip(15, 3, 0), flip(13, 100, 0), flip(13, 90, 0)], 'three.ptau'), ctx=ctx)[:3] == (False, 13, 90)
    # D onto L_3 and -D onto L_5 of the size-2^power block of section 12: on the curve, same sum
    lag = pl.lagrange_at(TAU, power); b = pl.block(power); D = 0xabcdef
    shifted = changed(env, img, [(12, b.start + 64 * 3, pl.g1_mont(lag[3] + D)), (12, b.start + 64 * 5, pl.g1_mont(lag[5] - D))], 'shift.ptau')
    ok, s, i, why = setup.check_prepared(shifted, ctx=ctx)
    assert (ok, s, i) == (False, 12, n - 1 + 3), why
    # ptau_lib's own file holds the true top block, which no preparer can write
    theirs = str(env['dir'] / 'lib7.ptau'); open(theirs, 'wb').write(pl.assemble(pp.images(power, pp.PLAIN, ctx)[2]))
    assert setup.check_prepared(theirs, ctx=ctx)[:3] == (False, 12, 2 * n - 1)
    # bad monomial points: refused, the smallest index named
    cases = [([flip(2, 150, 1), flip(2, 99, 40)], 'section 2 point 99 has a coordinate >= q or is not on the curve'),
             ([(3, 128 * 17 + 96, Q.to_bytes(32, 'little'))], 'section 3 point 17 has a coordinate >= q or is not on the twist'),
             ([flip(5, n - 1, 2)], 'section 5 point %d has' % (n - 1))]
    for j, (edits, text) in enumerate(cases):
        with pytest.raises(_native.ZkcError) as ei:
            setup.check_prepared(changed(env, img, edits, 'bad.ptau'), ctx=ctx)
        assert ei.value.code == 5 and text in str(ei.value), str(ei.value)
        src = files(env, power, 'plain')[0]
        out = env['dir'] / 'never.ptau'
        with pytest.raises(_native.ZkcError) as ei:
            setup.prepare_ptau(changed(env, open(src, 'rb').read(), edits, 'badu.ptau'), out, ctx=ctx)
        assert ei.value.code == 5 and text in str(ei.value) and not out.exists()
    assert not [f for f in os.listdir(env['dir']) if '.tmp' in f]


def test_ceremony_over_a_key_from_the_prepared_file(env):
    from zkcensus_amd import phase2, setup
    ctx, d = env['ctx'], env['dir']
    _, ptau, _, _ = files(env, 7, 'plain')
    r = str(d / 'c7.r1cs')
    big_circuit.big_instance(r, 128 - 3, 140, 2, seed=9)          # domain 2^7 = the file's power
    zk = str(d / 'c7.zkey')
    setup.from_ptau(r, ptau, zk, None, ctx=ctx)
    init = open(zk, 'rb').read()
    k1, _ = phase2.contribute(ctx, init, 0x1234567890abcdef % R, 'first')
    k2, _ = phase2.contribute(ctx, k1, (R - 7) // 5, 'second')
    assert phase2.verify_circuit(ctx, r, ptau, k2, SEED) == (True, 2, '')
