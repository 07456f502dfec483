"""GPU: the device key generator zkc_setup_from_r1cs_dev (include/zkcensus_setup.h) writes the host generator's files, byte for byte: the census circuit at nLevels 10 under
two seeds, a small random circuit with another nPublic, domain and many wires in no constraint (points at infinity), the same refusals for damaged .r1cs files -- and a
key it made proves and verifies."""
import ctypes, json, os, random, struct, sys
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))


@pytest.fixture(scope='module')
def gpu():
    import zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx
    ctx.close()


def _setup(ctx, r1, seed, stem):
    """either generator (ctx None: the host's) -> (rc, message, zkey path, vkey path)"""
    from zkcensus_amd import _native
    lib = _native.load()
    z, v = stem + '.zkey', stem + '_vkey.json'
    err = ctypes.create_string_buffer(512)
    if ctx is None:
        rc = lib.zkc_setup_from_r1cs(r1.encode(), seed, z.encode(), v.encode(), err, 512)
    else:
        rc = lib.zkc_setup_from_r1cs_dev(ctx._h, r1.encode(), seed, z.encode(), v.encode(), err, 512)
    return rc, err.value.decode(), z, v


def first_difference(a, b):
    """where two .zkey images part: (section id, offset inside the section), or ('header', offset) / ('length', sizes)"""
    if a[:12] != b[:12]:
        return 'header', next(i for i in range(12) if a[i:i + 1] != b[i:i + 1])
    p = 12
    while p < len(a):
        sid, n = struct.unpack_from('<IQ', a, p)
        if a[p:p + 12] != b[p:p + 12]:
            return 'section header', sid
        sa, sb = a[p + 12:p + 12 + n], b[p + 12:p + 12 + n]
        if sa != sb:
            return sid, next(i for i in range(n) if sa[i:i + 1] != sb[i:i + 1])
        p += 12 + n
    return ('length', (len(a), len(b))) if len(a) != len(b) else None


def assert_same_key(hz, hv, dz, dv):
    a, b = open(hz, 'rb').read(), open(dz, 'rb').read()
    assert a == b, 'device .zkey differs from the host .zkey first at (section, offset) = %r' % (first_difference(a, b),)
    assert open(hv, 'rb').read() == open(dv, 'rb').read(), 'verification_key.json differs'


@pytest.fixture(scope='module')
def census10():
    from zkcensus_amd import setup
    return setup.ensure_test_artifacts(10)                     # the host generator's key, default seed (shared artifact directory)


def test_first_difference_names_the_section():
    a = b'zkey' + struct.pack('<II', 1, 2) + struct.pack('<IQ', 1, 4) + b'abcd' + struct.pack('<IQ', 2, 3) + b'xyz'
    b = a[:-2] + b'Yz'
    assert first_difference(a, a) is None and first_difference(a, b) == (2, 1)


def test_device_key_equals_host_key_nl10_default_seed(gpu, census10, tmp_path):
    from zkcensus_amd import setup
    r1, hz, hv = census10
    _, dz, dv = setup.ensure_test_artifacts(10, directory=str(tmp_path), ctx=gpu)      # the Python path: same names, same stamp
    assert os.path.basename(dz) == os.path.basename(hz) and open(dz + '.stamp').read() == open(hz + '.stamp').read()
    assert_same_key(hz, hv, dz, dv)
    st = (ctypes.c_double * 4)()
    assert gpu._lib.zkc_setup_stats(st) == 0 and all(x > 0 for x in st)


def test_device_key_equals_host_key_nl10_other_seed(gpu, census10, tmp_path):
    r1 = census10[0]
    rc, msg, hz, hv = _setup(None, r1, 7, str(tmp_path / 'host'))
    assert rc == 0, msg
    rc, msg, dz, dv = _setup(gpu, r1, 7, str(tmp_path / 'dev'))
    assert rc == 0, msg
    assert_same_key(hz, hv, dz, dv)
    assert open(hz, 'rb').read() != open(census10[1], 'rb').read()


def test_device_key_equals_host_key_small_generic_circuit(gpu, tmp_path):
    """tests/big_circuit.py at its small end: 40 constraints over 1500 wires, 2 public -- domain 64, most wires in no constraint, so most points of the key are infinity"""
    import big_circuit as bc
    r1 = str(tmp_path / 'generic.r1cs')
    bc.big_instance(r1, 40, 1500, 2, seed=40)
    rc, msg, hz, hv = _setup(None, r1, 2024, str(tmp_path / 'host'))
    assert rc == 0, msg
    rc, msg, dz, dv = _setup(gpu, r1, 2024, str(tmp_path / 'dev'))
    assert rc == 0, msg
    assert_same_key(hz, hv, dz, dv)
    z = ol.zkey_parse(open(dz, 'rb').read())
    assert (z.nVars, z.nPublic, z.domainSize) == (1500, 2, 64)
    assert json.load(open(dv))['nPublic'] == 2


def test_device_made_key_proves_and_verifies(gpu, census10, tmp_path):
    from census_gen import random_voter
    from zkcensus_amd import groth16
    rc, msg, dz, dv = _setup(gpu, census10[0], 11, str(tmp_path / 'dev'))
    assert rc == 0, msg
    voter = random_voter(random.Random(6), ol.poseidon, nLevels=10, depth_c=5, depth_s=7)
    out = groth16.fullProve(voter, None, dz)
    vk = json.load(open(dv))
    assert groth16.verify(vk, out['publicSignals'], out['proof']) is True                     # zkc_verify under the device-made vkey
    bad = list(out['publicSignals']); bad[0] = str((int(bad[0]) + 1) % ol.R)
    assert groth16.verify(vk, bad, out['proof']) is False


def test_damaged_r1cs_is_refused_as_the_host_refuses_it(gpu, census10, tmp_path):
    raw = open(census10[0], 'rb').read()
    cases = {'cut_in_constraints': raw[:2 * len(raw) // 3], 'cut_in_header': raw[:40], 'not_r1cs': b'r1cz' + raw[4:], 'tiny': raw[:8]}
    texts = set()
    for name, img in cases.items():
        p = str(tmp_path / (name + '.r1cs'))
        open(p, 'wb').write(img)
        h = _setup(None, p, 1, str(tmp_path / ('h_' + name)))
        d = _setup(gpu, p, 1, str(tmp_path / ('d_' + name)))
        assert h[0] == d[0] == 5 and h[1] == d[1] and h[1], name                              # ZKC_ERR_FORMAT, the same words
        assert not os.path.exists(d[2]) and not os.path.exists(d[3])
        texts.add(h[1])
    assert 'r1cs constraints truncated' in texts and 'not an r1cs file' in texts
    missing = str(tmp_path / 'none.r1cs')
    h = _setup(None, missing, 1, str(tmp_path / 'h')); d = _setup(gpu, missing, 1, str(tmp_path / 'd'))
    assert h[:2] == d[:2] == (5, 'cannot open ' + missing)
