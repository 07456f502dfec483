"""CPU: keys from a prepared powers-of-tau file on host threads (ctx = None) for the circuit of tests/repeat_circuits.py, whose rows repeat one point up to 65 536 times:
P + P, P - P, equal and opposite partial sums, rows at each side of a third reduction step.  Every wire's A, B1, B2 and K point is held against its exponent, summed
over terms in Python and multiplied by the CPU oracle, and the whole key against the seeded generator with the same waste (zkc_debug_setup_from_waste), which never
sees a point of the file.  This is what tests/test_gpu_ptau_setup_repeats.py rests its "device bytes equal host bytes" on."""
import ctypes, os
import pytest
import oracle_lib as ol
import ptau_lib as pl
import repeat_circuits as rc
from zkcensus_amd import _native, setup

R = ol.R
TAU, ALPHA, BETA = 0x1f3a5c7e9b2d4f6081a3c5e7092b4d6f8fa1c3e5072 % R, 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da5 % R, 0x9e3779b97f4a7c15f39cc0605cedc8341082276bf3a27251 % R
WASTES = {'plain': (TAU, ALPHA, BETA), 'alpha=beta': (TAU, ALPHA, ALPHA)}


@pytest.fixture(scope='module')
def r1cs(tmp_path_factory):
    return rc.write(str(tmp_path_factory.mktemp('repeats') / 'repeats.r1cs'))


@pytest.fixture(scope='module', params=list(WASTES))
def key(request, r1cs, tmp_path_factory):
    """one host from_ptau and one seeded generation per waste"""
    d = tmp_path_factory.mktemp('key')
    waste = WASTES[request.param]
    ptau = pl.write(str(d / 'a.ptau'), rc.POWER, *waste)
    setup.from_ptau(r1cs, ptau, d / 'p.zkey', d / 'p.json')
    err = ctypes.create_string_buffer(512)
    res = _native.load().zkc_debug_setup_from_waste(os.fsencode(r1cs), *[ol.le32(x) for x in waste + (1, 1)], os.fsencode(d / 'w.zkey'), os.fsencode(d / 'w.json'), err, 512)
    assert res == 0, err.value
    return {'waste': waste, 'dir': d, 'sections': pl.zkey_sections(open(d / 'p.zkey', 'rb').read())}


def test_every_wire_is_its_exponent_times_the_generator(key):
    A, B, K = rc.exponents(*key['waste'])
    assert len(key['sections'][5]) == 64 * rc.N_WIRES and len(key['sections'][7]) == 128 * rc.N_WIRES and len(key['sections'][8]) == 64 * (rc.N_WIRES - 1)
    for w in range(rc.N_WIRES):
        assert rc.key_points(key['sections'], w) == rc.oracle_points(A, B, K, w), 'wire %d' % w
    for name, w in rc.WIRE.items():
        if name not in rc.ZERO_ROWS:
            assert A[w] and B[w] and K[w], name                  # a case that is meant to leave a point does


def test_rows_that_cancel_are_infinity(key):
    A, B, K = rc.exponents(*key['waste'])
    for name in rc.ZERO_ROWS:
        w = rc.WIRE[name]
        assert (A[w], B[w], K[w]) == (0, 0, 0), name
        assert rc.key_points(key['sections'], w) == (bytes(64), bytes(64), bytes(128), bytes(64)), name


def test_key_equals_the_seeded_generator_with_the_same_waste(key):
    d = key['dir']
    a, b = key['sections'], pl.zkey_sections(open(d / 'w.zkey', 'rb').read())
    for s in range(1, 10):
        assert a[s] == b[s], 'section %d' % s
    assert open(d / 'p.json', 'rb').read() == open(d / 'w.json', 'rb').read()
