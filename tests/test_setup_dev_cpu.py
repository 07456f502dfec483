"""CPU: the surface of the device key generator (include/zkcensus_setup.h) and the bytes of the host generator it must reproduce.  The host generator's nLevels-10 key
(default seed) is pinned by its SHA-256, taken before zkc_setup.hip was split into stages: tests/golden/setup_nl10_sha256.json."""
import ctypes, hashlib, json, os, re
import oracle_lib as ol
from zkcensus_amd import _native, setup

NEW = ('zkc_g1_fixed_mul_dev', 'zkc_g2_fixed_mul_dev', 'zkc_setup_from_r1cs_dev', 'zkc_fixed_mul_window', 'zkc_setup_stats')


def test_new_symbols_are_declared_and_exported():
    inc = os.path.join(ol.ROOT, 'include')
    assert re.search(r'^#include "zkcensus_setup.h"', open(os.path.join(inc, 'zkcensus.h')).read(), re.M)
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(inc, 'zkcensus_setup.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(zkc_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(NEW)
    lib = _native.load()
    for s in NEW:
        assert hasattr(lib, s), 'libzkcensus.so does not export ' + s
    assert lib.zkc_fixed_mul_window() in (1, 2, 4, 8, 16)          # the windows tile the 256 bits of a scalar


def test_device_setup_without_a_context_touches_no_file(tmp_path):
    lib = _native.load()
    z, v = tmp_path / 'k.zkey', tmp_path / 'k.json'
    err = ctypes.create_string_buffer(256)
    rc = lib.zkc_setup_from_r1cs_dev(None, str(tmp_path / 'missing.r1cs').encode(), 1, str(z).encode(), str(v).encode(), err, 256)
    assert rc == 4                                                  # ZKC_ERR_BAD_ARG, not the "cannot open" ZKC_ERR_FORMAT of a file that was tried
    assert 'cannot open' not in err.value.decode()
    assert os.listdir(str(tmp_path)) == []
    assert lib.zkc_setup_stats(None) == 4


def test_host_generator_bytes_are_the_pinned_ones(tmp_path):
    pin = json.load(open(ol.golden('setup_nl10_sha256.json')))
    assert pin['nLevels'] == 10 and int(pin['seed'], 16) == setup.DEFAULT_SEED
    _, z, v = setup.ensure_test_artifacts(10, directory=str(tmp_path))
    assert hashlib.sha256(open(z, 'rb').read()).hexdigest() == pin['zkey_sha256']
    assert hashlib.sha256(open(v, 'rb').read()).hexdigest() == pin['vkey_json_sha256']
    st = (ctypes.c_double * 4)()
    assert _native.load().zkc_setup_stats(st) == 0 and all(x >= 0 for x in st) and st[2] > 0
