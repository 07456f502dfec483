"""The host-only .r1cs reader (csrc/zkc_r1cs_parse.h) under AddressSanitizer + UBSan on the CPU, as a stand-alone program (tests/host/r1cs_parse_asan.cc): the census
circuit's image at nLevels 10, every prefix of its first 4 KB, cuts at the section boundaries and a few thousand seeded single-byte mutations.  Every malformed image is
refused or parsed within bounds."""
import os, subprocess
import pytest
from zkcensus_amd import r1cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_r1cs_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'r1cs_parse_asan')
    cmd = ['g++', '-std=c++17', '-O2', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'r1cs_parse_asan.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]
    L, cs = r1cs.build(10)
    path = str(tmp_path / 'census10.r1cs')
    cs.write(path)
    r = subprocess.run([exe, path, str(L.nWires), '8', str(len(cs.cons))], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'r1cs reader: ok' in r.stdout, (r.stdout + r.stderr)[-3000:]
