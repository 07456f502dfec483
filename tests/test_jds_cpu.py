"""The one builder of the jagged-diagonal sparse rows (csrc/zkc_jds.h: plain C++17, no HIP) under AddressSanitizer + UBSan on the CPU, as a stand-alone program
(tests/host/jds_host.cc) over a 32-byte stand-in for Fr: no rows, empty rows, a single row, lengths around both long-row thresholds (16: the prover's, 48: the witness
check's), many rows of equal length, one row of 521 terms among short ones, the +1 / -1 markers and their one-bit neighbours.  Both device loaders (zkc_prove.hip,
zkc_r1cs.hip) build their rows through this header."""
import os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jds_builder_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'jds_host')
    base = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', os.path.join(ROOT, 'tests', 'host', 'jds_host.cc'), '-o', exe]
    b = subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], capture_output=True, text=True)
    if b.returncode != 0 and 'cannot find' in (b.stderr or '') and 'san' in b.stderr.lower():
        b = subprocess.run(base, capture_output=True, text=True)               # no sanitizer runtime for g++ here: the checks of the program itself still run
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'jds builder: ok' in r.stdout and 'FAILED' not in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count(': ok (') == 20                                      # ten cases at each threshold
