"""CPU: the host side of the phase-2 ceremony (include/zkcensus_phase2.h) where no GPU is needed: BLAKE2b-512 against hashlib, the section-10 reader on hand-built
images and on every malformed shape it must refuse, the same reader (and BLAKE2b) under ASan + UBSan as a stand-alone program, the G2 challenge of a transcript against
a restatement in Python integers, and the addition chain of the scale kernel on the host (tools/probe/f29_scale_host_test.hip)."""
import ctypes, hashlib, os, shutil, struct, subprocess
import pytest
import oracle_lib as ol
from g2_py import g2_bytes, on_twist, in_g2
from g2_challenge import challenge_py
from zkcensus_amd import _native, phase2

ROOT = ol.ROOT
Q, R = ol.Q, ol.R
FMT = 5                                                        # ZKC_ERR_FORMAT
NEW_ENTRY_POINTS = sorted(['zkc_g1_scale_dev', 'zkc_blake2b512', 'zkc_zkey_contributions', 'zkc_zkey_contribute', 'zkc_zkey_verify_contributions', 'zkc_phase2_stats',
                           'zkc_debug_phase2_challenge_g2', 'zkc_debug_phase2_host_scale'])


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_phase2.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert '#include "zkcensus_phase2.h"' in open(os.path.join(ROOT, 'include', 'zkcensus.h')).read()


@pytest.mark.parametrize('n', [0, 1, 63, 64, 127, 128, 129, 1000])
def test_blake2b512_against_hashlib(n):
    data = bytes((7 * i + n) & 0xff for i in range(n))
    assert phase2.blake2b512(data) == hashlib.blake2b(data, digest_size=64).digest()


# ---- section 10 ----
def record(seed, typ=0, params=b''):
    body = bytes((seed + 3 * i) & 0xff for i in range(3 * 64 + 128 + 64))
    return body + struct.pack('<II', typ, len(params)) + params


def image(section10, with10=True, trailing=False):
    secs = [(1, struct.pack('<I', 1))] + ([(10, section10)] if with10 else []) + ([(3, bytes(8))] if trailing else [])
    return b'zkey' + struct.pack('<II', 1, len(secs)) + b''.join(struct.pack('<IQ', i, len(p)) + p for i, p in secs)


def section(records, count=None, cs=bytes(range(64))):
    return cs + struct.pack('<I', len(records) if count is None else count) + b''.join(records)


def refused(img):
    with pytest.raises(_native.ZkcError) as ei:
        phase2.contributions(img)
    assert ei.value.code == FMT
    return str(ei.value)


def test_contributions_of_the_test_key():
    from zkcensus_amd import setup
    _, z, _ = setup.ensure_test_artifacts(10)
    cs, recs = phase2.contributions(open(z, 'rb').read())
    assert cs == bytes(64) and recs == []


def test_contributions_of_hand_built_sections():
    name64 = bytes(range(65, 65 + 26)) * 3
    name64 = name64[:64]
    beacon = b'\x01\x03end' + b'\x02\x0a' + b'\x03\x20' + bytes(range(32))
    recs = [record(1, 0, b'\x01\x00'), record(2, 0, b'\x01\x40' + name64), record(3, 1, beacon), record(4)]
    for trailing in (False, True):
        cs, got = phase2.contributions(image(section(recs), trailing=trailing))
        assert cs == bytes(range(64)) and len(got) == 4
        assert [g['raw'] for g in got] == recs                                      # a beacon is carried through byte for byte
        assert got[0]['name'] == b'' and got[1]['name'] == name64 and got[3]['name'] is None
        assert got[2]['type'] == 1 and got[2]['name'] == b'end' and got[2]['iterExp'] == 10 and got[2]['beaconHash'] == bytes(range(32))
        assert got[1]['deltaAfter'] == recs[1][:64] and got[1]['g2_spx'] == recs[1][192:320] and got[1]['transcript'] == recs[1][320:384]
    two = phase2.contributions(image(section(recs[:2])))[1]
    assert len(two) == 2 and two[1]['name'] == name64


def test_malformed_sections_are_refused_with_their_text():
    r0, r1 = record(1, 0, b'\x01\x02ab'), record(2)
    good = section([r0, r1])
    assert len(phase2.contributions(image(good))[1]) == 2
    assert 'missing section 10' in refused(image(good, with10=False))
    assert 'shorter than its header' in refused(image(good[:67]))
    assert 'count does not fit' in refused(image(section([r0, r1], count=3)))
    assert 'count does not fit' in refused(image(section([r0, r1], count=0xffffffff)))
    assert 'truncated contribution record (record 1)' in refused(image(good[:-1]))
    assert 'truncated contribution record (record 1)' in refused(image(section([r0, r1[:391] + bytes(1)], count=2)[:-1]))
    assert 'bytes after the last contribution record' in refused(image(good + b'\x00'))
    assert 'bytes after the last contribution record' in refused(image(section([r0, r1], count=1)))
    big = record(2)[:388] + struct.pack('<I', 5)                                      # paramsLen 5 with no parameter bytes behind it
    assert 'paramsLen reaches beyond the section (record 1)' in refused(image(section([r0, big])))
    assert 'paramsLen reaches beyond the section' in refused(image(section([record(1)[:388] + struct.pack('<I', 0xffffffff)])))
    assert 'unknown parameter tag 7 (record 0)' in refused(image(section([record(1, 0, b'\x07\x00')])))
    assert 'truncated parameter (record 0)' in refused(image(section([record(1, 0, b'\x01\x05abc')])))
    assert 'truncated parameter (record 0)' in refused(image(section([record(1, 1, b'\x02')])))
    assert 'unknown contribution type 2' in refused(image(section([record(1, 2)])))
    assert 'beacon parameter in a contribution that is no beacon' in refused(image(section([record(1, 0, b'\x02\x0a')])))
    assert 'not a zkey' in refused(b'zkez' + image(good)[4:])


def test_section10_reader_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / 'phase2_parse_asan')
    cmd = ['g++', '-std=c++17', '-O2', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', os.path.join(ROOT, 'tests', 'host', 'phase2_parse_asan.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1'))
    assert r.returncode == 0 and 'phase2 reader: ok' in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- the G2 challenge against its restatement with hashlib and integers (tests/g2_challenge.py, which phase 1's record writer shares) ----
@pytest.mark.parametrize('transcript', [bytes(64), bytes(range(64)), hashlib.blake2b(b'zkcensus phase 2', digest_size=64).digest()])
def test_challenge_g2_against_the_python_restatement(transcript):
    out = ctypes.create_string_buffer(128)
    assert _native.load().zkc_debug_phase2_challenge_g2(transcript, out) == 0
    p = challenge_py(transcript)
    assert out.raw == g2_bytes(p)
    assert on_twist(p) and in_g2(p) and p is not None


def test_challenges_of_different_transcripts_differ():
    L, a, b = _native.load(), ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    L.zkc_debug_phase2_challenge_g2(bytes(64), a); L.zkc_debug_phase2_challenge_g2(bytes(63) + b'\x01', b)
    assert a.raw != b.raw and a.raw != bytes(128)


def test_scale_chain_on_the_host(tmp_path):
    """f29_acc_dbl + f29_madd along the non-adjacent form, on the host: equal to double-and-add for the edge scalars, the exceptional addition met by r - 2 alone, and the
    accumulator inside the invariant both formulas are written for"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'f29_scale_host_test')
    csrc = os.path.join(ROOT, 'zk-franchise-proof-circuit_amd', 'csrc')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O2', '-std=c++17', '-I' + csrc, '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tools', 'probe', 'f29_scale_host_test.hip'), '-o', exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and '0 mismatches' in out.stdout, out.stdout + out.stderr


def test_host_scale_hook_against_the_oracle():
    """the CPU side of the comparison tools/phase2_bench.py records: n Montgomery points times one scalar on host threads, more threads than points included"""
    lib = _native.load()
    G = (1).to_bytes(32, 'little') + (2).to_bytes(32, 'little')
    mont = lambda b: b''.join((int.from_bytes(b[i:i + 32], 'little') * (1 << 256) % Q).to_bytes(32, 'little') for i in range(0, 64, 32)) if any(b) else b
    pts = [ol.g1_mul(G, a) for a in (1, 2, 12345, R - 1)] + [bytes(64)]
    for k, threads in ((1, 1), (R - 1, 3), (0x1234567890abcdef1234567890abcdef % R, 16), (0, 2)):
        out, ms = ctypes.create_string_buffer(64 * len(pts)), ctypes.c_double(-1)
        assert lib.zkc_debug_phase2_host_scale(b''.join(mont(p) for p in pts), len(pts), k.to_bytes(32, 'little'), threads, out, ctypes.byref(ms)) == 0 and ms.value >= 0
        assert out.raw == b''.join(mont(ol.g1_mul(p, k)) if any(p) and k else bytes(64) for p in pts), k
    out = ctypes.create_string_buffer(64)
    assert lib.zkc_debug_phase2_host_scale(mont(G), 1, R.to_bytes(32, 'little'), 1, out, None) == 4
    assert lib.zkc_debug_phase2_host_scale(mont(G), 0, (1).to_bytes(32, 'little'), 1, out, None) == 4
    assert lib.zkc_debug_phase2_host_scale(mont(G), 1, (1).to_bytes(32, 'little'), 0, out, None) == 4
