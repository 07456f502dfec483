"""CPU: the ZKC_* environment switches of libzkcensus are one table (csrc/zkc_switches.h), read in one place, documented in one list (INTEGRATION.md "Switches"), and parsed
the way each reading site parsed its own before the table existed (tests/host/switches_host.cc under ASan + UBSan; the expected values below are those sites' expressions
worked out by hand, not the header's output)."""
import glob
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zk-franchise-proof-circuit_amd', 'csrc')
ROW = re.compile(r'^\s*X\((\w+),\s*(\w+),\s*(-?\w+),\s*(-?\w+),\s*(\w+),\s*"', re.M)
# not library switches: bench.py and the tests read these themselves ...
OWN = re.compile(r'ZKC_(BENCH_\w+|BATCH|CPU_BASELINE_\w+|TEST_FULL|AB_TAG)$')
# ... and these are constants of the C ABI or of the sources (status and error codes, profiling categories, tables), not environment variables
CONST = re.compile(r'ZKC_(ERR|W|SMT|TREE|PROF|POSEIDON)(_|$)|ZKC_OK$')
ENV_USE = re.compile(r'''(?:os\.environ(?:\.(?:get|pop|setdefault))?\s*[\[(]|monkeypatch\.(?:set|del)env\()\s*['"](ZKC_\w+)['"]''')
ENV_SET = re.compile(r'''(?:os\.environ(?:\.setdefault)?\s*[\[(]\s*['"](ZKC_\w+)['"]\s*(?:\]\s*=[^=]|,)|monkeypatch\.setenv\(\s*['"](ZKC_\w+)['"])''')


def table():
    rows = ROW.findall(open(os.path.join(CSRC, 'zkc_switches.h')).read())
    assert len(rows) >= 45
    return rows


def is_switch(name):
    """a row of the table (ZKC_SMT_WAVE_MAX is one, whatever its prefix), or a name that neither exemption covers and so has to be one"""
    return name in {r[0] for r in table()} or not (OWN.match(name) or CONST.match(name))


def test_the_environment_is_read_in_the_header_only():
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
    assert len(files) >= 30
    assert [os.path.basename(p) for p in files if 'getenv' in open(p).read()] == ['zkc_switches.h']


def test_rows_are_unique_and_well_formed():
    rows = table()
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)) and all(n.startswith('ZKC_') for n in names)
    for name, kind, lo, hi, when in rows:
        assert kind in ('SET', 'OFF_IF_ZERO', 'ON_IF_ONE', 'NUMBER', 'NUMBER_LONG', 'NUMBER_U64', 'TEXT') and when in ('PROCESS', 'LIVE'), name
        if not kind.startswith('NUMBER'):
            assert (lo, hi) == ('ANY', 'ANY'), name


def test_every_switch_that_tests_tools_and_the_benchmark_name_is_a_row():
    names = {r[0] for r in table()}
    seen = set()
    cfg = open(os.path.join(ROOT, 'tests', 'test_00_gpu_switches.py')).read()
    cfg = cfg[cfg.index('CONFIGS = ['):cfg.index('def test_')]
    seen |= set(re.findall(r"'(ZKC_\w+)'\s*:", cfg))
    assert len(seen) >= 18
    for p in glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tests', 'host', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py')) + \
            [os.path.join(ROOT, 'bench.py')]:
        seen |= set(ENV_USE.findall(open(p).read()))
    seen = {n for n in seen if is_switch(n)}
    assert {'ZKC_NO_FOLD', 'ZKC_SERIAL_STREAMS', 'ZKC_DEVICE', 'ZKC_SMT_WAVE_MAX', 'ZKC_VERIFY_CHUNK', 'ZKC_TEST_FAIL_ALLOC'} <= seen      # the scan sees what it should
    assert seen - names == set()


def test_the_documented_list_is_the_table():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sec = doc[re.search(r'^## (\d+\. )?Switches', doc, re.M).start():]
    nxt = re.search(r'^## ', sec[3:], re.M)
    sec = sec[:3 + nxt.start()] if nxt else sec
    documented = [m.group(1) for m in re.finditer(r'^\|\s*`(ZKC_\w+)`', sec, re.M)]          # first column of the tables
    assert len(documented) == len(set(documented))
    assert set(documented) == {r[0] for r in table()}
    # the "read" column agrees with the row's read time: a LIVE row says at which event, a PROCESS row says process
    when = {r[0]: r[4] for r in table()}
    for line in sec.splitlines():
        m = re.match(r'^\|\s*`(ZKC_\w+)`', line)
        if m:
            cells = [c.strip() for c in line.strip().strip('|').split('|')]
            assert (cells[3] == 'process') == (when[m.group(1)] == 'PROCESS'), line


def test_switches_that_are_set_inside_a_running_process_are_live():
    """Whatever a test, a tool or bench.py assigns in os.environ of its own process is read by a library that may already have been used there: such a row must be LIVE.
    (tests/test_00_gpu_switches.py hands its CONFIGS to child processes instead, because most of those are PROCESS rows.)"""
    when = {r[0]: r[4] for r in table()}
    assigned = set()
    for p in glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py')) + [os.path.join(ROOT, 'bench.py')]:
        assigned |= {n for pair in ENV_SET.findall(open(p).read()) for n in pair if n and is_switch(n)}
    must = {'ZKC_NO_FOLD', 'ZKC_SERIAL_STREAMS', 'ZKC_BLIND_TREE', 'ZKC_INFLIGHT', 'ZKC_TEST_FAIL_ALLOC', 'ZKC_TEST_FAIL_KEY_LOADS', 'ZKC_SERVICE_KEYS', 'ZKC_SERVICE_SPILL',
            'ZKC_VERIFY_BATCH_GPU', 'ZKC_VERIFY_CHUNK', 'ZKC_SMT_WAVE_MAX'}
    assert must <= assigned, must - assigned
    assert {n: when[n] for n in assigned if when[n] != 'LIVE'} == {}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('switches') / 'switches_host')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           os.path.join(ROOT, 'tests', 'host', 'switches_host.cc'), '-o', exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and 'asan' in (b.stderr or '').lower() and 'cannot find' in b.stderr:
        pytest.skip('no sanitizer runtime for g++ on this box')
    assert b.returncode == 0, b.stderr[-3000:]

    def run(mode, **env):
        e = {k: v for k, v in os.environ.items() if not k.startswith('ZKC_')}
        e.update(env)
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60, env=e)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        return r.stdout.splitlines()
    return run


VALUES = ['unset', 'empty', '0', '1', '2', 'abc', '-5', '100000']
# per switch: the accessor and what the reading site computed for VALUES before the table existed (e = the variable's text or NULL; atoi("") = atoi("abc") = 0)
LIVE = {
    'ZKC_NO_FOLD': ('on', [0, 1, 1, 1, 1, 1, 1, 1]),                                          # getenv(..) != nullptr: =0 switches it on too
    'ZKC_BLIND_TREE': ('on', [1, 0, 0, 1, 1, 0, 1, 1]),                                       # !(e && atoi(e) == 0)
    'ZKC_DEVICE_BLOCKING_SYNC': ('on', [0, 0, 0, 1, 0, 0, 0, 0]),                             # e && atoi(e) == 1
    'ZKC_INFLIGHT': ('given', [None, 1, 1, 1, 2, 1, 1, 128]),                                 # e ? max(1, min(atoi(e), MSM_MAX_JOBS / 4 = 128)) : ...
    'ZKC_C_DEEP': ('given', [None, 13, 13, 13, 13, 13, 13, 17]),                              # e ? max(13, min(atoi(e), MSM_C_BIG = 17)) : ...
    'ZKC_SERVICE_BUSY_WAIT_US': ('given', [None, 0, 0, 1, 2, 0, 0, 100000]),                  # if (e) .. = max(0, atoi(e))
    'ZKC_TEST_FAIL_ALLOC': ('given', [None, 0, 0, 1, 2, 0, -5, 100000]),                      # fail_at && inflight >= atoi(fail_at)
    'ZKC_VERIFY_BATCH_GPU': ('value', [-1, 0, 0, 1, 2, 0, -5, 100000]),                       # e ? atoi(e) : -1
    'ZKC_VERIFY_CHUNK': ('value', [16384, 2, 2, 2, 2, 2, 2, 16384]),                          # e ? min(16384, max(2, atoi(e))) : 16384
    'ZKC_SMT_WAVE_MAX': ('value', [64, 0, 0, 1, 2, 0, 2**64 - 5, 100000]),                    # e ? (size_t)strtoull(e, nullptr, 10) : 64
    'ZKC_DEVICE': ('text', ['(null)', '(empty)', '0', '1', '2', 'abc', '-5', '100000']),      # getenv(..) handed to the device-list parser as it is
}


def test_live_switches_parse_and_clamp_as_their_sites_did(host):
    kinds = {r[0]: (r[1], r[4]) for r in table()}
    assert [kinds[n] for n in ('ZKC_NO_FOLD', 'ZKC_BLIND_TREE', 'ZKC_DEVICE_BLOCKING_SYNC', 'ZKC_INFLIGHT', 'ZKC_SMT_WAVE_MAX', 'ZKC_DEVICE')] == \
        [('SET', 'LIVE'), ('OFF_IF_ZERO', 'LIVE'), ('ON_IF_ONE', 'LIVE'), ('NUMBER', 'LIVE'), ('NUMBER_U64', 'LIVE'), ('TEXT', 'LIVE')]      # one of each kind
    want = []
    for i, v in enumerate(VALUES):
        for name, (acc, exp) in LIVE.items():
            want.append('%s %s absent' % (name, v) if exp[i] is None else '%s %s %s %s' % (name, v, acc, exp[i]))
    want.append('ZKC_SMT_WAVE_MAX 2^64-1 value %d' % (2**64 - 1))                              # 64 bits wide, unsigned
    got = host('live')
    assert sorted(got) == sorted(want), [x for x in got if x not in want] + [x for x in want if x not in got]


@pytest.mark.parametrize('env, first', [
    # G2_LATE: getenv != nullptr; MATVEC_UNITS: !(e && atoi(e) == 0); REDUCE_STREAM: e && atoi(e) == 1; WITNESS_GROUP: e ? max(1, atoi(e)) : 8;
    # DEEP_WIRES: e ? (size_t)atol(e) : 16000; VW_BIG: e ? (uint32_t)atoi(e) : 0
    ({}, [0, 1, 0, 8, 16000, 0]),
    ({'ZKC_G2_LATE': '0', 'ZKC_MATVEC_UNITS': '0', 'ZKC_REDUCE_STREAM': '0', 'ZKC_WITNESS_GROUP': '0', 'ZKC_DEEP_WIRES': '0', 'ZKC_VW_BIG': '0'}, [1, 0, 0, 1, 0, 0]),
    ({'ZKC_G2_LATE': '', 'ZKC_MATVEC_UNITS': '', 'ZKC_REDUCE_STREAM': '', 'ZKC_WITNESS_GROUP': '', 'ZKC_DEEP_WIRES': '', 'ZKC_VW_BIG': ''}, [1, 0, 0, 1, 0, 0]),
    ({'ZKC_G2_LATE': '1', 'ZKC_MATVEC_UNITS': '1', 'ZKC_REDUCE_STREAM': '1', 'ZKC_WITNESS_GROUP': '1', 'ZKC_DEEP_WIRES': '1', 'ZKC_VW_BIG': '1'}, [1, 1, 1, 1, 1, 1]),
    ({'ZKC_G2_LATE': '2', 'ZKC_MATVEC_UNITS': '2', 'ZKC_REDUCE_STREAM': '2', 'ZKC_WITNESS_GROUP': '2', 'ZKC_DEEP_WIRES': '2', 'ZKC_VW_BIG': '2'}, [1, 1, 0, 2, 2, 2]),
    ({'ZKC_G2_LATE': 'abc', 'ZKC_MATVEC_UNITS': 'abc', 'ZKC_REDUCE_STREAM': 'abc', 'ZKC_WITNESS_GROUP': 'abc', 'ZKC_DEEP_WIRES': 'abc', 'ZKC_VW_BIG': 'abc'}, [1, 0, 0, 1, 0, 0]),
    ({'ZKC_G2_LATE': '-5', 'ZKC_MATVEC_UNITS': '-5', 'ZKC_REDUCE_STREAM': '-5', 'ZKC_WITNESS_GROUP': '-5', 'ZKC_DEEP_WIRES': '-5', 'ZKC_VW_BIG': '-5'},
     [1, 1, 0, 1, 2**64 - 5, 2**32 - 5]),
    ({'ZKC_WITNESS_GROUP': '100000', 'ZKC_DEEP_WIRES': '5000000000', 'ZKC_VW_BIG': '100000'}, [0, 1, 0, 100000, 5000000000, 100000]),      # no upper clamp on these; atol is 64 bits wide
])
def test_process_switches_parse_as_their_sites_did_and_cache_each_on_its_own(host, env, first):
    got = host('process', **env)
    names = ['ZKC_G2_LATE on', 'ZKC_MATVEC_UNITS on', 'ZKC_REDUCE_STREAM on', 'ZKC_WITNESS_GROUP value', 'ZKC_DEEP_WIRES value', 'ZKC_VW_BIG value']
    assert got[:6] == ['%s %d' % (n, v) for n, v in zip(names, first)]
    # the program then sets ZKC_WITNESS_GROUP=3, ZKC_G2_LATE=1 and ZKC_REDUCE_STREAM=1: a PROCESS switch keeps the value of its first read
    assert got[6:9] == ['again ZKC_WITNESS_GROUP value %d' % first[3], 'again ZKC_G2_LATE on %d' % first[0], 'again ZKC_REDUCE_STREAM on %d' % first[2]]
    # ... sets ZKC_NTT_RADIX=1 and ZKC_G2_ACC_HOLD=0, neither read before: they cache on their own, from their own first read (and =0 switches a SET switch on);
    # ZKC_NTT_RADIX removed again: still 1
    assert got[9:12] == ['late ZKC_NTT_RADIX value 1', 'late ZKC_G2_ACC_HOLD on 1', 'again ZKC_NTT_RADIX value 1']
    # a LIVE switch follows the environment: 5, 7, removed
    assert got[12:] == ['ZKC_INFLIGHT first given 5', 'ZKC_INFLIGHT second given 7', 'ZKC_INFLIGHT third absent']
