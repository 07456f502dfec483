"""Snapshots of a resident census tree where no GPU is needed (zkc_tree_snapshot / zkc_tree_snapshot_count, csrc/zkc_tree.hip): the two entry points are exported and
are exactly what include/zkcensus_snapshot.h declares, zkcensus.h includes that header, the three public headers compile as C99 in every include order, the Python
surface exists, and the argument checks refuse NULL handles and NULL outputs without writing anything."""
import ctypes
import itertools
import os
import re
import subprocess
from zkcensus_amd import _native

NEW_ENTRY_POINTS = ['zkc_tree_snapshot', 'zkc_tree_snapshot_count']
ZKC_ERR_BAD_ARG = 4
INCLUDE = os.path.join(os.path.dirname(_native.LIB_PATH), '..', 'include')


def test_entry_points_are_exported_and_declared():
    _native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    sub = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'zkcensus_snapshot.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(zkc_[a-z0-9_]+)\s*\(', sub)) == set(NEW_ENTRY_POINTS)
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
    hdr = open(os.path.join(INCLUDE, 'zkcensus.h')).read()
    assert '#include "zkcensus_snapshot.h"' in hdr
    # the older headers do not declare them: their own tests pin their exact sets of zkc_tree_* names
    for name in ('zkcensus.h', 'zkcensus_delete.h'):
        body = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, name)).read(), flags=re.S)
        assert not set(re.findall(r'\b(zkc_[a-z0-9_]+)\s*\(', body)) & set(NEW_ENTRY_POINTS), name


def test_headers_compile_as_c99_in_every_order(tmp_path):
    """A C client may include the three headers in any order."""
    for order in itertools.permutations(['zkcensus.h', 'zkcensus_delete.h', 'zkcensus_snapshot.h']):
        src = tmp_path / 'h.c'
        src.write_text(''.join('#include "%s"\n' % h for h in order) +
                       'int main(void) { int (*f)(zkc_tree*, zkc_tree**) = zkc_tree_snapshot; int (*g)(zkc_tree*, size_t*) = zkc_tree_snapshot_count;\n'
                       '  int (*d)(zkc_tree*, const void*, size_t, int32_t*) = zkc_tree_delete; return f == 0 && g == 0 && d == 0 && ZKC_SMT_OFF_PATH == 5; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, str(src)])


def test_python_surface():
    from zkcensus_amd import census
    for name in ['snapshot', 'snapshot_count', 'close', '__enter__', '__exit__']:
        assert callable(getattr(census.CensusTree, name)), name
    assert isinstance(census.CensusTree.is_snapshot, property)


def test_refusals_come_before_any_device_work():
    """Without a GPU no tree can be made, so every case passes a null handle or a null output; tests/test_gpu_census_snapshot.py repeats them on real trees.  Nothing
    is written on a refusal."""
    lib = _native.load()
    out = ctypes.c_void_p(12345)
    assert lib.zkc_tree_snapshot(None, ctypes.byref(out)) == ZKC_ERR_BAD_ARG
    assert out.value == 12345
    assert lib.zkc_tree_snapshot(None, None) == ZKC_ERR_BAD_ARG
    n = ctypes.c_size_t(777)
    assert lib.zkc_tree_snapshot_count(None, ctypes.byref(n)) == ZKC_ERR_BAD_ARG
    assert n.value == 777
    assert lib.zkc_tree_snapshot_count(None, None) == ZKC_ERR_BAD_ARG
