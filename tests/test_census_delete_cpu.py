"""Deletes, absence proofs and their batched check where no GPU is needed (zkc_tree_delete / zkc_tree_gen_absence_proof / zkc_tree_refs, csrc/zkc_tree.hip;
zkc_smt_check_absence, csrc/zkc_smt_check.hip): the new entry points are exported and declared, the two new ZKC_SMT_* verdicts carry their numbers, the Python
surface exists, and the argument checks come before any device work.  The four entry points are declared in include/zkcensus_delete.h, which
zkcensus.h includes at its end."""
import ctypes
import os
import re
import subprocess
from zkcensus_amd import _native

NEW_ENTRY_POINTS = ['zkc_tree_delete', 'zkc_tree_gen_absence_proof', 'zkc_tree_refs', 'zkc_smt_check_absence']
ZKC_ERR_BAD_ARG = 4
INCLUDE = os.path.join(os.path.dirname(_native.LIB_PATH), '..', 'include')


def test_new_entry_points_are_exported_and_declared():
    """The four entry points are exported and declared in include/zkcensus_delete.h, which zkcensus.h includes; the two new ZKC_SMT_* verdicts carry their numbers."""
    _native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    sub = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'zkcensus_delete.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(zkc_[a-z0-9_]+)\s*\(', sub))
    assert declared == set(NEW_ENTRY_POINTS)
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
    hdr = open(os.path.join(INCLUDE, 'zkcensus.h')).read()
    assert '#include "zkcensus_delete.h"' in hdr
    for code, value in [('ZKC_SMT_KEY_PRESENT', 4), ('ZKC_SMT_OFF_PATH', 5)]:
        assert '%s = %d' % (code, value) in hdr, code
    assert 'non-membership proofs are not made' not in hdr


def test_headers_compile_as_c99_in_either_order(tmp_path):
    """A C client may include either header first."""
    for first, second in [('zkcensus.h', 'zkcensus_delete.h'), ('zkcensus_delete.h', 'zkcensus.h')]:
        src = tmp_path / 'h.c'
        src.write_text('#include "%s"\n#include "%s"\nint main(void) { int (*f)(zkc_tree*, const void*, size_t, int32_t*) = zkc_tree_delete; return f == 0 '
                       '&& ZKC_SMT_OFF_PATH == 5; }\n' % (first, second))
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, str(src)])


def test_python_surface():
    from zkcensus_amd import census
    assert (census.SMT_KEY_PRESENT, census.SMT_OFF_PATH) == (4, 5)
    assert callable(census.check_absence)
    for name in ['delete', 'gen_absence_proof', 'refs', 'check_absence']:
        assert callable(getattr(census.CensusTree, name)), name


def test_refusals_come_before_any_device_work():
    """Without a GPU no tree or context can be made, so every case passes a null handle; tests/test_gpu_census_delete.py repeats the argument cases on real ones.
    Nothing is written on a refusal."""
    lib = _native.load()
    w = b'\0' * 32
    sib = lambda nl: b'\0' * 32 * (max(nl, 0) + 1)
    st = (ctypes.c_int32 * 1)(77)
    assert lib.zkc_tree_delete(None, w, 1, st) == ZKC_ERR_BAD_ARG
    assert lib.zkc_tree_delete(None, None, 0, None) == ZKC_ERR_BAD_ARG
    out = (ctypes.c_size_t * 2)(5, 6)
    assert lib.zkc_tree_refs(None, out) == ZKC_ERR_BAD_ARG
    assert list(out) == [5, 6]
    root = ctypes.create_string_buffer(32)
    buf = ctypes.create_string_buffer(32)
    o0 = (ctypes.c_int32 * 1)(77)
    assert lib.zkc_tree_gen_absence_proof(None, w, 1, root, None, None, buf, buf, o0, st) == ZKC_ERR_BAD_ARG
    old0 = (ctypes.c_int32 * 1)(0)
    assert lib.zkc_smt_check_absence(None, 160, 1, w, w, w, old0, sib(160), w, 0, st) == ZKC_ERR_BAD_ARG
    assert lib.zkc_smt_check_absence(None, 160, 0, None, None, None, None, None, None, 0, None) == ZKC_ERR_BAD_ARG
    for nl in (0, 254, -1):
        assert lib.zkc_smt_check_absence(None, nl, 1, w, w, w, old0, sib(nl), w, 0, st) == ZKC_ERR_BAD_ARG
    for k in range(7):
        args = [w, w, w, old0, sib(160), w, st]
        args[k] = None
        assert lib.zkc_smt_check_absence(None, 160, 1, *args[:6], 1, args[6]) == ZKC_ERR_BAD_ARG
    assert lib.zkc_smt_check_absence(None, 160, 1, w, w, w, (ctypes.c_int32 * 1)(2), sib(160), w, 0, st) == ZKC_ERR_BAD_ARG
    assert list(st) == [77] and list(o0) == [77]
