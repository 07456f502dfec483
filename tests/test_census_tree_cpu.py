"""The resident census tree's C ABI (zkc_tree_*, csrc/zkc_tree.hip) where no GPU is needed: every entry point is exported and declared, and the
argument checks of zkc_tree_create come before any device work."""
import ctypes
import os
import subprocess
from zkcensus_amd import _native

TREE_ENTRY_POINTS = ['zkc_tree_create', 'zkc_tree_free', 'zkc_tree_add', 'zkc_tree_update', 'zkc_tree_root', 'zkc_tree_size', 'zkc_tree_get',
                     'zkc_tree_gen_proof', 'zkc_tree_census_inputs', 'zkc_tree_stats']
ZKC_ERR_BAD_ARG = 4


def test_tree_entry_points_are_exported_and_declared():
    _native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    declared = set(_native.declared_symbols())
    for name in TREE_ENTRY_POINTS:
        assert name in exported, name
        assert name in declared, name
    assert {s for s in declared if s.startswith('zkc_tree_')} == set(TREE_ENTRY_POINTS)
    hdr = open(os.path.join(os.path.dirname(_native.LIB_PATH), '..', 'include', 'zkcensus.h')).read()
    for code in ['ZKC_TREE_OK', 'ZKC_TREE_KEY_EXISTS', 'ZKC_TREE_KEY_ABSENT', 'ZKC_TREE_COLLISION', 'ZKC_TREE_NOT_BELOW_R', 'ZKC_TREE_NOT_IN_CENSUS',
                 'ZKC_TREE_NOT_IN_SIK', 'ZKC_TREE_SIK_MISMATCH']:
        assert code in hdr, code


def test_tree_create_refuses_bad_arguments_without_a_gpu():
    lib = _native.load()
    h = ctypes.c_void_p(12345)
    assert lib.zkc_tree_create(None, 160, ctypes.byref(h)) == ZKC_ERR_BAD_ARG
    assert h.value is None                                    # *out is cleared on failure
    assert lib.zkc_tree_create(None, 160, None) == ZKC_ERR_BAD_ARG
    for nl in (0, -1, 254, 1000):
        h = ctypes.c_void_p()
        assert lib.zkc_tree_create(None, nl, ctypes.byref(h)) == ZKC_ERR_BAD_ARG
        assert h.value is None
    # the other entry points refuse a null handle the same way, and zkc_tree_free(NULL) is a no-op
    st = (ctypes.c_int32 * 1)()
    assert lib.zkc_tree_add(None, b'\0' * 32, b'\0' * 32, 1, st) == ZKC_ERR_BAD_ARG
    assert lib.zkc_tree_update(None, b'\0' * 32, b'\0' * 32, 1, st) == ZKC_ERR_BAD_ARG
    assert lib.zkc_tree_root(None, ctypes.create_string_buffer(32)) == ZKC_ERR_BAD_ARG
    assert lib.zkc_tree_size(None, ctypes.byref(ctypes.c_size_t())) == ZKC_ERR_BAD_ARG
    assert lib.zkc_tree_census_inputs(None, None, 1, b'\0' * 64, b'\0' * 32, b'\0' * 32, b'\0' * 32, b'\0' * 32, b'\0' * 64, None, None, None, st) == ZKC_ERR_BAD_ARG
    lib.zkc_tree_free(None)
