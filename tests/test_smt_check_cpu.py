"""The census proof checker's C ABI (zkc_smt_check_proofs, csrc/zkc_smt_check.hip) where no GPU is needed: the entry point is exported and declared with its
ZKC_SMT_* verdicts, and its argument checks come before any device work."""
import ctypes
import os
import subprocess
from zkcensus_amd import _native

ZKC_OK, ZKC_ERR_BAD_ARG = 0, 4
HEADER = os.path.join(os.path.dirname(_native.LIB_PATH), '..', 'include', 'zkcensus.h')


def test_check_proofs_is_exported_and_declared():
    _native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    declared = set(_native.declared_symbols())
    for name in ['zkc_smt_check_proofs', 'zkc_smt_check_stats']:
        assert name in exported, name
        assert name in declared, name
    hdr = open(HEADER).read()
    for code, value in [('ZKC_SMT_VALID', 0), ('ZKC_SMT_ROOT_MISMATCH', 1), ('ZKC_SMT_NOT_BELOW_R', 2), ('ZKC_SMT_LAST_SIBLING', 3)]:
        assert '%s = %d' % (code, value) in hdr, code


def test_check_proofs_refuses_bad_arguments_without_a_gpu():
    """Without a GPU no context can be made, so every case here passes a null context; tests/test_gpu_smt_check.py repeats the nLevels and null-pointer cases on a
    real one.  The refusal comes before any device work and writes no verdict."""
    lib = _native.load()
    w = b'\0' * 32
    sib = lambda nl: b'\0' * 32 * (max(nl, 0) + 1)
    st = (ctypes.c_int32 * 1)(77)
    assert lib.zkc_smt_check_proofs(None, 160, 1, w, w, sib(160), w, 0, st) == ZKC_ERR_BAD_ARG
    assert lib.zkc_smt_check_proofs(None, 160, 0, None, None, None, None, 0, None) == ZKC_ERR_BAD_ARG
    for nl in (0, 254, -1):
        assert lib.zkc_smt_check_proofs(None, nl, 1, w, w, sib(nl), w, 0, st) == ZKC_ERR_BAD_ARG
    for k in range(5):
        args = [w, w, sib(160), w, st]
        args[k] = None
        assert lib.zkc_smt_check_proofs(None, 160, 1, *args[:4], 1, args[4]) == ZKC_ERR_BAD_ARG
    assert list(st) == [77]
    assert lib.zkc_smt_check_stats(None, (ctypes.c_double * 3)()) == ZKC_ERR_BAD_ARG
