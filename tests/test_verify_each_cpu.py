"""The batch verifier with a verdict per proof where no GPU is needed (zkc_verify_batch_each / zkc_verify_each_stats, csrc/zkc_verify_batch.hip): the entry points are exported
and are what include/zkcensus_verify_each.h declares, zkcensus.h includes that header and still compiles as C, the Python surface exists, and the argument checks come
before any device work, with their text in zkc_verify_last_error()."""
import ctypes
import os
import re
import subprocess
import oracle_lib as ol
from zkcensus_amd import _native, groth16

NEW_ENTRY_POINTS = ['zkc_verify_batch_each', 'zkc_verify_each_stats']
ZKC_ERR_BAD_ARG = 4
INCLUDE = os.path.join(os.path.dirname(_native.LIB_PATH), '..', 'include')


def test_entry_points_are_exported_and_declared():
    _native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if ' T ' in line}
    sub = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, 'zkcensus_verify_each.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(zkc_[a-z0-9_]+)\s*\(', sub)) == set(NEW_ENTRY_POINTS)
    for name in NEW_ENTRY_POINTS:
        assert name in exported, name
    assert '#include "zkcensus_verify_each.h"' in open(os.path.join(INCLUDE, 'zkcensus.h')).read()


def test_header_compiles_as_c99(tmp_path):
    for first in ('zkcensus.h', 'zkcensus_verify_each.h'):
        src = tmp_path / 'h.c'
        src.write_text('#include "%s"\n#include "zkcensus.h"\n' % first +
                       'int main(void) { int (*f)(zkc_ctx*, const uint8_t*, int, const uint8_t*, const uint8_t*, int, const uint8_t*, int32_t*) = zkc_verify_batch_each;\n'
                       '  int (*g)(zkc_ctx*, uint64_t*) = zkc_verify_each_stats;\n'
                       '  return f == 0 && g == 0 && ZKC_PROOF_VALID == 0 && ZKC_PROOF_INVALID == 1 && ZKC_PROOF_MALFORMED == 2 && ZKC_PROOF_PUBLIC_RANGE == 3; }\n')
        subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-fsyntax-only', '-I' + INCLUDE, str(src)])


def test_python_surface():
    assert callable(groth16.verify_each) and callable(groth16.verify_each_stats)
    assert (groth16.PROOF_VALID, groth16.PROOF_INVALID, groth16.PROOF_MALFORMED, groth16.PROOF_PUBLIC_RANGE) == (0, 1, 2, 3)


def test_refusals_come_before_any_device_work():
    """No context can be made without a GPU, so a non-NULL context here is a pointer that must never be followed: the checks of the other arguments come first."""
    lib = _native.load()
    vk = ol.load_json('ref/verification_key.json'); pr = ol.load_json('ref/proof.json'); sig = ol.load_json('ref/signals.json')
    vkb, pubs, proof = ol.vk_bytes(vk), b''.join(ol.le32(x) for x in sig), ol.proof_bytes(pr)
    verdict = (ctypes.c_int32 * 1)(77)
    never = ctypes.c_void_p(8)
    for args in ((None, vkb, 8, pubs, proof, 1, None, verdict),          # ctx == NULL
                 (never, vkb, 8, pubs, proof, 1, None, None),            # verdict == NULL
                 (never, vkb, 8, pubs, proof, 0, None, verdict),         # N <= 0
                 (never, vkb, 8, pubs, proof, -3, None, verdict),
                 (never, None, 8, pubs, proof, 1, None, verdict),
                 (never, vkb, 8, None, proof, 1, None, verdict),
                 (never, vkb, 8, pubs, None, 1, None, verdict),
                 (never, vkb, -1, pubs, proof, 1, None, verdict)):
        assert lib.zkc_verify_batch_each(*args) == -ZKC_ERR_BAD_ARG, args[5:]
        assert b'zkc_verify_batch_each' in lib.zkc_verify_last_error()
        assert verdict[0] == 77
    out = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    assert lib.zkc_verify_each_stats(None, out) == ZKC_ERR_BAD_ARG and list(out) == [1, 2, 3, 4]


def test_verify_batch_refuses_under_its_own_name():
    """zkc_verify_batch and zkc_verify_batch_each share their first pass (csrc/zkc_verify_batch.hip); each keeps its own name in its texts.  The same never-followed context."""
    lib = _native.load()
    vk = ol.load_json('ref/verification_key.json'); pr = ol.load_json('ref/proof.json'); sig = ol.load_json('ref/signals.json')
    vkb, pubs, proof = ol.vk_bytes(vk), b''.join(ol.le32(x) for x in sig), ol.proof_bytes(pr)
    never = ctypes.c_void_p(8)
    for args in ((never, None, 8, pubs, proof, 1, None),                 # vk == NULL
                 (never, vkb, 8, None, proof, 1, None),                  # pubs == NULL
                 (never, vkb, 8, pubs, None, 1, None),                   # proofs == NULL
                 (never, vkb, 8, pubs, proof, 0, None),                  # N <= 0
                 (never, vkb, 8, pubs, proof, -3, None),
                 (never, vkb, -1, pubs, proof, 1, None)):                # nPublic < 0
        assert lib.zkc_verify_batch(*args) == -ZKC_ERR_BAD_ARG, args[2:6]
        text = lib.zkc_verify_last_error()
        assert b'zkc_verify_batch:' in text and b'zkc_verify_batch_each' not in text
