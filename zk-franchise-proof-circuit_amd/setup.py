"""Key generation.  Test-only keys: r1cs.build() -> .r1cs -> zkc_setup_from_r1cs[_dev] -> .zkey + verification_key.json, the stand-in for `make compile`
(circuit/circuit-compiler.sh:80-136) whose outputs are missing blobs; their toxic waste comes from a seed.  Keys nobody holds the waste of: from_ptau(), `snarkjs
groth16 setup` from a public prepared powers-of-tau file (include/zkcensus_ptau.h), to be followed by phase2.contribute; prepare_ptau() and check_prepared() are
`snarkjs powersoftau prepare phase2` and the check of a prepared file against its own monomial sections (include/zkcensus_ptau_prepare.h); verify_ptau() checks that
the monomial sections themselves are the powers of one tau, the point checks of `snarkjs powersoftau verify` (include/zkcensus_ptau_verify.h)."""
import ctypes
import hashlib
import os
from . import _native, r1cs

DEFAULT_SEED = 0x5A4B43454E535553        # "ZKCENSUS" 
_HERE = os.path.dirname(os.path.abspath(__file__))
ARTIFACT_DIR = os.path.join(_HERE, 'build', 'artifacts')


def artifact_paths(nLevels=160, seed=DEFAULT_SEED, directory=None):
    d = directory or ARTIFACT_DIR
    stem = os.path.join(d, 'zkcensus_%d_%x' % (nLevels, seed))
    return stem + '.r1cs', stem + '.zkey', stem + '_vkey.json'


def _generator_stamp():
    """sha256 over the sources that decide the artifacts' bytes: a key written by an older generator is regenerated, never reused."""
    h = hashlib.sha256()
    for f in (os.path.join(_HERE, 'r1cs.py'), os.path.join(_HERE, 'csrc', 'zkc_setup.hip'), os.path.join(_HERE, 'csrc', 'zkc_setup_write.h'), os.path.join(_HERE, 'csrc', 'zkc_fixedbase.h'),
              os.path.join(_HERE, 'csrc', 'zkc_fixedbase_dev.hip')):
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def ensure_test_artifacts(nLevels=160, seed=DEFAULT_SEED, directory=None, force=False, ctx=None):
    """Returns (r1cs_path, zkey_path, vkey_json_path), generating them on first use and again whenever r1cs.py or the generator's sources changed since
    they were written (stamp file next to them).  With a Context the points of the key are computed on its GPU (zkc_setup_from_r1cs_dev); the bytes, the
    paths and the stamp are the same either way.  Where the time goes at nLevels 160 (tools/setup_bench.py, profiles/setup_device.json, one MI355X box): r1cs.build + write 1.8 s of Python; the host generator 0.55 s
    (0.36 s of it the points); the device generator 0.19 s (5 ms the points, the rest reading the file, the scalars, the tables and writing the outputs)."""
    r, z, v = artifact_paths(nLevels, seed, directory)
    stamp_path, stamp = z + '.stamp', _generator_stamp()
    fresh = os.path.exists(stamp_path) and open(stamp_path).read().strip() == stamp
    if not force and fresh and all(os.path.exists(p) for p in (r, z, v)):
        return r, z, v
    os.makedirs(os.path.dirname(r), exist_ok=True)
    _, cs = r1cs.build(nLevels)
    cs.write(r)
    err = ctypes.create_string_buffer(512)
    tmpz, tmpv = z + '.tmp%d' % os.getpid(), v + '.tmp%d' % os.getpid()
    if ctx is None:
        rc = _native.load().zkc_setup_from_r1cs(r.encode(), seed, tmpz.encode(), tmpv.encode(), err, 512)
    else:
        rc = ctx._lib.zkc_setup_from_r1cs_dev(ctx._h, r.encode(), seed, tmpz.encode(), tmpv.encode(), err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    os.replace(tmpz, z); os.replace(tmpv, v)
    with open(stamp_path + '.tmp%d' % os.getpid(), 'w') as fh:
        fh.write(stamp)
    os.replace(stamp_path + '.tmp%d' % os.getpid(), stamp_path)
    return r, z, v


def from_ptau(r1cs_path, ptau_path, zkey_path, vkey=None, ctx=None, verify=False):
    """`snarkjs groth16 setup r1cs ptau zkey`: the initial key (gamma = delta = 1, no contributions) of the circuit from a PREPARED powers-of-tau file, and unless `vkey`
    is None its verification_key.json.  With a Context the sums over the file's points run on its GPU, without one on host threads; the bytes are the same.  Raises
    ZkcError with the refusal's text for a file that does not parse, does not fit the circuit, holds a point off its curve or fails a sanity check; nothing is written then.
    verify=True: the whole file is checked first -- verify_ptau (its monomial sections are the powers of one tau), then check_prepared (its Lagrange sections are their
    transforms) -- and a file that fails either raises ZkcError (ZKC_ERR_FORMAT) with that check's reason.  The key's bytes do not depend on `verify`."""
    if verify:
        for res in (verify_ptau(ptau_path, ctx=ctx), check_prepared(ptau_path, ctx=ctx)):
            if not res[0]:
                raise _native.ZkcError(5, res[-1])
    err = ctypes.create_string_buffer(512)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_setup_from_ptau(None if ctx is None else ctx._h, os.fsencode(r1cs_path), os.fsencode(ptau_path), os.fsencode(zkey_path),
                                 None if vkey is None else os.fsencode(vkey), err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    return zkey_path, vkey


def ptau_stats():
    """Milliseconds of the calling thread's last from_ptau (or phase2.verify_circuit), by stage."""
    ms = (ctypes.c_double * 6)()
    _native.load().zkc_setup_ptau_stats(ms)
    return dict(zip(['read_parse', 'transpose', 'upload', 'scale', 'accumulate_reduce', 'checks_write'], list(ms)))


def prepare_ptau(src, dst, ctx=None):
    """`snarkjs powersoftau prepare phase2 src dst`: dst = src's sections as they are, then the Lagrange sections 12 .. 15 (include/zkcensus_ptau_prepare.h, which also says
    what the top block of section 12 holds).  With a Context the transforms over the file's points run on its GPU, without one on host threads; the bytes are the same.
    Raises ZkcError with the refusal's text for a file that does not parse, is already prepared, holds a bad point or does not fit the device; nothing is left at dst then."""
    err = ctypes.create_string_buffer(512)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_ptau_prepare(None if ctx is None else ctx._h, os.fsencode(src), os.fsencode(dst), err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    return dst


def check_prepared(ptau, ctx=None):
    """Are sections 12 .. 15 of a prepared file the transforms of its sections 2 .. 5?  -> (ok, section, index, reason): the first point that differs, in the order 12, 13,
    14, 15 and then by index in the section (0, 0, '' when ok).  Raises ZkcError for a file that does not parse, is not prepared or holds a bad monomial point."""
    err = ctypes.create_string_buffer(512)
    sec, idx = ctypes.c_uint32(0), ctypes.c_uint64(0)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_ptau_check_prepared(None if ctx is None else ctx._h, os.fsencode(ptau), ctypes.byref(sec), ctypes.byref(idx), err, 512)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return rc == 1, sec.value, idx.value, err.value.decode()


PTAU_CHECKS = ('', 'POINT', 'G2_SUBGROUP', 'GENERATORS', 'TAU_G1_G2', 'TAU_G1', 'TAU_G2', 'ALPHA_TAU_G1', 'BETA_TAU_G1', 'BETA_G1_G2')      # ZKC_PTAU_CHECK_*, by id


def verify_ptau(ptau, ctx=None, seed=None):
    """Are sections 2 .. 6 of a powers-of-tau file (prepared or not) tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1 and beta G2 for ONE tau, alpha and beta?  The point
    checks of `snarkjs powersoftau verify` (include/zkcensus_ptau_verify.h says which, and in what order); with check_prepared on top, all of it but the contribution
    transcript.  -> (ok, check, section, index, reason): the first failing check as its ZKC_PTAU_CHECK_* id (0 when ok; PTAU_CHECKS[id] is its name), and the point to blame where there is one.
    With a Context the weighted sums run on its GPU, without one on host threads; verdict and sums are the same.  seed: 32 bytes make the weights reproducible (tests);
    None draws them from the OS, which is what a verifier wants.  Raises ZkcError for a file that does not parse."""
    err = ctypes.create_string_buffer(512)
    chk, sec, idx = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_ptau_verify(None if ctx is None else ctx._h, os.fsencode(ptau), None if seed is None else bytes(seed), ctypes.byref(chk), ctypes.byref(sec), ctypes.byref(idx), err, 512)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return rc == 1, chk.value, sec.value, idx.value, err.value.decode()


def debug_verify_ptau(ptau, weights16, ctx=None, chunk_terms=0):
    """Test hook (zkc_debug_ptau_verify): verify_ptau with the caller's weights (2N - 2 of 16 little-endian bytes) and chunk size (0: the default).
    -> (verify_ptau's tuple, the eight sums R1 R2 | S1 S2 | A pair | B pair as 640 bytes in standard form, all zero where a sum is infinity or was not reached)."""
    err = ctypes.create_string_buffer(512); sums = ctypes.create_string_buffer(640)
    chk, sec, idx = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    lib = _native.load() if ctx is None else ctx._lib
    w = bytes(weights16)
    rc = lib.zkc_debug_ptau_verify(None if ctx is None else ctx._h, os.fsencode(ptau), w, len(w) // 16, chunk_terms, sums, ctypes.byref(chk), ctypes.byref(sec), ctypes.byref(idx), err, 512)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return (rc == 1, chk.value, sec.value, idx.value, err.value.decode()), sums.raw


def ptau_verify_stats():
    """Milliseconds of the calling thread's last verify_ptau, by stage."""
    ms = (ctypes.c_double * 6)()
    _native.load().zkc_ptau_verify_stats(ms)
    return dict(zip(['read', 'upload_check', 'g2_membership', 'sums_g1', 'sums_g2', 'pairings'], list(ms)))


def ptau_prepare_stats():
    """Milliseconds of the calling thread's last prepare_ptau or check_prepared, by stage."""
    ms = (ctypes.c_double * 6)()
    _native.load().zkc_ptau_prepare_stats(ms)
    return dict(zip(['read', 'upload_check', 'transforms_g1', 'transforms_g2', 'affine_download', 'write_or_compare'], list(ms)))
