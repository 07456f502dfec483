"""Key generation.  Test-only keys: r1cs.build() -> .r1cs -> zkc_setup_from_r1cs[_dev] -> .zkey + verification_key.json, the stand-in for `make compile`
(circuit/circuit-compiler.sh:80-136) whose outputs are missing blobs; their toxic waste comes from a seed.  Keys nobody holds the waste of: from_ptau(), `snarkjs
groth16 setup` from a public prepared powers-of-tau file (include/zkcensus_ptau.h), to be followed by phase2.contribute; prepare_ptau() and check_prepared() are
`snarkjs powersoftau prepare phase2` and the check of a prepared file against its own monomial sections (include/zkcensus_ptau_prepare.h)."""
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


def from_ptau(r1cs_path, ptau_path, zkey_path, vkey=None, ctx=None):
    """`snarkjs groth16 setup r1cs ptau zkey`: the initial key (gamma = delta = 1, no contributions) of the circuit from a PREPARED powers-of-tau file, and unless `vkey`
    is None its verification_key.json.  With a Context the sums over the file's points run on its GPU, without one on host threads; the bytes are the same.  Raises
    ZkcError with the refusal's text for a file that does not parse, does not fit the circuit, holds a point off its curve or fails a sanity check; nothing is written then."""
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


def ptau_prepare_stats():
    """Milliseconds of the calling thread's last prepare_ptau or check_prepared, by stage."""
    ms = (ctypes.c_double * 6)()
    _native.load().zkc_ptau_prepare_stats(ms)
    return dict(zip(['read', 'upload_check', 'transforms_g1', 'transforms_g2', 'affine_download', 'write_or_compare'], list(ms)))
