"""Key generation.  Test-only keys: r1cs.build() -> .r1cs -> zkc_setup_from_r1cs[_dev] -> .zkey + verification_key.json, the stand-in for `make compile`
(circuit/circuit-compiler.sh:80-136) whose outputs are missing blobs; their toxic waste comes from a seed.  Keys nobody holds the waste of: from_ptau(), `snarkjs
groth16 setup` from a public prepared powers-of-tau file (include/zkcensus_ptau.h), to be followed by phase2.contribute; prepare_ptau() and check_prepared() are
`snarkjs powersoftau prepare phase2` and the check of a prepared file against its own monomial sections (include/zkcensus_ptau_prepare.h); verify_ptau() checks that
the monomial sections themselves are the powers of one tau, the point checks of `snarkjs powersoftau verify` (include/zkcensus_ptau_verify.h); new_ptau(),
contribute_ptau(), ptau_contributions() and verify_ptau_contributions() are phase 1 itself, `snarkjs powersoftau new / contribute` and the transcript part of
`powersoftau verify` (include/zkcensus_ptau_contribute.h)."""
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


def new_ptau(path, power):
    """`snarkjs powersoftau new bn128 power path`: an unprepared file with tau = alpha = beta = 1 (every point its group's generator) and no contribution.  Host only."""
    err = ctypes.create_string_buffer(512)
    rc = _native.load().zkc_ptau_new(os.fsencode(path), power, err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    return path


def _secrets96(secrets):
    if secrets is None:
        return None
    b = b''.join(s.to_bytes(32, 'little') if isinstance(s, int) else bytes(s) for s in secrets)
    if len(b) != 96:
        raise ValueError('secrets: (tau, alpha, beta), three integers below r or three times 32 little-endian bytes')
    return b


def contribute_ptau(src, dst, ctx=None, secrets=None, name='', verify=False):
    """`snarkjs powersoftau contribute src dst`: dst = src with every point of sections 2 .. 6 multiplied by its power of the secrets (tau', alpha', beta'; None draws them
    from the OS and forgets them) and one more record in section 7 (include/zkcensus_ptau_contribute.h); returns the 64-byte contribution hash.  With a Context the products
    run on its GPU, without one on host threads; the bytes are the same.  The output holds sections 1 .. 7 only: a prepared input loses its Lagrange sections.
    verify=True runs verify_ptau on src first and raises ZkcError (ZKC_ERR_FORMAT) with its reason.  Raises ZkcError for a secret that is 0 or >= r, a file that does not
    parse or a bad point (the section and the smallest index in the text); nothing is left at dst then."""
    if verify:
        res = verify_ptau(src, ctx=ctx)
        if not res[0]:
            raise _native.ZkcError(5, res[-1])
    err = ctypes.create_string_buffer(512); h = ctypes.create_string_buffer(64)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_ptau_contribute(None if ctx is None else ctx._h, os.fsencode(src), os.fsencode(dst), _secrets96(secrets), name.encode() if name else None, h, err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    return h.raw


def debug_contribute_ptau(src, dst, ctx=None, secrets=None, name='', chunk_points=0, form=0):
    """Test hook (zkc_debug_ptau_contribute): contribute_ptau with the chunk size in points (0: the default) and the kernel form (0 shipped, 1 bit-serial)."""
    err = ctypes.create_string_buffer(512); h = ctypes.create_string_buffer(64)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_debug_ptau_contribute(None if ctx is None else ctx._h, os.fsencode(src), os.fsencode(dst), _secrets96(secrets), name.encode() if name else None, chunk_points, form,
                                       h, err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    return h.raw


PTAU_RECORD_FIXED = 1288        # five points (448), three proofs of knowledge (3 x 256), transcript (64), type, paramsLen


def ptau_contributions(path):
    """The records of section 7 as this library writes them -> a list of dicts: the five points after the contribution (tauG1, tauG2, alphaG1, betaG1, betaG2), the three
    proofs of knowledge (pok: tau, alpha, beta -> g1_s, g1_sx, g2_spx), transcript, type, name, and `raw`, the record's bytes.  Raises ZkcError (ZKC_ERR_FORMAT) for a
    count that does not fit the section, a truncated record, an unknown tag or type, or trailing bytes."""
    lib = _native.load()
    err = ctypes.create_string_buffer(512); n = ctypes.c_uint32(0); need = ctypes.c_size_t(0)
    rc = lib.zkc_ptau_contributions(os.fsencode(path), ctypes.byref(n), None, ctypes.byref(need), err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    buf = ctypes.create_string_buffer(max(need.value, 1))
    rc = lib.zkc_ptau_contributions(os.fsencode(path), ctypes.byref(n), buf, ctypes.byref(need), err, 512)
    if rc != 0:
        raise _native.ZkcError(rc, err.value.decode())
    raw, out, at = buf.raw[:need.value], [], 0
    for _ in range(n.value):
        r = raw[at:]
        plen = int.from_bytes(r[1284:1288], 'little')
        rec = {'tauG1': r[0:64], 'tauG2': r[64:192], 'alphaG1': r[192:256], 'betaG1': r[256:320], 'betaG2': r[320:448], 'pok': {}, 'transcript': r[1216:1280],
               'type': int.from_bytes(r[1280:1284], 'little'), 'name': '', 'raw': r[:PTAU_RECORD_FIXED + plen]}
        for i, key in enumerate(('tau', 'alpha', 'beta')):
            q = r[448 + 256 * i:448 + 256 * (i + 1)]
            rec['pok'][key] = {'g1_s': q[0:64], 'g1_sx': q[64:128], 'g2_spx': q[128:256]}
        if plen:
            rec['name'] = r[PTAU_RECORD_FIXED + 2:PTAU_RECORD_FIXED + 2 + r[PTAU_RECORD_FIXED + 1]].decode(errors='replace')
        out.append(rec); at += PTAU_RECORD_FIXED + plen
    return out


def verify_ptau_contributions(prev, next, ctx=None, seed=None):
    """The transcript part of `snarkjs powersoftau verify`, on top of verify_ptau: is `next` what `prev` becomes under the contributions its section 7 adds?  prev = None:
    the chain starts at the generators (a new_ptau file of next's power).  -> (ok, n_new, reason): the number of records after prev's and, when not ok, the first failing
    check by name (include/zkcensus_ptau_contribute.h lists them in order).  Raises ZkcError for a HIP failure."""
    err = ctypes.create_string_buffer(768); n_new = ctypes.c_uint32(0)
    lib = _native.load() if ctx is None else ctx._lib
    rc = lib.zkc_ptau_verify_contributions(None if ctx is None else ctx._h, None if prev is None else os.fsencode(prev), os.fsencode(next), None if seed is None else bytes(seed),
                                           ctypes.byref(n_new), err, 768)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return rc == 1, n_new.value, err.value.decode()


def ptau_contribute_stats():
    """Milliseconds of the calling thread's last contribute_ptau, by stage."""
    ms = (ctypes.c_double * 6)()
    _native.load().zkc_ptau_contribute_stats(ms)
    return dict(zip(['read', 'upload_scalars_check', 'scale_g1', 'scale_g2', 'affine_download', 'hashes_write'], list(ms)))
