"""The phase-2 ceremony of a Groth16 key on the GPU (include/zkcensus_phase2.h): `snarkjs zkey contribute` and the ceremony part of `snarkjs zkey verify`
(circuit/circuit-compiler.sh:112-131).  Thin ctypes wrappers; the .zkey images are bytes in and bytes out.

The key material a contribution writes and the record layout of section 10 are snarkjs'; the proof of knowledge is not (its G2 challenge is this library's own hash to
G2), so snarkjs' `zkey verify` does not accept a contribution made here and verify() does not accept one made by snarkjs.  A key from setup.ensure_test_artifacts stays
TEST ONLY after any number of contributions: its toxic waste is known.  A key from setup.from_ptau over a public powers-of-tau file, with at least one honest
contribution on top, is not: verify_circuit() is `snarkjs zkey verify circuit.r1cs pot.ptau key.zkey` for it."""
import ctypes
from . import _native

FIXED = 3 * 64 + 128 + 64 + 8        # the fixed part of a record: deltaAfter, g1_s, g1_sx (G1), g2_spx (G2), transcript, type, paramsLen


def blake2b512(data):
    out = ctypes.create_string_buffer(64)
    _native.load().zkc_blake2b512(bytes(data), len(data), out)
    return out.raw


def contributions(zkey_bytes):
    """Section 10 of a .zkey image -> (csHash, [record, ...]); host only.  A record is a dict: the raw points (Montgomery coordinates, as stored) deltaAfter, g1_s, g1_sx,
    g2_spx, then transcript, type (0 contribution, 1 beacon), name (bytes or None), iterExp and beaconHash (beacons), and raw = the record's own bytes."""
    L = _native.load()
    cs, n, ln, err = ctypes.create_string_buffer(64), ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.create_string_buffer(512)
    rc = L.zkc_zkey_contributions(zkey_bytes, len(zkey_bytes), cs, ctypes.byref(n), None, ctypes.byref(ln), err, 512)
    if rc:
        raise _native.ZkcError(rc, err.value.decode())
    buf = ctypes.create_string_buffer(max(1, ln.value))
    rc = L.zkc_zkey_contributions(zkey_bytes, len(zkey_bytes), cs, ctypes.byref(n), buf, ctypes.byref(ln), err, 512)
    if rc:
        raise _native.ZkcError(rc, err.value.decode())
    raw, out, p = buf.raw[:ln.value], [], 0
    for _ in range(n.value):                                 # the library has checked the framing: every length below is inside the buffer
        plen = int.from_bytes(raw[p + 388:p + 392], 'little')
        rec = {'deltaAfter': raw[p:p + 64], 'g1_s': raw[p + 64:p + 128], 'g1_sx': raw[p + 128:p + 192], 'g2_spx': raw[p + 192:p + 320], 'transcript': raw[p + 320:p + 384],
               'type': int.from_bytes(raw[p + 384:p + 388], 'little'), 'name': None, 'iterExp': None, 'beaconHash': None, 'raw': raw[p:p + FIXED + plen]}
        q, end = p + FIXED, p + FIXED + plen
        while q < end:
            tag = raw[q]
            if tag == 2:
                rec['iterExp'] = raw[q + 1]; q += 2
            else:
                rec['name' if tag == 1 else 'beaconHash'] = raw[q + 2:q + 2 + raw[q + 1]]; q += 2 + raw[q + 1]
        out.append(rec); p = end
    return cs.raw, out


def contribute(ctx, zkey_bytes, delta=None, name=''):
    """One contribution on top of zkey_bytes -> (new zkey bytes, contribution hash).  delta: the secret, an int in [1, r) or its 32 little-endian bytes; None draws it
    from the OS generator.  name: str or bytes, cut at 64 bytes."""
    db = None if delta is None else (delta.to_bytes(32, 'little') if isinstance(delta, int) else bytes(delta))
    nb = name.encode() if isinstance(name, str) else bytes(name)
    ln = ctypes.c_size_t(0)
    ctx._check(ctx._lib.zkc_zkey_contribute(ctx._h, zkey_bytes, len(zkey_bytes), db, nb, None, ctypes.byref(ln), None))
    out, h = ctypes.create_string_buffer(ln.value), ctypes.create_string_buffer(64)
    ctx._check(ctx._lib.zkc_zkey_contribute(ctx._h, zkey_bytes, len(zkey_bytes), db, nb, out, ctypes.byref(ln), h))
    return out.raw[:ln.value], h.raw


def verify(ctx, init, final, seed=None):
    """Is `final` an honest chain of contributions on top of `init`?  -> (ok, n_new, reason): reason names the first failing check ('' when ok).  seed: 32 bytes that make
    the weights of the batch check reproducible (tests); None draws them from the OS generator."""
    n, err = ctypes.c_uint32(0), ctypes.create_string_buffer(512)
    rc = ctx._lib.zkc_zkey_verify_contributions(ctx._h, init, len(init), final, len(final), None if seed is None else bytes(seed), ctypes.byref(n), err, 512)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return rc == 1, n.value, err.value.decode()


def verify_circuit(ctx, r1cs_path, ptau_path, final, seed=None):
    """`snarkjs zkey verify` in full: is `final` an honest chain of contributions on top of THE initial key of this circuit and this powers-of-tau file?  The initial key
    is derived on ctx's GPU (setup.from_ptau, into memory) and checked as verify() checks.  -> (ok, n_new, reason)."""
    import os
    n, err = ctypes.c_uint32(0), ctypes.create_string_buffer(512)
    rc = ctx._lib.zkc_zkey_verify_circuit(ctx._h, os.fsencode(r1cs_path), os.fsencode(ptau_path), final, len(final), None if seed is None else bytes(seed), ctypes.byref(n), err, 512)
    if rc < 0:
        raise _native.ZkcError(-rc, err.value.decode())
    return rc == 1, n.value, err.value.decode()


def stats():
    """Milliseconds of the calling thread's last contribute (parse, upload, scale kernel, to affine, download, hash and write) and verify (table loads, MSMs, pairings)."""
    ms = (ctypes.c_double * 9)()
    _native.load().zkc_phase2_stats(ms)
    k = ['parse', 'upload', 'scale_kernel', 'to_affine', 'download', 'hash_write', 'verify_table_load', 'verify_msm', 'verify_pairings']
    return dict(zip(k, list(ms)))
