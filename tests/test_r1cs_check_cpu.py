"""The witness checker's host side where no GPU is needed (include/zkcensus_r1cs.h, csrc/zkc_r1cs_parse.h): the entry points are exported, zkc_r1cs_header_info reads the
census circuit's header, every truncation and corruption the reader names is ZKC_ERR_FORMAT with its text -- through zkc_r1cs_header_info for what the header decides and
through the host-only key generator, the reader's other consumer, for what the constraint walk decides -- and the order of the sections does not matter."""
import ctypes, struct
import pytest
from zkcensus_amd import r1cs, _native

ZKC_ERR_BAD_ARG, ZKC_ERR_FORMAT = 4, 5
NEW_ENTRY_POINTS = ['zkc_r1cs_check', 'zkc_r1cs_check_dev', 'zkc_r1cs_check_stats', 'zkc_r1cs_free', 'zkc_r1cs_header_info', 'zkc_r1cs_info', 'zkc_r1cs_load']


@pytest.fixture(scope='module')
def census10(tmp_path_factory):
    L, cs = r1cs.build(10)
    path = str(tmp_path_factory.mktemp('r1cs') / 'census10.r1cs')
    cs.write(path)
    return L, cs, open(path, 'rb').read()


def sections(img):
    """[(id, offset of the section's 12-byte header, payload size)]"""
    out, p = [], 12
    for _ in range(struct.unpack_from('<I', img, 8)[0]):
        sid, sz = struct.unpack_from('<IQ', img, p)
        out.append((sid, p, sz)); p += 12 + sz
    return out


def reorder(img, order):
    parts = {sid: img[p:p + 12 + sz] for sid, p, sz in sections(img)}
    return img[:12] + b''.join(parts[s] for s in order)


def header_info(img):
    lib = _native.load()
    a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib.zkc_r1cs_header_info(img, len(img), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return rc, (a.value, b.value, c.value), (lib.zkc_last_error(None) or b'').decode()


def setup_rc(tmp_path, img, name='x'):
    """the host-only consumer of the whole reader: (rc, text, zkey bytes or None)"""
    lib = _native.load()
    p, z = tmp_path / (name + '.r1cs'), tmp_path / (name + '.zkey')
    p.write_bytes(img)
    err = ctypes.create_string_buffer(256)
    rc = lib.zkc_setup_from_r1cs(str(p).encode(), 7, str(z).encode(), None, err, 256)
    return rc, err.value.decode(), z.read_bytes() if rc == 0 else None


def test_entry_points_are_declared_and_exported():
    lib = _native.load()
    assert _native.declared_symbols('zkcensus_r1cs.h') == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
    hdr = open(_native.LIB_PATH.replace('zk-franchise-proof-circuit_amd/libzkcensus.so', 'include/zkcensus.h')).read()
    assert '#include "zkcensus_r1cs.h"' in hdr
    assert (r1cs.SATISFIED, r1cs.WIRE_RANGE, r1cs.NOT_ONE) == (-1, -2, -3)


def test_header_info_of_the_census_circuit(census10):
    L, cs, img = census10
    assert header_info(img)[:2] == (0, (L.nWires, 8, len(cs.cons))) and L.nWires == 8354
    assert r1cs.header_info(img) == (L.nWires, 8, len(cs.cons))
    lib = _native.load()
    assert lib.zkc_r1cs_header_info(img, len(img), None, None, None) == 0
    assert lib.zkc_r1cs_header_info(None, 0, None, None, None) == ZKC_ERR_BAD_ARG


def test_load_without_a_context_is_a_bad_argument(census10):
    lib = _native.load()
    h = ctypes.c_void_p()
    assert lib.zkc_r1cs_load(None, census10[2], len(census10[2]), ctypes.byref(h)) == ZKC_ERR_BAD_ARG and not h.value
    first = (ctypes.c_int64 * 1)()
    assert lib.zkc_r1cs_check(None, b'\0' * 32, 1, 1, first, None) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check_dev(None, None, 1, 1, first, None) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_info(None, None, None, None) == ZKC_ERR_BAD_ARG
    assert lib.zkc_r1cs_check_stats(None, (ctypes.c_double * 3)()) == ZKC_ERR_BAD_ARG
    lib.zkc_r1cs_free(None)


def small_system():
    """4 wires, 1 public: a . 1 = out ; (a + b) . (a + b) = c"""
    cs = r1cs.R1CS(5, 1)
    cs.add({2: 1}, {0: 1}, {1: 1}); cs.add({2: 1, 3: 1}, {2: 1, 3: 1}, {4: 1})
    return cs


def test_header_corruptions_are_format_errors(census10, tmp_path):
    L, cs, img = census10
    (_, p1, _), (_, p2, _), _ = sections(img)
    h = p1 + 12                                    # the header section's payload
    put = lambda at, b: img[:at] + b + img[at + len(b):]
    cases = {
        'bad magic': (b'r1cz' + img[4:], 'not an r1cs file'),
        'field size 16': (put(h, struct.pack('<I', 16)), 'bad r1cs header'),
        'wrong prime': (put(h + 4, bytes([img[h + 4] ^ 1])), 'r1cs prime is not BN254 r'),
        'nPub >= nWires': (put(h + 44, struct.pack('<I', L.nWires)), 'bad r1cs header'),
        'header section of 60 bytes': (put(p1 + 4, struct.pack('<Q', 60)), 'bad r1cs header'),
        'cut inside the section table': (img[:p1 + 5], 'r1cs sections truncated'),
        'cut before the header section': (img[:p1], 'r1cs sections truncated'),
        'cut inside the header section': (img[:h + 40], 'bad r1cs header'),
        'cut before the constraint section': (img[:p2], 'r1cs sections truncated'),
        'cut inside the second section entry': (img[:p2 + 7], 'r1cs sections truncated'),
        'empty': (b'', 'not an r1cs file'),
    }
    for name, (bad, text) in cases.items():
        rc, _, err = header_info(bad)
        assert (rc, err) == (ZKC_ERR_FORMAT, text), name
    for name in ('bad magic', 'wrong prime', 'nPub >= nWires'):          # ... and the same texts from the key generator, as before
        rc, err, _ = setup_rc(tmp_path, cases[name][0])
        assert (rc, err) == (ZKC_ERR_FORMAT, cases[name][1]), name


def test_constraint_corruptions_are_format_errors(census10, tmp_path):
    """what the constraint walk decides, through the reader's host-only consumer (zkc_r1cs_load reports the same on a GPU: tests/test_gpu_r1cs_check.py)"""
    L, cs, img = census10
    (_, p1, _), (_, p2, s2), (_, p3, _) = sections(img)
    body = p2 + 12
    first_term = body + 4                           # constraint 0, A: count, then (wire, coefficient)
    assert struct.unpack_from('<I', img, body)[0] >= 1
    cases = {
        'cut behind the constraint section header': img[:body],
        'cut in mid-constraint (inside a coefficient)': img[:first_term + 20],
        'cut in mid-constraint (between two rows)': img[:body + 4 + 36 * struct.unpack_from('<I', img, body)[0] + 2],
        'cut in the middle of the section': img[:body + s2 // 2],
        'cut one byte before the end of the section': img[:p3 - 1],
        'constraint count too large': img[:p1 + 12 + 60] + struct.pack('<I', len(cs.cons) + 1) + img[p1 + 12 + 64:],
    }
    for name, bad in cases.items():
        rc, err, _ = setup_rc(tmp_path, bad)
        assert (rc, err) == (ZKC_ERR_FORMAT, 'r1cs constraints truncated'), name
    bad = img[:first_term] + struct.pack('<I', L.nWires) + img[first_term + 4:]
    assert setup_rc(tmp_path, bad)[:2] == (ZKC_ERR_FORMAT, 'r1cs wire index out of range')
    ok = img[:first_term] + struct.pack('<I', L.nWires - 1) + img[first_term + 4:]
    assert header_info(ok)[0] == 0


def test_sections_in_any_order_and_unknown_sections(tmp_path):
    cs = small_system()
    p = tmp_path / 'small.r1cs'
    cs.write(str(p)); img = p.read_bytes()
    rc, err, key = setup_rc(tmp_path, img, 'a')
    assert rc == 0, err
    back = reorder(img, (3, 2, 1))
    assert back != img and header_info(back)[:2] == header_info(img)[:2] == (0, (5, 1, 2))
    assert setup_rc(tmp_path, back, 'b') == (0, '', key)
    # an unknown section id ahead of the others is skipped
    extra = img[:8] + struct.pack('<I', 4) + struct.pack('<IQ', 77, 5) + b'hello' + img[12:]
    assert header_info(extra)[:2] == (0, (5, 1, 2)) and setup_rc(tmp_path, extra, 'c') == (0, '', key)
    # a coefficient written as value + r means the value; a wire named twice contributes the sum of its coefficients
    def lc_bytes(items):
        return struct.pack('<I', len(items)) + b''.join(struct.pack('<I', w) + c.to_bytes(32, 'little') for w, c in items)
    body = lc_bytes([(2, 1 + r1cs.R)]) + lc_bytes([(0, 1)]) + lc_bytes([(1, 1)]) + lc_bytes([(2, 3), (3, 1), (2, r1cs.R - 2)]) + lc_bytes([(2, 1), (3, 1)]) + lc_bytes([(4, 1)])
    (_, p1, s1), (_, p2, s2), (_, p3, s3) = sections(img)
    odd = img[:p2] + struct.pack('<IQ', 2, len(body)) + body + img[p3:]
    rc, err, key2 = setup_rc(tmp_path, odd, 'd')
    assert rc == 0, err
    # the coefficient section lists terms as the file has them; every point of the key -- the polynomials at tau -- is the same
    pts = lambda z: [z[p + 12:p + 12 + sz] for sid, p, sz in sections(z) if sid != 4]
    assert pts(key2) == pts(key) and len(pts(key)) == 9
