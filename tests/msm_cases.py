"""Scalar sets for the MSM sections of a key (zkc_msm_debug), shared by tests/test_gpu_prover.py and tests/test_00_gpu_msm_forms.py (with its child
tests/host/msm_forms_child.py): a mix with a heavy bucket, and sets that put equal and opposite points into one bucket.  No GPU: the oracle's
zkey_parse and plain Python; edge_key alone calls the library's host-side key generator, once per directory."""
import collections, ctypes
import oracle_lib as ol

R = ol.R
SECTIONS = {0: ('pointsA', 64), 1: ('pointsB1', 64), 2: ('pointsB2', 128)}        # which -> (field of oracle_lib.ZKey, bytes per point); each holds nVars points


def section_points(z, which, cnt):
    """(raw, std): section `which` of the parsed key z as the .zkey stores it (Montgomery words) and in standard form, the oracle's MSM input"""
    name, psz = SECTIONS[which]
    raw = ctypes.string_at(getattr(z, name), cnt * psz)
    q, qinv = ol.Q, pow(1 << 256, -1, ol.Q)
    std = b''.join((int.from_bytes(raw[32 * i:32 * i + 32], 'little') * qinv % q).to_bytes(32, 'little') for i in range(len(raw) // 32))
    return raw, std


def scalar_bytes(cnt, vals):
    """vals: {wire: scalar}; every other wire is 0"""
    sc = [0] * cnt
    for k, v in vals.items(): sc[k] = v
    return b''.join(x.to_bytes(32, 'little') for x in sc)


def heavy_mix(cnt, rng):
    """random field elements, witness-like small values, zeros, r - 1, and 600 wires with scalar 1: a heavy bucket, which the merge kernel sums"""
    sc = [rng.randrange(R) for _ in range(cnt)]
    for i in range(0, cnt, 7): sc[i] = rng.choice([0, 1, 2, R - 1, (1 << 128) - 1])
    for i in range(cnt // 2, cnt // 2 + 600): sc[i % cnt] = 1          # a heavy bucket
    return b''.join(x.to_bytes(32, 'little') for x in sc)


def largest_duplicate_group(raw, psz, cnt):
    """the wires of the largest group of identical finite points of a section (same polynomial in the key)"""
    groups = collections.defaultdict(list)
    for i in range(cnt):
        pt = raw[psz * i:psz * i + psz]
        if any(pt): groups[pt].append(i)
    dup = max(groups.values(), key=len)
    assert len(dup) >= 3, 'test key lost its duplicated base points'
    return dup


def equal_opposite_cases(dup, cnt, rng):
    """Wires of `dup` share a base point, so equal digits put P and P into one bucket and opposite digits P and -P.  The pair (3, 2^13 - 3) gives the digits 3 and -3 in
    the lowest window for EVERY window width up to 13 bits (2^13 - 3 = -3 mod 2^c, a carry goes up): that covers the 8-bit lone-proof table and the 12- / 13-bit sections
    of the test key.  A wider section window would leave 2^13 - 3 a plain positive digit and quietly empty the opposite cases: move the power of two with it."""
    a, b, c = dup[:3]
    cases = [{a: 3, b: 3}, {a: 3, b: (1 << 13) - 3}, {a: 5, b: 5, c: 5}, {a: 7, b: R - 7}, {a: 1, b: 1, c: R - 1},
             {i: 9 for i in dup},                                         # a whole group in one bucket (doubling, then additions of 2P + P ...)
             {i: (9 if k % 2 else (1 << 13) - 9) for k, i in enumerate(dup)}]
    base = [rng.randrange(R) for _ in range(cnt)]
    cases.append(dict(enumerate(base)) | {i: base[dup[0]] for i in dup})   # random everywhere, the group shares one full-size scalar
    return cases


def form_cases(dup):
    """What the cases above leave open: P, -P and a third P in one bucket; and the whole group with the signs +, -, +, + by blocks of 32 wires.
    Which lane meets which pair depends on the order of the entries inside the bucket, and that is the sort's business (zkc_msm_sort.hip ranks entries with LDS
    atomics inside a tile of 1024 scalars, so only the order of tiles is fixed): nothing here relies on it.  In wire order a lane of the half-wave walk, which takes
    every 32nd entry, would set, cancel, set again and double, and a lane that walks 16 entries in a row would start with a doubling and meet P + (-P) where a segment
    straddles a block; in any other order the same 95 + 32 points still put equal and opposite pairs next to each other in most lanes, since the bucket holds nothing
    else.  Every result is compared with the oracle's sum, whatever branch produced it."""
    a, b, c = dup[:3]
    return [{a: 3, b: (1 << 13) - 3, c: 3},
            {i: ((1 << 13) - 9 if k // 32 == 1 else 9) for k, i in enumerate(dup)}]


# ---- tests/test_00_gpu_msm_forms.py and its child: the same sets on both sides, from the key alone ----
FORMS_NL = 10
FORMS_SECTIONS = (0, 2)                  # A in G1, B2 in G2


def forms_scalars(z, which):
    """(std points of the section, the scalar sets in the order the child runs them): the equal / opposite sets, the two above, the heavy-bucket mix"""
    import random
    cnt = z.nVars
    raw, std = section_points(z, which, cnt)
    dup = largest_duplicate_group(raw, SECTIONS[which][1], cnt)
    assert len(dup) > 96, 'the largest group of equal points no longer fills four blocks of 32 entries: form_cases has lost its point'
    sets = [scalar_bytes(cnt, v) for v in equal_opposite_cases(dup, cnt, random.Random(11)) + form_cases(dup)]
    return std, sets + [heavy_mix(cnt, random.Random(3))]


# ---- a generic key whose point sections hold bases with coordinates at the edges of the field (tests/edge_points.py) ----
EDGE_KEY = (5000, 3000, 8)               # constraints, wires, public signals of the random circuit: a 12-bit window, a G2 section of half a wave per bucket
EDGE_KEY_SEEDS = (3000, 68, 21)          # circuit, toxic waste, patch
EDGE_KEY_FILE = 'edge_points_3000.zkey'


def edge_key_dir(tmp_path_factory):
    """one directory per test session, so that every module (and every child) that wants the key shares one image"""
    d = tmp_path_factory.getbasetemp() / 'edge_key'
    d.mkdir(exist_ok=True)
    return d


def edge_key(directory):
    """The patched image: made on the host and written to `directory` on first use, read from there afterwards (the bytes are the same either way).  A random R1CS
    key of 3 000 wires, its sections A, B1, B2 and C overwritten with pool points by edge_points.patch_zkey -- the key loader takes a section's points as they are."""
    import os, pathlib
    import edge_points as ep
    path = os.path.join(str(directory), EDGE_KEY_FILE)
    if not os.path.exists(path):
        from test_generic_circuit import random_instance, setup_key
        r1, _ = random_instance(pathlib.Path(str(directory)), *EDGE_KEY, seed=EDGE_KEY_SEEDS[0])
        zk, _ = setup_key(r1, EDGE_KEY_SEEDS[1])
        img, _ = ep.patch_zkey(zk, ([e.point for e in ep.g1_pool()], [e.point for e in ep.g2_pool()]), EDGE_KEY_SEEDS[2])
        with open(path + '.tmp%d' % os.getpid(), 'wb') as fh:
            fh.write(img)
        os.replace(path + '.tmp%d' % os.getpid(), path)
    return open(path, 'rb').read()


def low_window(cnt, rng, c=12):
    """every scalar inside the lowest window: each addition then takes a window-0 table row, which is the key's own coordinates"""
    return b''.join(rng.randrange(1, 1 << c).to_bytes(32, 'little') for _ in range(cnt))


def edge_forms_scalars(z, which):
    """(std points of the section of the parsed edge key, its scalar sets in the order the child runs them): low window, uniform, heavy mix"""
    import random
    cnt = z.nVars
    _, std = section_points(z, which, cnt)
    rng = random.Random(40 + which)
    uniform = b''.join(rng.randrange(R).to_bytes(32, 'little') for _ in range(cnt))
    return std, [low_window(cnt, rng), uniform, heavy_mix(cnt, random.Random(5))]
