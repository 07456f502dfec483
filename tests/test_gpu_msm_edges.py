"""GPU: the stand-alone G1 MSM (zkc_msm_g1_dev) at every window size and at the scalar and base values where a signed-digit Pippenger goes
wrong.  msm_c_for picks 12 / 13 / 15 / 16 / 17-bit windows by n: every threshold is taken from both sides, and n = 1, 2, 1023, 1025 and 4097
sit off the 1024-scalar tile of the bucketing.  Every size runs the same scalar kinds on ONE loaded handle, in an order that alternates
skewed and uniform digit distributions (stale segment or heavy-bucket state of one call must not leak into the next):

  zero (result: infinity), one non-zero scalar, all equal (one bucket per window, the heavy-bucket merge with the most segments), all r - 1,
  digits of exactly half and half + 1 in every window (the signed-digit carry chain), powers of two, the lowest window only, the top window
  only, uniform, and a random set whose exponent-space sum is zero.

The bases k_i G come from the GPU (sampled against the oracle's scalar multiplication) and hold a block of one repeated base (doublings inside
a bucket), a block of P / -P pairs (a bucket through infinity and on) and a few zero bases (infinity).  The reference is exact and GPU-free:
(sum s_i k_i mod r) G; for n <= 4096 also the oracle's MSM byte for byte.  Scalars are any 256-bit integers: r, 2r + 1, 2^255, 2^256 - 1 ...
give the result of their residue mod r (ffjavascript's multiExpAffine, which this replaces, takes integers).

The same scalar kinds also go through a generic key's own sections (zkc_msm_debug) at 12-, 13- and 15-bit windows, against the oracle's MSMs."""
import os
import random
import pytest
import oracle_lib as ol

pytestmark = pytest.mark.gpu
R = ol.R
G = (1).to_bytes(32, 'little') + (2).to_bytes(32, 'little')
FULL = os.environ.get('ZKC_TEST_FULL') == '1'


def c_for(n):                                       # csrc/zkc_prover.h msm_c_for
    return 12 if n < 12000 else 13 if n < 22000 else 15 if n < 90000 else 16 if n < 180000 else 17


def nw_for(c):                                      # csrc/zkc_pass_plan.h msm_nw
    return (254 + c) // c


# both sides of every window threshold, and sizes off the 1024-scalar tile
SIZES = [1, 2, 1023, 1025, 4097, 11999, 12000, 21999, 22000, 89999, 90000, 179999, 180000]
UNREDUCED = [R, R + 1, 2 * R + 1, 1 << 254, 1 << 255, (1 << 256) - 1]


def _dev(torch, b):
    import numpy as np
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope='module')
def gpu():
    import torch, zkcensus_amd
    ctx = zkcensus_amd.Context(0)
    yield ctx, torch
    ctx.close()


def _bases(ctx, torch, n, seed):
    """-> (ks, device bases): k_i G with a repeated block, a P / -P block and zero bases mixed into random ones"""
    from zkcensus_amd import engines
    rng = random.Random(seed)
    ks = [rng.randrange(1, R) for _ in range(n)]
    if n >= 8:
        rep = rng.randrange(1, R)
        for i in range(n // 8, n // 4): ks[i] = rep                                   # one base at many indices
        for i in range(n // 4, n // 4 + n // 8 - 1, 2): ks[i + 1] = R - ks[i]        # P, -P
        for i in range(n // 2, n // 2 + max(1, n // 64)): ks[i] = 0                   # infinity
    d_k = _dev(torch, b''.join(k.to_bytes(32, 'little') for k in ks))
    d_bases = torch.empty(64 * n, dtype=torch.uint8, device='cuda')
    engines.g1_mul_batch(ctx, G, d_k.data_ptr(), n, d_bases.data_ptr())
    for i in sorted({0, n // 2, n - 1, n // 8, n // 4 + 1}):
        if i < n:
            assert d_bases[64 * i:64 * i + 64].cpu().numpy().tobytes() == ol.g1_mul(G, ks[i]), 'k_i G, i = %d' % i
    return ks, d_bases


def _kinds(n, ks, rng, c=None):
    """(name, scalars) in an order that alternates skewed and uniform digit distributions (ks = None: no exponent-space kind)"""
    c = c or c_for(n); nw = nw_for(c); half = 1 << (c - 1)
    top = c * (nw - 1)                                                                # first bit of the top window
    hh = 0
    for w in range(nw): hh |= (half + (w & 1)) << (c * w)                             # digits half, half + 1, half, ...
    hh2 = 0
    for w in range(nw): hh2 |= (half + 1 - (w & 1)) << (c * w)
    mask253 = (1 << 253) - 1
    kinds = [('zero', [0] * n)]
    one = [0] * n; one[n // 3] = rng.randrange(1, R); kinds.append(('single', one))
    kinds.append(('equal', [rng.randrange(1, R)] * n))
    kinds.append(('uniform', [rng.randrange(R) for _ in range(n)]))
    kinds.append(('r-1', [R - 1] * n))
    kinds.append(('half', [(hh if i % 2 else hh2) & mask253 for i in range(n)]))
    kinds.append(('pow2', [1 << (i % 254) for i in range(n)]))
    kinds.append(('low-window', [rng.randrange(1, 1 << c) for _ in range(n)]))
    kinds.append(('top-window', [rng.randrange(1, ((R - 1) >> top) + 1) << top for _ in range(n)]))
    if n >= 2 and ks:                                                                 # sum s_i k_i = 0 mod r, every term non-zero
        j = max(i for i in range(n) if ks[i])
        ss = [rng.randrange(1, R) for _ in range(n)]
        ss[j] = 0
        ss[j] = -sum(s * k for s, k in zip(ss, ks)) * pow(ks[j], -1, R) % R
        kinds.append(('sum-zero', ss))
    kinds.append(('equal-again', [R - 2] * n))                                        # skewed right after uniform-like data, on the same handle
    return kinds


def _check(tbl, torch, ks, bases, ss, what, direct):
    scb = b''.join(s.to_bytes(32, 'little') for s in ss)
    got = tbl.multiExpAffine(_dev(torch, scb).data_ptr())
    t = sum(s * k for s, k in zip(ss, ks)) % R
    exp = ol.g1_mul(G, t) if t else bytes(64)
    assert got == exp, what
    if direct:
        red = b''.join((s % R).to_bytes(32, 'little') for s in ss)
        assert got == ol.msm_g1(bases, red), what + ' (oracle MSM)'


@pytest.mark.parametrize('n', SIZES, ids=lambda n: 'n%d-c%d' % (n, c_for(n)))
def test_msm_scalar_kinds(gpu, n):
    ctx, torch = gpu
    from zkcensus_amd import engines
    ks, d_bases = _bases(ctx, torch, n, 500 + n)
    bases = d_bases.cpu().numpy().tobytes()
    tbl = engines.G1Bases(ctx, d_bases.data_ptr(), n)
    try:
        rng = random.Random(n)
        for name, ss in _kinds(n, ks, rng):
            _check(tbl, torch, ks, bases, ss, '%s scalars, n = %d (c = %d)' % (name, n, c_for(n)), n <= 4096)
    finally:
        tbl.close()


@pytest.mark.parametrize('n', [1, 1025, 12000, 22000, 90000, 180000] + ([11999, 21999, 89999, 179999] if FULL else []),
                         ids=lambda n: 'n%d-c%d' % (n, c_for(n)))
def test_msm_unreduced_scalars(gpu, n):
    """scalars at or above r: each one alone at the top of the digit range, and all of them mixed into random scalars"""
    ctx, torch = gpu
    from zkcensus_amd import engines
    ks, d_bases = _bases(ctx, torch, n, 900 + n)
    bases = d_bases.cpu().numpy().tobytes()
    tbl = engines.G1Bases(ctx, d_bases.data_ptr(), n)
    try:
        rng = random.Random(7 * n)
        for u in UNREDUCED:
            _check(tbl, torch, ks, bases, [u] * n, 'all scalars %#x, n = %d (c = %d)' % (u, n, c_for(n)), n <= 4096)
        ss = [rng.randrange(R) for _ in range(n)]
        for i in range(0, n, 3): ss[i] = UNREDUCED[(i // 3) % len(UNREDUCED)]
        _check(tbl, torch, ks, bases, ss, 'unreduced scalars mixed in, n = %d (c = %d)' % (n, c_for(n)), n <= 4096)
    finally:
        tbl.close()


@pytest.mark.parametrize('n_cons,n_wires,n_pub', [(12000, 9000, 2), (28000, 20000, 1), (50000, 40000, 6)], ids=['c12', 'c13', 'c15'])
def test_section_msms_generic_keys(gpu, tmp_path, n_cons, n_wires, n_pub):
    """The key's own MSM sections (zkc_msm_debug: A, B1, C in G1, B2 in G2) at the window its wire count picks, with the scalar kinds above, against the
    oracle's MSMs.  Random R1CS keys whose wires sit in constraints (real bases, not infinity); the G2 section takes the one-wave-per-bucket form at
    c = 12 and 13 and the segment form at c = 15 (more than 8192 buckets)."""
    ctx, torch = gpu
    import ctypes, collections
    import zkcensus_amd
    from test_generic_circuit import random_instance, setup_key
    r1, _ = random_instance(tmp_path, n_cons, n_wires, n_pub, seed=n_wires)
    zk, _ = setup_key(r1, 60 + n_pub)
    z = ol.zkey_parse(zk)
    q, qinv = ol.Q, pow(1 << 256, -1, ol.Q)
    pk = zkcensus_amd.ProvingKey(ctx, zk)
    try:
        nv = pk.n_vars; c = c_for(nv)
        jobs = []
        for which, ptr, cnt, psz in ((0, z.pointsA, nv, 64), (1, z.pointsB1, nv, 64), (2, z.pointsB2, nv, 128), (3, z.pointsC, nv - n_pub - 1, 64)):
            raw = ctypes.string_at(ptr, cnt * psz)
            std = b''.join((int.from_bytes(raw[32 * i:32 * i + 32], 'little') * qinv % q).to_bytes(32, 'little') for i in range(len(raw) // 32))
            rng = random.Random(which * 7 + c)
            kinds = [(k, ss) for k, ss in _kinds(cnt, None, rng, c) if k in ('equal', 'uniform', 'r-1', 'half', 'top-window', 'zero')]
            groups = collections.defaultdict(list)                                    # bases the key holds more than once (infinity aside)
            for i in range(cnt):
                pt = raw[psz * i:psz * i + psz]
                if any(pt): groups[pt].append(i)
            dup = max(groups.values(), key=len)
            if len(dup) >= 2:
                ss = [rng.randrange(R) for _ in range(cnt)]
                for k, i in enumerate(dup): ss[i] = 9 if k % 2 else R - 9                # P + (-P) and 2P inside one bucket
                kinds.append(('duplicated bases', ss))
            for name, ss in kinds:
                scb = b''.join(x.to_bytes(32, 'little') for x in ss)
                got = pk.msm_debug(which, _dev(torch, scb).data_ptr(), cnt)
                jobs.append((which, name, std, scb, got))
        exps = ol.pmap(lambda j: ol.msm_g2(j[2], j[3]) if j[0] == 2 else ol.msm_g1(j[2], j[3]), jobs)
        for (which, name, _, _, got), exp in zip(jobs, exps):
            assert got == exp, 'section %d, %s scalars, %d wires (c = %d)' % (which, name, nv, c)
    finally:
        pk.close()
