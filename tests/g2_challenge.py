"""TEST INFRASTRUCTURE: the G2 challenge of the ceremonies restated with hashlib and Python integers -- the derivation of include/zkcensus_phase2.h /
csrc/zkc_phase2.hip (zkc_debug_phase2_challenge_g2), which phase 1 uses for its proofs of knowledge as well (include/zkcensus_ptau_contribute.h).  The square root here
is the norm method (sqrt of the norm in Fq, then of (a0 +- s) / 2), not the library's complex method: the choice between +-y is canonical, so the two must agree.
tests/test_phase2_cpu.py holds it against the library; tests/ptau_contrib_lib.py builds section-7 records on it."""
import hashlib, struct
import oracle_lib as ol
from g2_py import f2add, f2mul, f2sub, f2inv, g2_mul, TWIST_H

Q = ol.Q


def fq_sqrt(a):
    s = pow(a, (Q + 1) // 4, Q)
    return s if s * s % Q == a % Q else None


def f2_sqrt(a):
    a0, a1 = a
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None: return (s, 0)
        s = fq_sqrt(-a0 % Q)
        return (0, s)                                                               # (s u)^2 = -s^2 = a0
    n = fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None: return None
    half = pow(2, -1, Q)
    for t in ((a0 + n) * half % Q, (a0 - n) * half % Q):
        y0 = fq_sqrt(t)
        if y0 is not None and y0 != 0:
            y = (y0, a1 * pow(2 * y0, -1, Q) % Q)
            if f2mul(y, y) == (a0 % Q, a1 % Q): return y
    return None


def challenge_py(transcript):
    b2 = f2mul((3, 0), f2inv((9, 1)))
    ctr = 0
    while True:
        stream = b''.join(hashlib.sha256(transcript + struct.pack('<I', ctr) + bytes([j])).digest() for j in range(4))
        ctr += 1
        c0, c1 = (int.from_bytes(stream[32 * w:32 * w + 32], 'big') & ((1 << 254) - 1) for w in range(2))
        if c0 >= Q or c1 >= Q: continue
        x = (c0, c1)
        y = f2_sqrt(f2add(f2mul(f2mul(x, x), x), b2))
        if y is None: continue
        ny = f2sub((0, 0), y)
        small, large = sorted([y, ny], key=lambda v: (v[1], v[0]))
        p = g2_mul((x, large if stream[127] & 1 else small), TWIST_H)
        if p is not None: return p
