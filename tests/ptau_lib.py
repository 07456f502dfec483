"""TEST INFRASTRUCTURE: WRITES a prepared powers-of-tau file (`.ptau`, the layout csrc/zkc_ptau_parse.h reads) from known waste (power, tau, alpha, beta).

Every scalar -- tau^i and the values L_c(tau) of the Lagrange bases of the domains of size 1, 2, .., 2^(power+1) -- is a Python integer; the points are scalar x
generator, from the CPU oracle (oracle_lib.g1_mul, and its one-term G2 MSM, which tests/test_gpu_fixed_mul.py pins against g2_py) or, given a Context, from the
fixed-base engines zkc_g1_fixed_mul_dev / zkc_g2_fixed_mul_dev.  The writer is Python and the reader is C++: they share no code, only the layout's description.

    "ptau" 1 nSections | per section id(u32) len(u64) body
    1: n8 = 32, q, power, ceremonyPower      2: tau^i G1, i < 2^(power+1) - 1     3: tau^i G2, i < 2^power     4: alpha tau^i G1     5: beta tau^i G1     6: beta G2
    7: contributions (none)                  12 .. 15: sections 2 .. 5 in Lagrange form: for p = 0 .. power the 2^p points L^(p)_c(tau) [x alpha, x beta] at point
                                             offset 2^p - 1; section 12 goes on to p = power + 1
Points are little-endian Montgomery coordinates (x 2^256 mod q), G2 as x.c0 x.c1 y.c0 y.c1, infinity all zero."""
import struct
import oracle_lib as ol

R, Q = ol.R, ol.Q
MONT = 1 << 256
G1_GEN = (1).to_bytes(32, 'little') + (2).to_bytes(32, 'little')
G2_GEN = b''.join(x.to_bytes(32, 'little') for x in (
    10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634,
    8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))
PT_BYTES = {2: 64, 3: 128, 4: 64, 5: 64, 6: 128, 12: 64, 13: 128, 14: 64, 15: 64}


def root_of_unity(logn):
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - logn):
        w = w * w % R
    return w


def lagrange_at(tau, logn):
    """[L_c(tau) for c < 2^logn] over the domain of the 2^logn-th roots of unity: Z(tau) w^c / (n (tau - w^c)); for tau ON the domain the indicator of its index"""
    n = 1 << logn; w = root_of_unity(logn)
    wp = [1] * n
    for c in range(1, n):
        wp[c] = wp[c - 1] * w % R
    if pow(tau, n, R) == 1:
        return [1 if x == tau % R else 0 for x in wp]
    den = [(tau - x) % R for x in wp]
    pre = [1] * n; acc = 1
    for c in range(n):
        pre[c] = acc; acc = acc * den[c] % R
    inv = pow(acc, -1, R); zn = (pow(tau, n, R) - 1) * pow(n, -1, R) % R; out = [0] * n
    for c in range(n - 1, -1, -1):
        out[c] = inv * pre[c] % R * wp[c] % R * zn % R
        inv = inv * den[c] % R
    return out


def section_scalars(power, tau, alpha, beta):
    """section id -> the exponents of its points (the generator's multiples), in file order"""
    N = 1 << power
    tp = [1] * (2 * N - 1)
    for i in range(1, 2 * N - 1):
        tp[i] = tp[i - 1] * tau % R
    lag = []
    for p in range(power + 2):
        lag.append(lagrange_at(tau, p))
    flat = [x for p in range(power + 1) for x in lag[p]]
    return {2: tp, 3: tp[:N], 4: [alpha * x % R for x in tp[:N]], 5: [beta * x % R for x in tp[:N]], 6: [beta % R],
            12: flat + lag[power + 1], 13: flat, 14: [alpha * x % R for x in flat], 15: [beta * x % R for x in flat]}


def to_mont(b):
    """points in standard form -> the file's Montgomery form; infinity (all zero) stays"""
    return b''.join((int.from_bytes(b[i:i + 32], 'little') * MONT % Q).to_bytes(32, 'little') for i in range(0, len(b), 32))


def _points_cpu(width, ks):
    if width == 64:
        return b''.join(ol.g1_mul(G1_GEN, k) if k else bytes(64) for k in ks)
    return b''.join(ol.msm_g2(G2_GEN, ol.le32(k)) if k else bytes(128) for k in ks)


def _points_gpu(ctx, width, ks):
    import numpy as np, torch
    from zkcensus_amd import engines
    d_k = torch.from_numpy(np.frombuffer(b''.join(k.to_bytes(32, 'little') for k in ks), dtype=np.uint8).copy()).cuda()
    d_o = torch.zeros(width * len(ks), dtype=torch.uint8, device='cuda')
    (engines.g1_fixed_mul if width == 64 else engines.g2_fixed_mul)(ctx, G1_GEN if width == 64 else G2_GEN, d_k.data_ptr(), len(ks), d_o.data_ptr())
    return d_o.cpu().numpy().tobytes()


def sections(power, tau, alpha, beta, ctx=None):
    """section id -> bytearray of its body (1 .. 7 and 12 .. 15): what write() puts into the file, for a test to change first"""
    sc = section_scalars(power, tau, alpha, beta)
    # one batch per group: the scalars of all sections back to back
    out = {1: bytearray(struct.pack('<I', 32) + Q.to_bytes(32, 'little') + struct.pack('<II', power, power)), 7: bytearray(struct.pack('<I', 0))}
    for width in (64, 128):
        ids = [i for i in sorted(sc) if PT_BYTES[i] == width]
        ks = [k for i in ids for k in sc[i]]
        raw = to_mont(_points_gpu(ctx, width, ks) if ctx is not None else _points_cpu(width, ks))
        at = 0
        for i in ids:
            out[i] = bytearray(raw[at:at + width * len(sc[i])]); at += width * len(sc[i])
    return out


def assemble(secs, order=None):
    ids = order or sorted(secs)
    return b'ptau' + struct.pack('<II', 1, len(ids)) + b''.join(struct.pack('<IQ', i, len(secs[i])) + bytes(secs[i]) for i in ids)


def write(path, power, tau, alpha, beta, ctx=None, change=None):
    """the prepared file of (power, tau, alpha, beta) at `path`.  change(secs): edits the section bodies (a dict id -> bytearray) before they are assembled"""
    secs = sections(power, tau, alpha, beta, ctx)
    if change:
        change(secs)
    with open(path, 'wb') as f:
        f.write(assemble(secs))
    return path


def block(logn, width=64):
    """the byte range of the size-2^logn Lagrange block inside a section 12 .. 15"""
    return slice(width * ((1 << logn) - 1), width * ((2 << logn) - 1))


# ---- circuits and expected keys ----
def write_r1cs(path, n_wires, n_pub, cons):
    """an iden3 .r1cs from cons = [(A, B, C)], each side a list of (wire, coefficient)"""
    pk = struct.pack
    side = lambda terms: pk('<I', len(terms)) + b''.join(pk('<I', w) + (c % (1 << 256)).to_bytes(32, 'little') for w, c in terms)
    body = b''.join(side(a) + side(b) + side(c) for a, b, c in cons)
    hdr = pk('<I', 32) + R.to_bytes(32, 'little') + pk('<IIIIQI', n_wires, 0, n_pub, n_wires - 1 - n_pub, n_wires, len(cons))
    with open(path, 'wb') as f:
        f.write(b'r1cs' + pk('<II', 1, 2))
        for sid, data in ((1, hdr), (2, body)):
            f.write(pk('<IQ', sid, len(data))); f.write(data)
    return path


def key_exponents(n_wires, n_pub, cons, tau, alpha, beta):
    """the key of include/zkcensus_ptau.h in the exponent: (logn, A, B, K, H), lists of integers mod r (B serves B1 and B2)"""
    logn = 0
    while (1 << logn) < len(cons) + n_pub + 1:
        logn += 1
    L = lagrange_at(tau, logn); L2n = lagrange_at(tau, logn + 1)
    A, B, C = [0] * n_wires, [0] * n_wires, [0] * n_wires
    for k, (ra, rb, rc) in enumerate(cons):
        for w, c in ra: A[w] = (A[w] + c * L[k]) % R
        for w, c in rb: B[w] = (B[w] + c * L[k]) % R
        for w, c in rc: C[w] = (C[w] + c * L[k]) % R
    for i in range(n_pub + 1):
        A[i] = (A[i] + L[len(cons) + i]) % R
    K = [(beta * a + alpha * b + c) % R for a, b, c in zip(A, B, C)]
    return logn, A, B, K, [L2n[2 * i + 1] for i in range(1 << logn)]


def zkey_sections(z):
    """id -> the bytes of a .zkey's section"""
    out, p = {}, 12
    for _ in range(struct.unpack_from('<I', z, 8)[0]):
        i, sz = struct.unpack_from('<IQ', z, p)
        out[i] = z[p + 12:p + 12 + sz]; p += 12 + sz
    return out


def g1_mont(k):
    return to_mont(ol.g1_mul(G1_GEN, k)) if k % R else bytes(64)


def g2_mont(k):
    return to_mont(ol.msm_g2(G2_GEN, ol.le32(k % R))) if k % R else bytes(128)
