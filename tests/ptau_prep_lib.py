"""TEST INFRASTRUCTURE for `powersoftau prepare phase2` (include/zkcensus_ptau_prepare.h): the UNPREPARED image of known waste and the prepared image a preparer must write
from it, both from tests/ptau_lib.py's Python integers and the oracle / fixed-base engines -- never from the transform under test.

The expected image is ptau_lib's prepared file except for the top block of section 12 (size 2N = 2^(power+1)): ptau_lib knows tau and writes the true L_c(tau) there; a
preparer has only M_0 .. M_(2N-2) and writes the transform of (M_0 .. M_(2N-2), infinity), in the exponent

    L'_c = L_c(tau) - w_2N^c tau^(2N-1) / 2N.

intt() is the transform itself on Python integers, for the engine tests: (1/n) sum_i w^(-c i) k_i, in n log n steps (direct_intt is the n^2 definition it is held to)."""
import ptau_lib as pl

R = pl.R
PLAIN = (0x2f1c9a7e4b3d58601f7e6d5c4b3a29180716253443526170 % R, 0x51a7d3c9e2b4f60718293a4b5c6d7e8f9fa0b1c2d3e4f5061728394a5b6c7d % R, 0x7b2e4d6f8a1c3e507192b3d4f5a6c7e8091a2b3c4d5e6f70 % R)


def wastes(power):
    """name -> (tau, alpha, beta): plain; tau = 1; tau = r - 1; tau a primitive 2^power-th root (on the domain: most Lagrange points are infinity, the butterflies meet
    equal and opposite points); tau a primitive 2^(power+1)-th root (on the double domain only)"""
    _, a, b = PLAIN
    return {'plain': PLAIN, 'one': (1, a, b), 'minus-one': (R - 1, a, b), 'on-domain': (pow(pl.root_of_unity(power), 3, R), a, b),
            'on-double-domain': (pow(pl.root_of_unity(power + 1), 3 if power else 1, R), a, b)}


def top_block_exponents(power, tau):
    """[L'_c for c < 2N]: what the p = power + 1 block of section 12 holds in a file prepared from the monomial points alone"""
    n2 = 2 << power
    L = pl.lagrange_at(tau, power + 1)
    w = pl.root_of_unity(power + 1)
    t = pow(tau, n2 - 1, R) * pow(n2, -1, R) % R
    out, wc = [], 1
    for c in range(n2):
        out.append((L[c] - wc * t) % R); wc = wc * w % R
    return out


def points(ks, width=64, ctx=None):
    """[k G] in the file's Montgomery form, G1 (width 64) or G2 (128): the oracle, or the fixed-base engine when given a context"""
    if ctx is None:
        return b''.join((pl.g1_mont if width == 64 else pl.g2_mont)(k) for k in ks)
    return pl.to_mont(pl._points_gpu(ctx, width, [k % R for k in ks]))


_cache = {}


def images(power, waste, ctx=None):
    """(unprepared image, expected prepared image, section bodies of ptau_lib's own prepared file) for (power, (tau, alpha, beta)); computed once and shared"""
    key = (power, waste, ctx is not None)
    if key not in _cache:
        tau, alpha, beta = waste
        secs = pl.sections(power, tau, alpha, beta, ctx)
        unprepared = pl.assemble({i: secs[i] for i in range(1, 8)})
        exp = {i: bytes(b) for i, b in secs.items()}
        top = pl.block(power + 1)
        assert top.stop == len(secs[12])
        exp[12] = exp[12][:top.start] + points(top_block_exponents(power, tau), 64, ctx)
        _cache[key] = (unprepared, pl.assemble(exp), {i: bytes(b) for i, b in secs.items()})
    return _cache[key]


def monomial_image(power, waste, ctx):
    """the unprepared image alone, without the Lagrange exponents ptau_lib.sections also computes (the measurement tool's files: power 20)"""
    import struct
    tau, alpha, beta = waste
    N = 1 << power
    tp = [1] * (2 * N - 1)
    for i in range(1, 2 * N - 1):
        tp[i] = tp[i - 1] * tau % R
    secs = {1: struct.pack('<I', 32) + pl.Q.to_bytes(32, 'little') + struct.pack('<II', power, power), 7: struct.pack('<I', 0),
            2: points(tp, 64, ctx), 3: points(tp[:N], 128, ctx), 4: points([alpha * x % R for x in tp[:N]], 64, ctx), 5: points([beta * x % R for x in tp[:N]], 64, ctx),
            6: points([beta], 128, ctx)}
    return pl.assemble(secs)


def parse(img):
    """image -> (order of ids, id -> body)"""
    import struct
    order, body, p = [], {}, 12
    for _ in range(struct.unpack_from('<I', img, 8)[0]):
        i, sz = struct.unpack_from('<IQ', img, p)
        order.append(i); body[i] = img[p + 12:p + 12 + sz]; p += 12 + sz
    assert p == len(img)
    return order, body


def offsets(img):
    """id -> byte offset of the section's body in the image"""
    import struct
    off, p = {}, 12
    for _ in range(struct.unpack_from('<I', img, 8)[0]):
        i, sz = struct.unpack_from('<IQ', img, p)
        off[i] = p + 12; p += 12 + sz
    return off


# ---- the transform on integers ----
def direct_intt(ks, logn):
    n = 1 << logn; wi = pow(pl.root_of_unity(logn), -1, R); ninv = pow(n, -1, R)
    return [ninv * sum(pow(wi, c * i, R) * k for i, k in enumerate(ks)) % R for c in range(n)]


def intt(ks, logn):
    """(1/n) sum_i w^(-c i) k_i for c < n = 2^logn, natural order: recursive decimation in time on Python integers"""
    n = 1 << logn
    assert len(ks) == n
    wi = pow(pl.root_of_unity(logn), -1, R)

    def rec(v, w):
        if len(v) == 1:
            return v
        e, o = rec(v[0::2], w * w % R), rec(v[1::2], w * w % R)
        h = len(v) // 2; out = [0] * len(v); t = 1
        for k in range(h):
            x = t * o[k] % R
            out[k] = (e[k] + x) % R; out[k + h] = (e[k] - x) % R
            t = t * w % R
        return out
    ninv = pow(n, -1, R)
    return [x * ninv % R for x in rec([k % R for k in ks], wi)]
