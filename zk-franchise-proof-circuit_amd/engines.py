"""The NTT and G1 MSM engines on their own -- the ffjavascript calls under snarkjs' groth16.prove (`Fr.fft`, `Fr.ifft`,
`G1.multiExpAffine`; ts_inputs/src/example.ts:358) over device buffers.  Thin ctypes wrappers of include/zkcensus.h
zkc_ntt_dev / zkc_g1_mul_batch_dev / zkc_msm_g1_*; used by SURVEY.md 8(d) config 5 (ii) (tools/stress.py) and its parity tests.
g1_fixed_mul / g2_fixed_mul (include/zkcensus_setup.h) are the windowed fixed-base batch products the device key generator is built from; g1_scale
(include/zkcensus_phase2.h) is the opposite shape, many points times one scalar, which a phase-2 contribution is made of; g1_lagrange / g2_lagrange
(include/zkcensus_ptau_prepare.h) are the inverse transform over points that prepares a powers-of-tau file; g1_scale_each / g2_scale_each
(include/zkcensus_ptau_contribute.h) are many points each times its own scalar, which a powers-of-tau contribution is made of."""
import ctypes

R_MONT = 1 << 256
G1_GENERATOR = (1).to_bytes(32, 'little') + (2).to_bytes(32, 'little')
G2_GENERATOR = b''.join(c.to_bytes(32, 'little') for c in (       # x.c0 | x.c1 | y.c0 | y.c1
    0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2,
    0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def fft(ctx, d_src_ptr, d_dst_ptr, logn, nvec=1):
    """Forward NTT of nvec vectors of 2^logn Montgomery-form Fr elements (natural order in and out); d_src != d_dst."""
    ctx._check(ctx._lib.zkc_ntt_dev(ctx._h, d_src_ptr, d_dst_ptr, logn, nvec, 0))


def ifft(ctx, d_src_ptr, d_dst_ptr, logn, nvec=1):
    ctx._check(ctx._lib.zkc_ntt_dev(ctx._h, d_src_ptr, d_dst_ptr, logn, nvec, 1))


def g1_mul_batch(ctx, base64, d_scalars_ptr, n, d_out_ptr):
    """d_out[i] = k_i * base; scalars 32 B standard form, points affine standard form (64 B)."""
    ctx._check(ctx._lib.zkc_g1_mul_batch_dev(ctx._h, bytes(base64), d_scalars_ptr, n, d_out_ptr))


def g1_fixed_mul(ctx, base64, d_scalars_ptr, n, d_out_ptr):
    """d_out[i] = k_i * base through a window table of the base: one mixed addition per non-zero byte of k_i.  Scalars 32 B standard form BELOW r,
    points affine standard form (64 B); the base must be on the curve."""
    ctx._check(ctx._lib.zkc_g1_fixed_mul_dev(ctx._h, bytes(base64), d_scalars_ptr, n, d_out_ptr))


def g2_fixed_mul(ctx, base128, d_scalars_ptr, n, d_out_ptr):
    """The same in G2: base and outputs 128 B (x.c0 | x.c1 | y.c0 | y.c1), the base on the twist."""
    ctx._check(ctx._lib.zkc_g2_fixed_mul_dev(ctx._h, bytes(base128), d_scalars_ptr, n, d_out_ptr))


def g1_scale(ctx, d_points_ptr, n, k, d_out_ptr, mont=False):
    """d_out[i] = k * d_points[i]: n affine points (64 B, all zero = infinity) times ONE scalar k (an int below r, or its 32 little-endian bytes); include/zkcensus_phase2.h.
    mont: the coordinates are in Montgomery form on both sides, as a .zkey stores them.  d_out may equal d_points.  A point off the curve raises (ZKC_ERR_FORMAT, the index in
    the text)."""
    kb = k.to_bytes(32, 'little') if isinstance(k, int) else bytes(k)
    ctx._check(ctx._lib.zkc_g1_scale_dev(ctx._h, d_points_ptr, n, kb, 1 if mont else 0, d_out_ptr))


def g1_scale_each(ctx, d_points_ptr, n, d_scalars_ptr, d_out_ptr, mont=False):
    """d_out[i] = k_i * d_points[i]: n affine points (64 B, all zero = infinity), each times its OWN scalar (n x 32 little-endian bytes on the device, standard form, below r;
    0 gives infinity); include/zkcensus_ptau_contribute.h.  mont: the coordinates are in Montgomery form on both sides, as a .ptau stores them.  d_out may equal d_points.
    A coordinate >= q, a point off the curve or a scalar >= r raises (ZKC_ERR_FORMAT, the smallest index in the text) and nothing is written."""
    ctx._check(ctx._lib.zkc_g1_scale_each_dev(ctx._h, d_points_ptr, n, d_scalars_ptr, 1 if mont else 0, d_out_ptr))


def g2_scale_each(ctx, d_points_ptr, n, d_scalars_ptr, d_out_ptr, mont=False):
    """The same in G2: points 128 B (x.c0 | x.c1 | y.c0 | y.c1), anywhere on the twist."""
    ctx._check(ctx._lib.zkc_g2_scale_each_dev(ctx._h, d_points_ptr, n, d_scalars_ptr, 1 if mont else 0, d_out_ptr))


def debug_scale_each(ctx, g2, d_points_ptr, n, d_scalars_ptr, d_out_ptr, mont=False, form=0):
    """Test hook (zkc_debug_scale_each_dev): g1_scale_each / g2_scale_each with the kernel form, 0 the shipped windowed form, 1 bit-serial double-and-add."""
    ctx._check(ctx._lib.zkc_debug_scale_each_dev(ctx._h, 1 if g2 else 0, d_points_ptr, n, d_scalars_ptr, 1 if mont else 0, d_out_ptr, form))


def debug_tau_scalars(ctx, tau, mult, first, n, d_out_ptr):
    """Test hook (zkc_debug_tau_scalars_dev): d_out[i] = mult * tau^(first + i) mod r for i < n, 32 bytes little endian each, made by the power table and the kernel a
    powers-of-tau contribution makes its scalars with.  tau, mult: integers in [1, r); first + n <= 2^32."""
    ctx._check(ctx._lib.zkc_debug_tau_scalars_dev(ctx._h, tau.to_bytes(32, 'little'), mult.to_bytes(32, 'little'), first, n, d_out_ptr))


def scale_each_stats():
    """Milliseconds of the calling thread's last g1_scale_each / g2_scale_each / debug_scale_each: the scale kernel (point checks included), the conversion to affine."""
    from . import _native
    ms = (ctypes.c_double * 2)()
    _native.load().zkc_debug_scale_each_stats(ms)
    return {'scale_kernel': ms[0], 'affine': ms[1]}


def g1_lagrange(ctx, d_points_ptr, logn, d_out_ptr, mont=False):
    """d_out[c] = 1/n sum_i w^(-c i) d_points[i] for n = 2^logn affine G1 points (64 B, all zero = infinity), natural order on both sides: monomial powers-of-tau points
    to the Lagrange basis of the size-n domain (include/zkcensus_ptau_prepare.h).  mont: Montgomery coordinates on both sides, as a .ptau stores them.  d_out may equal
    d_points.  A point off the curve raises (ZKC_ERR_FORMAT, the smallest index in the text) and nothing is written."""
    ctx._check(ctx._lib.zkc_g1_lagrange_dev(ctx._h, d_points_ptr, logn, 1 if mont else 0, d_out_ptr))


def g2_lagrange(ctx, d_points_ptr, logn, d_out_ptr, mont=False):
    """The same in G2: points 128 B (x.c0 | x.c1 | y.c0 | y.c1)."""
    ctx._check(ctx._lib.zkc_g2_lagrange_dev(ctx._h, d_points_ptr, logn, 1 if mont else 0, d_out_ptr))


def _wsum_pair(fn, width, ctx, d_points_ptr, n, d_weights16_ptr, mont):
    lo, hi = ctypes.create_string_buffer(width), ctypes.create_string_buffer(width)
    ctx._check(fn(ctx._h, d_points_ptr, n, 1 if mont else 0, d_weights16_ptr, lo, hi))
    return lo.raw, hi.raw


def g1_wsum_pair(ctx, d_points_ptr, n, d_weights16_ptr, mont=False):
    """(sum_(i<n-1) w_i P_i, sum_(i<n-1) w_i P_(i+1)) for n >= 2 affine G1 points on the device (64 B, all zero = infinity) and n - 1 weights of 16 little-endian bytes
    on the device: the pair of sums a powers-of-tau section is checked with (include/zkcensus_ptau_verify.h).  mont: the points' coordinates are in Montgomery form, as a
    .ptau stores them.  Returns two 64-byte points in standard form (all zero = infinity).  A point off the curve raises (ZKC_ERR_FORMAT, the smallest index in the text)."""
    return _wsum_pair(ctx._lib.zkc_g1_wsum_pair_dev, 64, ctx, d_points_ptr, n, d_weights16_ptr, mont)


def g2_wsum_pair(ctx, d_points_ptr, n, d_weights16_ptr, mont=False):
    """The same in G2: points 128 B (x.c0 | x.c1 | y.c0 | y.c1), anywhere on the twist."""
    return _wsum_pair(ctx._lib.zkc_g2_wsum_pair_dev, 128, ctx, d_points_ptr, n, d_weights16_ptr, mont)


def fixed_mul_window():
    """The window width w of the fixed-base tables (256 / w windows of 2^w - 1 rows)."""
    from . import _native
    return _native.load().zkc_fixed_mul_window()


class G1Bases:
    """n fixed G1 bases resident as pre-shifted window tables; multiExpAffine(scalars) = sum s_i P_i."""

    def __init__(self, ctx, d_bases_ptr, n):
        self.ctx, self.n = ctx, n
        h = ctypes.c_void_p()
        ctx._check(ctx._lib.zkc_msm_g1_load_dev(ctx._h, d_bases_ptr, n, ctypes.byref(h)))
        self._h = h

    def multiExpAffine(self, d_scalars_ptr):
        out = ctypes.create_string_buffer(64)
        self.ctx._check(self.ctx._lib.zkc_msm_g1_dev(self._h, d_scalars_ptr, out))
        return out.raw

    def close(self):
        if getattr(self, '_h', None):
            self.ctx._lib.zkc_msm_g1_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
