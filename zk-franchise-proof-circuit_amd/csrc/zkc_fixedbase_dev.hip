// zkc_fixedbase_dev.hip -- fixed-base batch products k_i * P in G1 and G2 on the GPU, one scalar per lane (product code), and the engines built on them:
// zkc_g1_fixed_mul_dev / zkc_g2_fixed_mul_dev (include/zkcensus_setup.h) and the point stage of zkc_setup_from_r1cs_dev (zkc_setup.hip).
//
// With the window table T[j][d - 1] = d 2^(8 j) P of zkc_fixedbase.h (w = 8: 32 windows of 255 affine points) a product needs no doubling and no sorting: the scalar's
// 32 bytes are its digits, and every non-zero digit costs one mixed addition XYZZ += affine in the radix-2^29 arithmetic of the MSM bucket accumulation (zkc_f29_g1.h,
// zkc_f29_g2.h).  Two launches per batch:
//   zkc_fixed_acc_g1 / _g2   one lane per scalar: walk the digits from the lowest window up, gather T[j][d - 1], add; the sum leaves as a canonical XYZZ point
//   zkc_fixed_affine<F>      XYZZ -> affine without an inversion per point: a lane takes FIXED_INV_CHUNK points (strided, so that the lanes of a wave read neighbours),
//                            multiplies their ZZZ up (Montgomery's trick), inverts the product once and walks back: 3 products per point plus 1 / 8 of an inversion
//   zkc_points_check<G>      not part of a product: one lane per affine point of a file, coordinates < q and on the curve (zkc_point_ops.h).  It is here because this
//                            file is what every user of it already builds on, for zkc_fixed_affine
// The tables live in global memory (G1: 8160 x 64 B = 510 KB; G2: 8160 x 240 B = 1.9 MB in the row format of zkc_g2_table29) and are built on the host.
#include <cstring>
#include <string>
#include <vector>
#include "zkc_prover.h"
#include "zkc_fixedbase.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_f29.h"
#include "zkc_f29_g1.h"
#include "zkc_f29_g2.h"
#include "zkc_host_util.h"
#include "zkc_point_ops.h"
#include "zkc_pairing.h"
#include "../../include/zkcensus_setup.h"

using namespace zkc;

namespace {

constexpr int FIXED_INV_CHUNK = 8;       // points per lane of zkc_fixed_affine

// the scalar of lane i as eight words of standard form
__device__ __forceinline__ void load_scalar(uint32_t s[8], const uint32_t* __restrict__ scalars, uint32_t i, int scalars_mont) {
    const uint4* ip = reinterpret_cast<const uint4*>(scalars + 8 * (size_t)i); const uint4 a = ip[0], b = ip[1];
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    if (scalars_mont) {
        Fr m;
#pragma unroll
        for (int k = 0; k < 8; k++) m.v[k] = s[k];
        fp_to_std<FrParams>(s, m);
    }
}
// the lowest digit, and the scalar moved down by one window: the words stay in registers (an index that depends on the loop counter would send them to scratch)
__device__ __forceinline__ uint32_t next_digit(uint32_t s[8]) {
    const uint32_t d = s[0] & ((1u << FIXED_W) - 1);
#pragma unroll
    for (int k = 0; k < 7; k++) s[k] = (s[k] >> FIXED_W) | (s[k + 1] << (32 - FIXED_W));
    s[7] >>= FIXED_W;
    return d;
}

// Why the incomplete addition is enough (both groups).  The windows are walked from the lowest up, so when digit d of window j is added the accumulator holds m P with
// m = k mod 2^(8 j), and m > 0 (an accumulator at infinity is set, not added to).  For a scalar k < r:  0 < m < 2^(8 j) <= d 2^(8 j) <= k < r.  The table entry is
// t P with t = d 2^(8 j), so 0 < m < t < r and 0 < m + t <= k < r: neither m = t nor m = -t (mod r) can hold, P having order r.  The accumulator is therefore never
// equal to the entry nor to its negative, f29_madd / f29g2_madd_lean never meet their exceptional case, and their `false` return is not handled here.  Scalars of r
// and above are outside the contract (zkcensus_setup.h).
__global__ void __launch_bounds__(64)
zkc_fixed_acc_g1(const Affine<Fq>* __restrict__ table, const uint32_t* __restrict__ scalars, int scalars_mont, uint32_t n, XYZZ<Fq>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8]; load_scalar(s, scalars, i, scalars_mont);
    Acc29 acc; bool inf = true;
    for (int j = 0; j < FIXED_NWIN; j++) {
        const uint32_t d = next_digit(s);
        if (!d) continue;
        const uint4* q = reinterpret_cast<const uint4*>(table + (size_t)j * ((1 << FIXED_W) - 1) + (d - 1));
        const uint4 a = q[0], b = q[1], c = q[2], e = q[3];
        const uint32_t px[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, py[8] = {c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
        uint32_t x2[9], y2[9];
        f29_from_fp_shl5(x2, px); f29_from_fp_shl5(y2, py);
        if (inf) {
            f29_mul<FqParams>(acc.X, x2, F29K<FqParams>::one.l); f29_mul<FqParams>(acc.Y, y2, F29K<FqParams>::one.l);
#pragma unroll
            for (int k = 0; k < 9; k++) acc.ZZ[k] = acc.ZZZ[k] = F29K<FqParams>::one.l[k];
            inf = false;
        } else {
            bool same_y = false;
            (void)f29_madd(acc, x2, y2, same_y);           // never exceptional for a scalar below r: see above
        }
    }
    XYZZ<Fq> o = XYZZ<Fq>::inf();
    if (!inf) { o.X = f29_to_fp<FqParams>(acc.X); o.Y = f29_to_fp<FqParams>(acc.Y); o.ZZ = f29_to_fp<FqParams>(acc.ZZ); o.ZZZ = f29_to_fp<FqParams>(acc.ZZZ); }
    out[i] = o;
}

// G2: the accumulator alone is 8 x 9 limbs = 72 registers, so the addition is the lean form of the G2 MSM (f29g2_madd_lean: its ten Fq2 products in an order that keeps
// few values alive) and the table row is loaded only once the digit is known, 2 x 80 bytes, straight into the operands.  Registers and scratch: DESIGN.md.
__global__ void __launch_bounds__(64)
zkc_fixed_acc_g2(const uint32_t* __restrict__ table29, const uint32_t* __restrict__ scalars, int scalars_mont, uint32_t n, XYZZ<Fq2>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8]; load_scalar(s, scalars, i, scalars_mont);
    Acc29G2 acc; bool inf = true;
    for (int j = 0; j < FIXED_NWIN; j++) {
        const uint32_t d = next_digit(s);
        if (!d) continue;
        const uint4* q = reinterpret_cast<const uint4*>(table29 + ((size_t)j * ((1 << FIXED_W) - 1) + (d - 1)) * G2ROW_WORDS);       // x and y, the first two chunks of a row (zkc_f29_g2.h)
        uint32_t w[40];
#pragma unroll
        for (int k = 0; k < 10; k++) { const uint4 v = q[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
        F2x29 x2, y2;
#pragma unroll
        for (int k = 0; k < 9; k++) { x2.c0[k] = w[k]; x2.c1[k] = w[9 + k]; y2.c0[k] = w[G2ROW_Y + k]; y2.c1[k] = w[G2ROW_Y + 9 + k]; }
        if (inf) {
            acc.X = x2; acc.Y = y2;
#pragma unroll
            for (int k = 0; k < 9; k++) { acc.ZZ.c0[k] = acc.ZZZ.c0[k] = F29K<FqParams>::one.l[k]; acc.ZZ.c1[k] = acc.ZZZ.c1[k] = 0; }
            inf = false;
        } else {
            bool same_y = false;
            (void)f29g2_madd_lean(acc, x2, y2, same_y);    // never exceptional for a scalar below r: see above
        }
    }
    XYZZ<Fq2> o = XYZZ<Fq2>::inf();
    if (!inf) { o.X = f29g2_leave(acc.X); o.Y = f29g2_leave(acc.Y); o.ZZ = f29g2_leave(acc.ZZ); o.ZZZ = f29g2_leave(acc.ZZZ); }
    out[i] = o;
}

__device__ __forceinline__ void store_coord(uint32_t* __restrict__ o, const Fq& a, int mont) {
    uint32_t s[8];
    if (mont) {
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = a.v[k];
    } else fp_to_std<FqParams>(s, a);
    uint4* op = reinterpret_cast<uint4*>(o);
    op[0] = make_uint4(s[0], s[1], s[2], s[3]); op[1] = make_uint4(s[4], s[5], s[6], s[7]);
}
__device__ __forceinline__ void store_coord(uint32_t* __restrict__ o, const Fq2& a, int mont) { store_coord(o, a.c0, mont); store_coord(o + 8, a.c1, mont); }

// in -> affine (x | y, 2 x sizeof(F) bytes per point; infinity = all zero).  Lane g owns the points g, g + nlanes, g + 2 nlanes, ...: at most FIXED_INV_CHUNK of them.
// pre[i] = the product of the finite ZZZ before point i in its lane's walk (n x F of work space).
template <class F>
__global__ void __launch_bounds__(64)
zkc_fixed_affine(const XYZZ<F>* __restrict__ in, F* __restrict__ pre, uint32_t n, uint32_t nlanes, int out_mont, uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nlanes) return;
    constexpr uint32_t W = 2 * sizeof(F) / 4;          // words per affine point
    F acc = F::one();
    uint32_t cnt = 0;
    for (uint64_t i = g; i < n && cnt < FIXED_INV_CHUNK; i += nlanes, cnt++) {
        const F z = in[i].ZZZ;
        pre[i] = acc;
        if (!z.is_zero()) acc = acc * z;
    }
    F inv = fp_inv(acc);
    for (uint32_t k = cnt; k-- > 0;) {
        const uint64_t i = g + (uint64_t)k * nlanes;
        const XYZZ<F> p = in[i];
        uint32_t* o = out + i * W;
        if (p.ZZ.is_zero()) {
#pragma unroll
            for (uint32_t q = 0; q < W / 4; q++) reinterpret_cast<uint4*>(o)[q] = make_uint4(0, 0, 0, 0);
            continue;
        }
        const F zi3 = inv * pre[i];                    // 1 / ZZZ
        inv = inv * p.ZZZ;
        const F zi = zi3 * p.ZZ;                       // 1 / Z (ZZ = Z^2, ZZZ = Z^3), as xyzz_to_affine
        const F zi2 = fp_sqr(zi);
        store_coord(o, p.X * zi2, out_mont); store_coord(o + W / 2, p.Y * zi3, out_mont);
    }
}

// *bad (initialised to 0xffffffff) = the smallest index of a point with a coordinate >= q or off its curve y^2 = x^3 + b; all zero is infinity and passes.  Montgomery words
template <class G>
__global__ void __launch_bounds__(256)
zkc_points_check(const uint32_t* __restrict__ pts, uint32_t n, typename G::F b, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[G::W]; load_words<G::W>(w, pts + (size_t)G::W * i);
    if (all_zero<G::W>(w)) return;
    if (!coords_below_q<G>(w) || !on_curve<G>(w, b)) atomicMin(bad, i);
}

// the second launch of a batch: d_sum (n XYZZ points) -> d_out (n affine points), d_pre = n x F of work space; enqueued on ctx->stream, not waited for
template <class F>
hipError_t launch_affine(zkc_ctx* ctx, const XYZZ<F>* d_sum, F* d_pre, uint32_t n, bool out_mont, void* d_out) {
    const uint32_t nlanes = (n + FIXED_INV_CHUNK - 1) / FIXED_INV_CHUNK;
    hipLaunchKernelGGL(zkc_fixed_affine<F>, dim3((nlanes + 63) / 64), dim3(64), 0, ctx->stream, d_sum, d_pre, n, nlanes, out_mont ? 1 : 0, (uint32_t*)d_out);
    return hipGetLastError();
}

template <class F, class Launch>
int fixed_mul(zkc_ctx* ctx, const char* what, uint32_t n, void* d_out, bool out_mont, Launch launch_acc) {
    DevBuf sum, pre; int rc;
    if ((rc = sum.alloc(ctx, (size_t)n * sizeof(XYZZ<F>))) || (rc = pre.alloc(ctx, (size_t)n * sizeof(F)))) return rc;
    launch_acc(sum.as<XYZZ<F>>());
    hipError_t e = launch_affine<F>(ctx, sum.as<XYZZ<F>>(), pre.as<F>(), n, out_mont, d_out);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return ZKC_OK;
}

}  // namespace

namespace zkc {

int fixed_table_g1(zkc_ctx* ctx, const G1Affine& base, G1Affine** d_table, double* host_ms) {
    const clk::time_point t0 = clk::now();
    const FixedBase<Fq> fb(base);
    if (host_ms) *host_ms = ms_since(t0);
    *d_table = nullptr;
    DevBuf tab; int rc;
    if ((rc = tab.alloc(ctx, fb.tab.size() * sizeof(G1Affine)))) return rc;
    const hipError_t e = hipMemcpy(tab.p, fb.tab.data(), fb.tab.size() * sizeof(G1Affine), hipMemcpyHostToDevice);
    if (e != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, std::string("fixed_table_g1: ") + hipGetErrorString(e));
    *d_table = (G1Affine*)tab.release();
    return ZKC_OK;
}

int fixed_table_g2(zkc_ctx* ctx, const G2Affine& base, uint32_t** d_table29, double* host_ms) {
    const clk::time_point t0 = clk::now();
    const FixedBase<Fq2> fb(base);
    if (host_ms) *host_ms = ms_since(t0);
    *d_table29 = nullptr;
    DevBuf tmp; int rc;
    if ((rc = tmp.alloc(ctx, fb.tab.size() * sizeof(G2Affine)))) return rc;
    const hipError_t e = hipMemcpy(tmp.p, fb.tab.data(), fb.tab.size() * sizeof(G2Affine), hipMemcpyHostToDevice);
    if (e != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, std::string("fixed_table_g2: ") + hipGetErrorString(e));
    return msm_g2_rows29(ctx, tmp.as<G2Affine>(), fb.tab.size(), "fixed_table_g2", d_table29);      // the row format of the G2 MSM, made by its kernel
}

template <class F>
int fixed_affine(zkc_ctx* ctx, const XYZZ<F>* d_in, uint32_t n, void* d_out, bool out_mont) {
    DevBuf pre; int rc;
    if ((rc = pre.alloc(ctx, (size_t)n * sizeof(F)))) return rc;
    hipError_t e = launch_affine<F>(ctx, d_in, pre.as<F>(), n, out_mont, d_out);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, std::string(GroupOf<F>::g2 ? "fixed_affine<Fq2>: " : "fixed_affine<Fq>: ") + hipGetErrorString(e));
    return ZKC_OK;
}
template int fixed_affine<Fq>(zkc_ctx*, const XYZZ<Fq>*, uint32_t, void*, bool);
template int fixed_affine<Fq2>(zkc_ctx*, const XYZZ<Fq2>*, uint32_t, void*, bool);

template <class F>
int points_check_dev(zkc_ctx* ctx, const void* d_pts, uint32_t n, uint32_t* bad) {
    F b;
    if constexpr (GroupOf<F>::g2) b = pairing::consts().twist_b; else b = fp_from_u32<FqParams>(3);
    DevBuf flag; int rc;
    if ((rc = flag.alloc(ctx, 4))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(flag.p, 0xff, 4, ctx->stream));
    hipLaunchKernelGGL(zkc_points_check<typename GroupOf<F>::Ops>, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)d_pts, n, b, flag.as<uint32_t>());
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(bad, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKC_OK;
}
template int points_check_dev<Fq>(zkc_ctx*, const void*, uint32_t, uint32_t*);
template int points_check_dev<Fq2>(zkc_ctx*, const void*, uint32_t, uint32_t*);

int fixed_mul_g1(zkc_ctx* ctx, const G1Affine* d_table, const void* d_scalars, bool scalars_mont, uint32_t n, void* d_out, bool out_mont) {
    return fixed_mul<Fq>(ctx, "fixed_mul_g1", n, d_out, out_mont, [&](XYZZ<Fq>* d_sum) {
        hipLaunchKernelGGL(zkc_fixed_acc_g1, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_table, (const uint32_t*)d_scalars, scalars_mont ? 1 : 0, n, d_sum);
    });
}
int fixed_mul_g2(zkc_ctx* ctx, const uint32_t* d_table29, const void* d_scalars, bool scalars_mont, uint32_t n, void* d_out, bool out_mont) {
    return fixed_mul<Fq2>(ctx, "fixed_mul_g2", n, d_out, out_mont, [&](XYZZ<Fq2>* d_sum) {
        hipLaunchKernelGGL(zkc_fixed_acc_g2, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_table29, (const uint32_t*)d_scalars, scalars_mont ? 1 : 0, n, d_sum);
    });
}

}  // namespace zkc

extern "C" int zkc_fixed_mul_window(void) { return FIXED_W; }

// d_out[i] = k_i * base through the window table of `base`; conventions of zkc_g1_mul_batch_dev, plus the curve check.
extern "C" int zkc_g1_fixed_mul_dev(zkc_ctx* ctx, const uint8_t base_std[64], const void* d_scalars, uint32_t n, void* d_out) {
    if (!ctx || !base_std || !d_scalars || !d_out || n == 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_fixed_mul_dev: bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    G1Affine p;
    if (!rd_g1_std(p, base_std)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_fixed_mul_dev: base coordinate >= q");
    if (p.is_inf()) {                                          // k * infinity
        ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, (size_t)n * 64, ctx->stream));
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return ZKC_OK;
    }
    if (!pairing::g1_on_curve(p)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_fixed_mul_dev: base not on the curve");
    DevBuf table;
    int rc = fixed_table_g1(ctx, p, (G1Affine**)&table.p, nullptr); if (rc) return rc;
    return fixed_mul_g1(ctx, table.as<G1Affine>(), d_scalars, false, n, d_out, false);
}

extern "C" int zkc_g2_fixed_mul_dev(zkc_ctx* ctx, const uint8_t base_std[128], const void* d_scalars, uint32_t n, void* d_out) {
    if (!ctx || !base_std || !d_scalars || !d_out || n == 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g2_fixed_mul_dev: bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    G2Affine p;
    if (!rd_g2_std(p, base_std)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g2_fixed_mul_dev: base coordinate >= q");
    if (p.is_inf()) {
        ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, (size_t)n * 128, ctx->stream));
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return ZKC_OK;
    }
    if (!pairing::g2_on_curve(p)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g2_fixed_mul_dev: base not on the twist");      // y^2 = x^3 + 3 / (9 + u)
    DevBuf table;
    int rc = fixed_table_g2(ctx, p, (uint32_t**)&table.p, nullptr); if (rc) return rc;
    return fixed_mul_g2(ctx, table.as<uint32_t>(), d_scalars, false, n, d_out, false);
}
