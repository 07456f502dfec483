// zkc_generic.hip -- the prover's NTT and G1 MSM engines as stand-alone device entry points (no .zkey): what ffjavascript's
// `Fr.fft / Fr.ifft` and `G1.multiExpAffine` are to snarkjs (ts_inputs/src/example.ts:358 -> groth16.prove).  They exist for
// the circuit cannot reach a 2^20 domain, so the "large census" stress figures are a synthetic
// 2^20-point MSM over bases k_i G and a 2^20 NTT (tools/stress.py), checked against the oracle in exponent space.
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include "zkc_prover.h"
#include "zkc_host_util.h"

using namespace zkc;

namespace {
__global__ void __launch_bounds__(256) zkc_fill_fr(Fr* __restrict__ dst, Fr v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}
// affine standard form (x, y little endian; all zero = infinity)  <->  affine Montgomery
__global__ void __launch_bounds__(256) zkc_g1_std_to_mont(const uint32_t* __restrict__ in, G1Affine* __restrict__ out, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[8], y[8];
    for (int k = 0; k < 8; k++) { x[k] = in[16 * (size_t)i + k]; y[k] = in[16 * (size_t)i + 8 + k]; }
    if (!fp_std_lt_p<FqParams>(x) || !fp_std_lt_p<FqParams>(y)) { atomicOr(bad, 1u); return; }
    G1Affine a; a.x = fp_from_std<FqParams>(x); a.y = fp_from_std<FqParams>(y);
    if (!a.is_inf() && !(fp_sqr(a.y) == fp_sqr(a.x) * a.x + fp_from_u32<FqParams>(3))) atomicOr(bad, 2u);
    out[i] = a;
}
__global__ void __launch_bounds__(64) zkc_g1_xyzz_to_std(const G1XYZZ* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const G1Affine a = xyzz_to_affine(in[i]);
    uint32_t s[8];
    fp_to_std<FqParams>(s, a.x); for (int k = 0; k < 8; k++) out[16 * (size_t)i + k] = s[k];
    fp_to_std<FqParams>(s, a.y); for (int k = 0; k < 8; k++) out[16 * (size_t)i + 8 + k] = s[k];
}
// out[i] = k[i] * P by double-and-add (P: one affine Montgomery point)
__global__ void __launch_bounds__(64) zkc_g1_mul_same_base(G1Affine p, const uint32_t* __restrict__ scalars, uint32_t n, G1XYZZ* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8]; for (int q = 0; q < 8; q++) k[q] = scalars[8 * (size_t)i + q];
    out[i] = xyzz_mul(G1XYZZ::from_affine(p), k);
}
// out[i] = in[i] mod r for any 256-bit in[i] (2^256 < 6 r: at most five subtractions).  The signed-digit bucketing (msm_tile_digit) needs
// scalars below 2^254: it reads nw c bits (255 for c = 15 and 17, 256 for c = 16) and drops the carry out of the top window.
__global__ void __launch_bounds__(256) zkc_reduce_scalars(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* ip = reinterpret_cast<const uint4*>(in + 8 * (size_t)i); const uint4 a = ip[0], b = ip[1];
    uint32_t s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    for (int k = 0; k < 5 && !fp_std_lt_p<FrParams>(s); k++) {
        uint64_t br = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) { const uint64_t d = (uint64_t)s[q] - FrParams::p[q] - br; s[q] = (uint32_t)d; br = (d >> 63) & 1; }
    }
    uint4* op = reinterpret_cast<uint4*>(out + 8 * (size_t)i);
    op[0] = make_uint4(s[0], s[1], s[2], s[3]); op[1] = make_uint4(s[4], s[5], s[6], s[7]);
}
}  // namespace

struct zkc_msm {
    zkc_zkey zk;                 // only ctx and d_g1 are used by the MSM pipeline
    MsmWork w; uint32_t n = 0; int c = 0; MsmJobList jl;
    uint32_t* d_red = nullptr;   // n x 8 u32: the caller's scalars reduced mod r (zkc_reduce_scalars)
};

// In-place-capable NTT over BN254 Fr on `nvec` contiguous vectors of 2^logn elements in MONTGOMERY form (R = 2^256), natural order in
// and out; inverse != 0 computes the inverse transform including the 1/n factor.  d_src != d_dst.  3 <= logn <= 27.
extern "C" int zkc_ntt_dev(zkc_ctx* ctx, const void* d_src, void* d_dst, int logn, int nvec, int inverse) {
    if (!ctx || !d_src || !d_dst || d_src == d_dst || logn < 3 || logn > 27 || nvec <= 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_ntt_dev: bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = 1u << logn;
    zkc_ctx::TwiddleSet& t = ctx->ntt_tw[logn];     // owned by the context (its lock is held): released with it, never inherited by another device's context
    if (!t.fwd) {              // the set is complete or absent: its three tables are handed over together, once all of them exist
        DevBuf ninv, fwd, inv; TwiddleTables tw; int rc;
        if ((rc = ninv.alloc(ctx, (size_t)n * sizeof(Fr))) || (rc = ntt_twiddle_tables(ctx, logn, false, &tw))) return rc;
        fwd.p = tw.fwd29; inv.p = tw.inv29;
        hipLaunchKernelGGL(zkc_fill_fr, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ninv.as<Fr>(), fp_inv<FrParams>(fp_from_u32<FrParams>(n)), n);
        ZKC_HIP_CHECK(ctx, hipGetLastError());
        t.fwd = (uint32_t*)fwd.release(); t.inv = (uint32_t*)inv.release(); t.ninv = ninv.release();
    }
    zkc_prof_scope _pn(ctx, ZKC_PROF_NTT, (uint64_t)nvec * 2ull * n * 32, ctx->stream);
    return ntt_run(ctx, ctx->stream, (const Fr*)d_src, (Fr*)d_dst, inverse ? t.inv : t.fwd, inverse ? (const Fr*)t.ninv : nullptr, logn, nvec);
}

// d_out[i] = k_i * base for n scalars (device, standard form 32 B each); base and outputs are affine points in standard form (64 B).
extern "C" int zkc_g1_mul_batch_dev(zkc_ctx* ctx, const uint8_t base_std[64], const void* d_scalars, uint32_t n, void* d_out) {
    if (!ctx || !base_std || !d_scalars || !d_out || n == 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_mul_batch_dev: bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    G1Affine p;
    if (!rd_g1_std(p, base_std)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_mul_batch_dev: base coordinate >= q");
    DevBuf tmp; int rc;
    if ((rc = tmp.alloc(ctx, (size_t)n * sizeof(G1XYZZ)))) return rc;
    hipLaunchKernelGGL(zkc_g1_mul_same_base, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, p, (const uint32_t*)d_scalars, n, tmp.as<G1XYZZ>());
    hipLaunchKernelGGL(zkc_g1_xyzz_to_std, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, tmp.as<G1XYZZ>(), (uint32_t*)d_out, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, std::string("zkc_g1_mul_batch_dev: ") + hipGetErrorString(e));
    return ZKC_OK;
}

// A fixed set of n G1 bases (device, affine standard form, 64 B each) made resident as pre-shifted window tables.
extern "C" int zkc_msm_g1_load_dev(zkc_ctx* ctx, const void* d_bases_std, uint32_t n, zkc_msm** out) {
    if (!ctx || !d_bases_std || !out || n == 0 || n > (1u << 21)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_msm_g1_load_dev: bad argument (1 <= n <= 2^21)");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<zkc_msm, void (*)(zkc_msm*)> m(new zkc_msm(), zkc_msm_g1_free);      // a half-built set goes the way of a finished one
    m->zk.ctx = ctx; m->n = n; m->c = msm_c_for(n);
    const int nw = msm_nw(m->c);
    DevBuf d_bad; uint32_t bad = 0; int rc = ZKC_OK;
    if (hipMalloc((void**)&m->zk.d_g1, (size_t)nw * n * sizeof(G1Affine)) != hipSuccess || hipMalloc((void**)&m->d_red, (size_t)n * 32) != hipSuccess ||
        hipMalloc(&d_bad.p, 4) != hipSuccess || hipMemset(d_bad.p, 0, 4) != hipSuccess)
        return zkc_fail(ctx, ZKC_ERR_HIP, "zkc_msm_g1_load_dev: hipMalloc failed");
    hipLaunchKernelGGL(zkc_g1_std_to_mont, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)d_bases_std, m->zk.d_g1, n, d_bad.as<uint32_t>());
    if (hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return zkc_fail(ctx, ZKC_ERR_HIP, "zkc_msm_g1_load_dev: base conversion failed");
    if (bad) return zkc_fail(ctx, ZKC_ERR_FORMAT, bad & 1 ? "zkc_msm_g1_load_dev: base coordinate >= q" : "zkc_msm_g1_load_dev: base not on the curve");
    if ((rc = msm_precompute_g1(ctx, n, m->zk.d_g1, m->c))) return rc;
    if ((rc = msm_work_alloc(ctx, m->w, (size_t)nw * n, (size_t)msm_half(m->c), 1, false))) return rc;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, "zkc_msm_g1_load_dev: table build failed");
    *out = m.release();
    return ZKC_OK;
}
// sum_i (s_i mod r) P_i over the resident bases; d_scalars: n x 32 B, any 256-bit integers (device); out: affine standard form (all zero = infinity)
extern "C" int zkc_msm_g1_dev(zkc_msm* m, const void* d_scalars, uint8_t out[64]) {
    if (!m || !d_scalars || !out) return ZKC_ERR_BAD_ARG;
    zkc_ctx* ctx = m->zk.ctx;
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(zkc_reduce_scalars, dim3((m->n + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)d_scalars, m->d_red, m->n);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    m->jl.clear(); m->jl.add(m->d_red, nullptr, m->n, 0, m->n, 0, m->c);
    int rc = msm_pass_g1(&m->zk, m->w, m->jl, 0, true, ctx->stream); if (rc) return rc;
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const G1Affine a = xyzz_to_affine(*(const G1XYZZ*)m->w.h_results);
    wr_g1_std(out, a);
    return ZKC_OK;
}
extern "C" void zkc_msm_g1_free(zkc_msm* m) {
    if (!m) return;
    ZKC_LOCK(m->zk.ctx);
    (void)hipSetDevice(m->zk.ctx->device); (void)hipStreamSynchronize(m->zk.ctx->stream);
    if (m->zk.d_g1) (void)hipFree(m->zk.d_g1);
    if (m->d_red) (void)hipFree(m->d_red);
    m->zk.d_g1 = nullptr; msm_work_free(m->w);
    delete m;
}
