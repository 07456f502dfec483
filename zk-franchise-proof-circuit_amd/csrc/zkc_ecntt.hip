// zkc_ecntt.hip -- the inverse discrete Fourier transform of a vector of curve POINTS ("EC-NTT"), in G1 and in G2 (product code): monomial powers-of-tau points
// M_i = tau^i G to the Lagrange basis L_c = 1/n sum_i w^(-c i) M_i of the size-n domain, n = 2^logn, natural order on both sides.  `snarkjs powersoftau prepare phase2`
// is this transform at every size up to the file's power, over G1 three times and over G2 once (zkc_ptau_prepare.hip); zkc_g1_lagrange_dev / zkc_g2_lagrange_dev are the
// engine on its own (include/zkcensus_ptau_prepare.h).
//
// Shape.  Decimation in time, radix 2, one kernel launch per stage, one lane per butterfly, the vector in global memory as canonical XYZZ between the launches:
//   load    one lane per input point: (1/n) M_i by double-and-add over the bits of 1/n -- they come in the launch arguments, so every branch on them is wave-uniform --
//           with the mixed addition (G::madd through add_point: the operand is affine), stored at the bit-reversed index.  The 1/n factor is applied here, once.
//   stage s (s = 0 .. logn - 1, half = 2^s): butterfly j takes P = v[a], Q = v[a + half], a = (j >> s) 2^(s+1) + k, k = j mod half, to (P + t Q, P - t Q) with
//           t = w_(2 half)^(-k) = w_n'^(-k 2^(logn' - 1 - s)) read from the inverse half of the loaders' twiddle set (ntt_twiddle_tables; one table of the largest domain
//           serves every smaller one by stride).  k = 0 is the unit twiddle and does no product: all of stage 0, half of stage 1, a 2^-s share of stage s.  (-1 never
//           appears: k < half.)  Otherwise t Q is double-and-add from the scalar's leading bit with the COMPLETE doubling and addition (G::pt_dbl, G::add): after the
//           load no operand is affine.  The two additions of the butterfly are complete as well: with tau on a domain the monomial points repeat, and P + t Q meets equal
//           points, opposite points and infinity (zkc_point_ops.h).
//   affine  the batched inversion of the fixed-base engine (fixed_affine<F>): the bytes are canonical, so host and device compare byte for byte.
// There is no workgroup-resident group of stages and no tile: no constant here sets how many stages or points a workgroup handles (the tests' T), every launch is
// (n / 2 + 63) / 64 workgroups of one wave.  A product is ~254 doublings and ~127 additions of ~9 and ~14 field products on ONE lane, so a stage moves 256 (G2: 512) bytes
// per butterfly against some 4 000 (G2: 12 000) field products: the kernel is bound by the vector units, not by the trips through global memory that separate launches
// cost, which is why the stages are not fused.  Every loop is bounded by a constant or by a count from the launch arguments.
#include <cstring>
#include <string>
#include "zkc_prover.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_host_util.h"
#include "zkc_point_ops.h"
#include "zkc_kernels.h"
#include "zkc_ecntt.h"
#include "../../include/zkcensus_ptau_prepare.h"

using namespace zkc;

namespace {

struct EcScalar { uint32_t k[8]; int top; };       // standard form; top: the index of the leading bit

// ================================================================ device ================================================================

// n x ncoord coordinates in standard form -> Montgomery form.  A coordinate >= q is copied as it is, for the check that follows to find
__global__ void __launch_bounds__(256)
zkc_ecntt_to_mont(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t ncoord) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncoord) return;
    uint32_t w[8]; load_words<8>(w, in + 8 * i);
    if (fp_std_lt_p<FqParams>(w)) { const Fq a = fp_from_std<FqParams>(w);
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = a.v[k]; }
    uint4* q = reinterpret_cast<uint4*>(out + 8 * i);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]); q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// ---- load: work[bitrev(i)] = s * pts[i] as canonical XYZZ (infinity: all zero); s != 0 ----
template <class G> __global__ void __launch_bounds__(64)
zkc_ecntt_load(const uint32_t* __restrict__ pts, uint32_t logn, EcScalar s, XYZZ<typename G::F>* __restrict__ work) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << logn)) return;
    uint32_t w[G::W]; load_words<G::W>(w, pts + (size_t)G::W * i);
    const uint32_t at = logn ? __brev(i) >> (32 - logn) : 0;
    XYZZ<typename G::F> o = XYZZ<typename G::F>::inf();
    if (!all_zero<G::W>(w)) {
        const typename G::Pt p = G::enter(w, false);
        typename G::Acc acc; G::set(acc, p); bool inf = false;
        for (int j = s.top - 1; j >= 0; j--) {       // wave-uniform
            if (!inf) G::dbl(acc);                   // a doubling never meets infinity: the group has odd order
            if ((s.k[j >> 5] >> (j & 31)) & 1u) add_point<G>(acc, inf, p);
        }
        if (!inf) o = G::leave(acc);
    }
    work[at] = o;
}

// ---- one stage: see the head of the file.  tw_shift = tw_logn - 1 - s: the stride of this stage's twiddles in the table ----
// The kernel below only hands its arguments to this body: written in the kernel itself the G2 stage was measured at 1232 bytes of scratch per lane, in this form at 1200.
template <class G> __device__ __forceinline__ void stage_body(XYZZ<typename G::F>* __restrict__ work, uint32_t logn, uint32_t s, const Fr* __restrict__ tw, uint32_t tw_shift) {
    typedef XYZZ<typename G::F> X;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (1u << (logn - 1))) return;
    const uint32_t half = 1u << s, k = j & (half - 1);
    const size_t a = ((size_t)(j >> s) << (s + 1)) | k, b = a + half;
    const X P = work[a]; X Q = work[b];
    if (k != 0 && !Q.is_inf()) {
        uint32_t e[8]; fp_to_std<FrParams>(e, ld_fr(tw + ((size_t)k << tw_shift)));     // a power of a root of unity: never zero
        const typename G::Acc q = G::from_xyzz(Q);
        typename G::Acc acc = q, r; bool started = false;
        // 256 steps from the top bit; the words move up one bit per step, so no register is indexed by the loop counter.  Until the leading one a step is eight shifts.
        for (int it = 0; it < 256; it++) {
            const uint32_t bit = shl1_out(e);
            if (!started) { started = bit != 0; continue; }
            if (!G::is_inf(acc)) { G::pt_dbl(r, acc); acc = r; }
            if (bit) { G::add(r, acc, q); acc = r; }
        }
        Q = G::is_inf(acc) ? X::inf() : G::leave(acc);
    }
    const typename G::Acc p = G::from_xyzz(P);
    typename G::Acc q = G::from_xyzz(Q), r;
    G::add(r, p, q);
    work[a] = G::is_inf(r) ? X::inf() : G::leave(r);
    q = G::from_xyzz(xyzz_neg(Q));                  // the negative of infinity is infinity: ZZ stays zero
    G::add(r, p, q);
    work[b] = G::is_inf(r) ? X::inf() : G::leave(r);
}

template <class G> __global__ void __launch_bounds__(64)
zkc_ecntt_stage(XYZZ<typename G::F>* __restrict__ work, uint32_t logn, uint32_t s, const Fr* __restrict__ tw, uint32_t tw_shift) { stage_body<G>(work, logn, s, tw, tw_shift); }

// ================================================================ host ================================================================

// the body of the two public calls
template <class F>
int lagrange_entry(zkc_ctx* ctx, const void* d_points, uint32_t logn, int mont, void* d_out) {
    const std::string name = GroupOf<F>::lagrange_dev;
    if (!ctx || !d_points || !d_out || logn > ECNTT_MAX_LOGN) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, name + ": bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = 1u << logn; constexpr size_t PT = sizeof(Affine<F>);
    DevBuf conv, tw; int rc;
    const void* src = d_points;
    if (!mont) {
        if ((rc = conv.alloc(ctx, (size_t)n * PT)) || (rc = coords_to_mont(ctx, d_points, conv.p, (size_t)n * (PT / 32)))) return rc;
        src = conv.p;
    }
    uint32_t bad = 0;
    if ((rc = points_check_dev<F>(ctx, src, n, &bad))) return rc;
    if (bad != 0xffffffffu) return zkc_fail(ctx, ZKC_ERR_FORMAT, name + ": point " + std::to_string(bad) + " has a coordinate >= q or is not on the curve");
    if (logn >= 2 && (rc = ecntt_twiddles(ctx, logn, (Fr**)&tw.p))) return rc;
    return ecntt<F>(ctx, src, logn, tw.as<Fr>(), logn, d_out, mont != 0, nullptr);
}

}  // namespace

namespace zkc {

int coords_to_mont(zkc_ctx* ctx, const void* d_in, void* d_out, size_t ncoord) {
    if (!ncoord) return ZKC_OK;
    hipLaunchKernelGGL(zkc_ecntt_to_mont, dim3((unsigned)((ncoord + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_in, (uint32_t*)d_out, ncoord);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    return ZKC_OK;
}

int ecntt_twiddles(zkc_ctx* ctx, uint32_t logn, Fr** d_tw) {
    if (logn < 1 || logn > ECNTT_MAX_LOGN) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "ecntt_twiddles: bad size");
    TwiddleTables t;
    const int rc = ntt_twiddle_tables(ctx, (int)logn, true, &t, false); if (rc) return rc;      // the Fr tables alone: no limb form is made
    (void)hipFree(t.fwd);
    *d_tw = t.inv;
    return ZKC_OK;
}

template <class F>
int ecntt(zkc_ctx* ctx, const void* d_pts, uint32_t logn, const Fr* d_tw, uint32_t tw_logn, void* d_out, bool out_mont, double* ms) {
    typedef typename GroupOf<F>::Ops G;
    if (logn > ECNTT_MAX_LOGN || (logn >= 2 && (!d_tw || tw_logn < logn))) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "ecntt: bad size or twiddle table");
    const uint32_t n = 1u << logn;
    EcScalar s{}; s.top = 0;
    fp_to_std<FrParams>(s.k, fp_inv<FrParams>(fp_from_u32<FrParams>(n)));
    for (int i = 255; i >= 0; i--) if ((s.k[i >> 5] >> (i & 31)) & 1u) { s.top = i; break; }
    DevBuf work; int rc;
    if ((rc = work.alloc(ctx, (size_t)n * sizeof(XYZZ<F>)))) return rc;
    const clk::time_point t0 = clk::now();
    hipLaunchKernelGGL(zkc_ecntt_load<G>, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const uint32_t*)d_pts, logn, s, work.as<XYZZ<F>>());
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    for (uint32_t st = 0; st < logn; st++) {
        hipLaunchKernelGGL(zkc_ecntt_stage<G>, dim3((n / 2 + 63) / 64), dim3(64), 0, ctx->stream, work.as<XYZZ<F>>(), logn, st, d_tw, st ? tw_logn - 1 - st : 0);      // stage 0 reads no twiddle
        ZKC_HIP_CHECK(ctx, hipGetLastError());
    }
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const clk::time_point t1 = clk::now();
    rc = fixed_affine<F>(ctx, work.as<XYZZ<F>>(), n, d_out, out_mont);      // synchronises
    if (ms) { ms[0] += ms_since(t0, t1); ms[1] += ms_since(t1); }
    return rc;
}
template int ecntt<Fq>(zkc_ctx*, const void*, uint32_t, const Fr*, uint32_t, void*, bool, double*);
template int ecntt<Fq2>(zkc_ctx*, const void*, uint32_t, const Fr*, uint32_t, void*, bool, double*);

}  // namespace zkc

extern "C" int zkc_g1_lagrange_dev(zkc_ctx* ctx, const void* d_points, uint32_t logn, int mont, void* d_out) { return lagrange_entry<Fq>(ctx, d_points, logn, mont, d_out); }
extern "C" int zkc_g2_lagrange_dev(zkc_ctx* ctx, const void* d_points, uint32_t logn, int mont, void* d_out) { return lagrange_entry<Fq2>(ctx, d_points, logn, mont, d_out); }
