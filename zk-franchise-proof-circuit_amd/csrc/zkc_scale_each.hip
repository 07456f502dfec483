// zkc_scale_each.hip -- the phase-1 ceremony of a powers-of-tau file (include/zkcensus_ptau_contribute.h): the batch product k_i * P_i for n points, EACH UNDER ITS OWN
// full-width scalar, on the GPU (product code), and the host side built on it: zkc_ptau_new, zkc_ptau_contribute (snarkjs `powersoftau new` / `contribute`),
// zkc_ptau_contributions and zkc_ptau_verify_contributions (the transcript part of `powersoftau verify`; the point checks are zkc_ptau_verify.hip).
//
// The kernel.  The library's other batch products are one scalar times many points (zkc_p2_scale_g1: the digits are wave-uniform) and one base times many scalars
// (zkc_fixedbase_dev.hip: a table of the base).  Here neither is shared: a contribution replaces T_i by tau'^i T_i.  One lane per point, one template over G1Ops / G2Ops
// (zkc_point_ops.h), two forms:
//   windowed (shipped)   the lane recodes its scalar into 64 signed 4-bit digits d_j in [-8, 7], sum d_j 16^j = k: k' = (k + 0x88..8) ^ 0x88..8 holds digit j as the
//                        two's-complement nibble j (the carry of the addition IS the recoding's carry; k < r < 2^254 leaves the top digit at most 4).  It builds the
//                        table 1P .. 8P of its own point (one doubling, six additions) in device work space, entry-major -- row e of lane i at (e n + i), so the lanes
//                        of a wave read neighbouring rows: 8 x 144 B per G1 lane, 8 x 288 B per G2 lane; not registers (the G2 accumulator alone is 72) and not LDS
//                        (a per-lane table there leaves one or two waves per CU).  Then every lane runs the same 64 steps from the top digit: four doublings
//                        (G::pt_dbl), one complete addition (G::add) of row |d_j| with y negated for d_j < 0 -- a select per limb, the sign is free -- and for d_j = 0 of
//                        that row with ZZ cleared, i.e. infinity.  No branch depends on a lane's bits except through the exceptional cases below.
//                        By count: 252 doublings, 64 complete additions, 7 table steps per point.
//   bit-serial           double-and-add from the top bit, G::dbl and the mixed add_point, as zkc_ptau_scale: on random scalars some lane of the wave adds at every
//                        step, so a wave pays about 254 doublings and 254 mixed additions.  Reachable only through the hooks: the yardstick of
//                        tools/ptau_contribute_bench.py.
// Both leave canonical XYZZ sums that become affine through the batched inversion of the fixed-base products (fixed_affine<F>); the point check is that of every kernel
// over the points of a file, fused into the scale kernel, with the scalar's range beside it: a refusal is found before anything reaches d_out.
//
// Which scalars reach which case of the complete addition (windowed form; P of order r, as every point of G1 and of G2 is).  Write m_j = sum_(i >= j) d_i 16^(i - j) for
// the prefixes: m_0 = k, and at step j the accumulator holds 16 m_(j+1) P = (m_j - d_j) P and the addend is d_j P, |d_j| <= 8.
//   accumulator at infinity   while every higher digit is zero: every scalar below 16^63, and k = 0 to the end (the result is infinity); the doublings are skipped
//   addend at infinity        every zero digit: k = 0, 1, 16, 2^k ..
//   equal operands            16 m_(j+1) = d_j mod r with 0 < 16 m_(j+1) <= k / 16^j + 8 < r + 8: only 16 m_1 = r + d_0, i.e. j = 0 and k = r + 2 d_0 with 16 | r + d_0;
//                             r = 1 mod 16, so d_0 = -1 and k = r - 2: the accumulator holds (r - 1) P = -P and -P is added.  G::add doubles.
//   opposite operands         16 m_(j+1) = -d_j mod r: 16 m_1 = r - d_0 means k = r.  No scalar below r.
// A point of the twist outside G2 has another order and may meet any of them: the additions are complete, so the result is still k P.  The table steps 2P .. 8P never
// meet an exceptional case (P has odd order above 8).  tests/test_gpu_scale_each.py has k = 0, 1, 16, r - 2 and the digits' carry chains.  Every loop is bounded by a
// constant (64 digits, 254 bits, 8 rows) or a host-computed count; nothing waits on a flag.
//
// The contribution.  Sections 2 .. 6 in chunks (CHUNK points; the device holds one chunk, its scalars, its table and its sums, never a section): read, upload, the
// chunk's scalars tau'^(first + lane) [x alpha', x beta'] from an uploaded table of tau'^(2^k) (zkc_tau_scalars: the host forms no per-point scalar), scale, affine,
// download, write to the temporary file of zkc_ptau_write.h.  With ctx = NULL the same steps run on the threads of par_chunks with zkc_curve.h; both paths leave canonical
// affine points, so the bytes agree.  Secrets and what derives from them are cleared before their storage is released: Secret on the host, a memset on the stream for the
// device's power table and scalars.
#include <cstring>
#include <string>
#include <vector>
#include "zkc_prover.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_f29.h"
#include "zkc_f29_g1.h"
#include "zkc_f29_g2.h"
#include "zkc_point_ops.h"
#include "zkc_host_util.h"
#include "zkc_pairing.h"
#include "zkc_file_points.h"
#include "zkc_phase2_parse.h"
#include "zkc_ptau_parse.h"
#include "zkc_ptau_write.h"
#include "zkc_ptau_contrib_parse.h"
#include "../../include/zkcensus_ptau_contribute.h"

using namespace zkc;

namespace {

constexpr uint32_t CHUNK = 1u << 20;             // points per chunk of a section: 2.8 GB of G2 work space (128 B point, 32 B scalar, 2304 B table, 256 B sum per lane)
constexpr uint32_t NONE = 0xffffffffu;
constexpr int WIN_ROWS = 8;                      // 1P .. 8P
constexpr int POW_ROWS = 32;                     // tau'^(2^k), k < 32: zkc_tau_scalars walks these 32 bits of first + lane and no more.  A contribution stays far below
                                                 // 2^32 through the limit on the file's power (exponents reach 2^29 - 2 at power 28); the hook refuses first + n > 2^32
constexpr int MULT_ROWS = 3;                     // then 1, alpha', beta': the multiplier of a section is a row of the same table, which is cleared with it

// ================================================================ device ================================================================

// an accumulator as the words of a table row (Acc29: 36 words, Acc29G2: 72), moved 16 bytes at a time.  The words pass through a local array with constant indices,
// which stays in registers; a cast of the accumulator itself would put it on the stack
__device__ __forceinline__ void acc_words(uint32_t* w, const Acc29& a) {
#pragma unroll
    for (int k = 0; k < 9; k++) { w[k] = a.X[k]; w[9 + k] = a.Y[k]; w[18 + k] = a.ZZ[k]; w[27 + k] = a.ZZZ[k]; }
}
__device__ __forceinline__ void acc_words(uint32_t* w, const Acc29G2& a) {
#pragma unroll
    for (int k = 0; k < 9; k++) { w[k] = a.X.c0[k]; w[9 + k] = a.X.c1[k]; w[18 + k] = a.Y.c0[k]; w[27 + k] = a.Y.c1[k];
                                  w[36 + k] = a.ZZ.c0[k]; w[45 + k] = a.ZZ.c1[k]; w[54 + k] = a.ZZZ.c0[k]; w[63 + k] = a.ZZZ.c1[k]; }
}
__device__ __forceinline__ void acc_of_words(Acc29& a, const uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 9; k++) { a.X[k] = w[k]; a.Y[k] = w[9 + k]; a.ZZ[k] = w[18 + k]; a.ZZZ[k] = w[27 + k]; }
}
__device__ __forceinline__ void acc_of_words(Acc29G2& a, const uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 9; k++) { a.X.c0[k] = w[k]; a.X.c1[k] = w[9 + k]; a.Y.c0[k] = w[18 + k]; a.Y.c1[k] = w[27 + k];
                                  a.ZZ.c0[k] = w[36 + k]; a.ZZ.c1[k] = w[45 + k]; a.ZZZ.c0[k] = w[54 + k]; a.ZZZ.c1[k] = w[63 + k]; }
}
template <class A> __device__ __forceinline__ void row_store(uint32_t* __restrict__ dst, const A& a) {
    uint32_t s[sizeof(A) / 4]; acc_words(s, a);
    uint4* q = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(A) / 16); k++) q[k] = make_uint4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
}
template <class A> __device__ __forceinline__ void row_load(A& a, const uint32_t* __restrict__ src) {
    uint32_t d[sizeof(A) / 4]; load_words<(int)(sizeof(A) / 4)>(d, src);
    acc_of_words(a, d);
}
// a table row made the addend of one step: y negated when neg, ZZ cleared (infinity) when zero.  G1 rows hold Y carried and below 18.7 p (f29_pt_dbl's bound, the
// widest of the operations that fill the table), which D26 dominates (carried values below 21.1 p): the negation is below 22.2 p and carried again, inside what
// f29_pt_add takes (below 32 p).  G2 rows hold Y below 3 p per component (tame), which D24 dominates: below 6.3 p, tame.
__device__ __forceinline__ void addend(Acc29& t, bool neg, bool zero) {
    constexpr L9 D26 = f29_dominator<FqParams>(1u << 29, 1u << 26);
    uint32_t nY[9];
#pragma unroll
    for (int k = 0; k < 9; k++) nY[k] = D26.l[k] - t.Y[k];
    f29_carry(nY);
#pragma unroll
    for (int k = 0; k < 9; k++) { t.Y[k] = neg ? nY[k] : t.Y[k]; t.ZZ[k] = zero ? 0u : t.ZZ[k]; }
}
__device__ __forceinline__ void addend(Acc29G2& t, bool neg, bool zero) {
    F2x29 nY; f29g2_neg_hi(nY, t.Y, Dom29G2::D24);
    f29_carry(nY.c0); f29_carry(nY.c1);
#pragma unroll
    for (int k = 0; k < 9; k++) { t.Y.c0[k] = neg ? nY.c0[k] : t.Y.c0[k]; t.Y.c1[k] = neg ? nY.c1[k] : t.Y.c1[k]; t.ZZ.c0[k] = zero ? 0u : t.ZZ.c0[k]; t.ZZ.c1[k] = zero ? 0u : t.ZZ.c1[k]; }
}
// the leading nibble of the 256-bit k leaves as the return value; k moves up by four bits
__device__ __forceinline__ uint32_t shl4_out(uint32_t k[8]) {
    const uint32_t top = k[7] >> 28;
#pragma unroll
    for (int i = 7; i > 0; i--) k[i] = (k[i] << 4) | (k[i - 1] >> 28);
    k[0] <<= 4;
    return top;
}

// out[i] = ks[i] * pts[i] as canonical XYZZ (infinity: all zero).  FORM 0: windowed, tab = WIN_ROWS x n rows; FORM 1: bit-serial, tab unused.  curve_b: the b of
// y^2 = x^3 + b in Montgomery form.  *bad (initialised to 0xffffffff) = the smallest index of a point with a coordinate >= q or off its curve, or of a scalar >= r
template <class G, int FORM> __global__ void __launch_bounds__(64)
zkc_scale_each(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks, uint32_t n, int mont, typename G::F curve_b, uint32_t* __restrict__ tab,
               XYZZ<typename G::F>* __restrict__ out, uint32_t* __restrict__ bad) {
    typedef typename G::Acc Acc;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8]; load_words<8>(k, ks + 8 * (size_t)i);
    uint32_t w[G::W]; load_words<G::W>(w, pts + (size_t)G::W * i);
    XYZZ<typename G::F> o = XYZZ<typename G::F>::inf();
    const bool pinf = all_zero<G::W>(w);
    bool ok = fp_std_lt_p<FrParams>(k);
    if (ok && !pinf) {
        ok = coords_below_q<G>(w);
        if (ok) {
            if (!mont) {
#pragma unroll
                for (int c = 0; c < G::W; c += 8) { const Fq v = fp_from_std<FqParams>(w + c);
#pragma unroll
                    for (int j = 0; j < 8; j++) w[c + j] = v.v[j]; }
            }
            ok = on_curve<G>(w, curve_b);
        }
    }
    if (!ok) { atomicMin(bad, i); out[i] = o; return; }
    if (pinf || all_zero<8>(k)) { out[i] = o; return; }
    const typename G::Pt p = G::enter(w, false);
    if constexpr (FORM == 0) {
        constexpr size_t ROW = sizeof(Acc) / 4;
        uint32_t* const lane = tab + ROW * i;                  // row e of this lane: lane + ROW n e
        const size_t step = ROW * (size_t)n;
        {
            Acc t1; G::set(t1, p); row_store(lane, t1);
            Acc cur; G::pt_dbl(cur, t1); row_store(lane + step, cur);
            for (int e = 2; e < WIN_ROWS; e++) { Acc nx; G::add(nx, cur, t1); cur = nx; row_store(lane + step * e, cur); }
        }
        { uint64_t c = 0;                                       // k' = (k + 0x88..8) ^ 0x88..8: nibble j = digit j in two's complement
#pragma unroll
          for (int j = 0; j < 8; j++) { c += (uint64_t)k[j] + 0x88888888u; k[j] = (uint32_t)c ^ 0x88888888u; c >>= 32; } }
        Acc acc; G::set_inf(acc);
        for (int j = 0; j < 64; j++) {
            const uint32_t nib = shl4_out(k);
            const bool neg = (nib & 8u) != 0;
            const uint32_t mag = neg ? 16u - nib : nib;         // 0 .. 8
            if (!G::is_inf(acc)) {                              // a doubling never meets infinity: odd order
#pragma unroll 1
                for (int d = 0; d < 4; d++) { Acc r; G::pt_dbl(r, acc); acc = r; }
            }
            Acc t; row_load(t, lane + step * (mag ? mag - 1 : 0));
            addend(t, neg, mag == 0);
            Acc sum; G::add(sum, acc, t); acc = sum;
        }
        if (!G::is_inf(acc)) o = G::leave(acc);
    } else {
        Acc acc; bool inf = true, started = false;
        for (int it = 0; it < 256; it++) {                      // as zkc_ptau_scale: until the leading one a step is eight shifts
            const uint32_t bit = shl1_out(k);
            if (!started) { if (bit) { G::set(acc, p); inf = false; started = true; } continue; }
            if (!inf) G::dbl(acc);
            if (bit) add_point<G>(acc, inf, p);
        }
        if (!inf) o = G::leave(acc);
    }
    out[i] = o;
}

// out[i] = pw[mult_row] * tau^(first + i), 32 B standard form: pw[k] = tau^(2^k) for k < POW_ROWS, then the multipliers, all in Montgomery form.  No secret rides in the
// kernel arguments
__global__ void __launch_bounds__(256)
zkc_tau_scalars(const Fr* __restrict__ pw, uint32_t mult_row, uint64_t first, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t e = first + i;
    Fr a = pw[mult_row];
    for (int b = 0; b < POW_ROWS; b++) if ((e >> b) & 1) a = a * pw[b];
    uint32_t s[8]; fp_to_std<FrParams>(s, a);
    uint4* q = reinterpret_cast<uint4*>(out + 8 * (size_t)i);
    q[0] = make_uint4(s[0], s[1], s[2], s[3]); q[1] = make_uint4(s[4], s[5], s[6], s[7]);
}

// ================================================================ host ================================================================

thread_local double g_con_ms[6] = {0, 0, 0, 0, 0, 0};
thread_local double g_each_ms[2] = {0, 0};       // the last engine call of the thread: the scale kernel, the conversion to affine

// Secret, SecretFr and std_is_zero: zkc_host_util.h
inline Fq curve_b_host(const Fq*) { return fp_from_u32<FqParams>(3); }
inline Fq2 curve_b_host(const Fq2*) { return pairing::consts().twist_b; }

// the work space one call of scale_each_dev allocates beside points, scalars and output
template <class F> size_t scale_each_work_bytes(uint32_t n, int form) {
    typedef typename GroupOf<F>::Ops G;
    return (size_t)n * sizeof(XYZZ<F>) + (form == 0 ? (size_t)WIN_ROWS * n * sizeof(typename G::Acc) : 0) + 4;
}

// d_out[i] = d_scalars[i] * d_points[i]: the body of the engines and of a chunk of a contribution.  The lock is held and the device is set; has synchronised and freed its
// work space on return.  *bad: the index the kernel refused (NONE: none), in which case d_out is untouched and the return is ZKC_OK.  ms (may be NULL): [0] the scale
// kernel, [1] the conversion to affine
template <class F>
int scale_each_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars, bool mont, void* d_out, int form, uint32_t* bad, double* ms) {
    typedef typename GroupOf<F>::Ops G;
    DevBuf sum, flag, tab; int rc;
    if ((rc = sum.alloc(ctx, (size_t)n * sizeof(XYZZ<F>))) || (rc = flag.alloc(ctx, 4)) || (form == 0 && (rc = tab.alloc(ctx, (size_t)WIN_ROWS * n * sizeof(typename G::Acc))))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(flag.p, 0xff, 4, ctx->stream));
    const clk::time_point t0 = clk::now();
    const F b = curve_b_host((const F*)nullptr);
    if (form == 0) hipLaunchKernelGGL((zkc_scale_each<G, 0>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const uint32_t*)d_points, (const uint32_t*)d_scalars, n, mont ? 1 : 0, b,
                                      (uint32_t*)tab.p, (XYZZ<F>*)sum.p, (uint32_t*)flag.p);
    else hipLaunchKernelGGL((zkc_scale_each<G, 1>), dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const uint32_t*)d_points, (const uint32_t*)d_scalars, n, mont ? 1 : 0, b,
                            (uint32_t*)nullptr, (XYZZ<F>*)sum.p, (uint32_t*)flag.p);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(bad, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const clk::time_point t1 = clk::now();
    if (ms) ms[0] = ms_since(t0, t1);
    if (*bad != NONE) return ZKC_OK;
    rc = fixed_affine<F>(ctx, (const XYZZ<F>*)sum.p, n, d_out, mont);
    if (ms) ms[1] = ms_since(t1);
    return rc;
}

template <class F>
int scale_each_entry(const char* name, zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out, int form) {
    if (!ctx || !d_points || !d_scalars32 || !d_out || n == 0 || form < 0 || form > 1) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, std::string(name) + ": bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t bad = NONE;
    g_each_ms[0] = g_each_ms[1] = 0;
    const int rc = scale_each_dev<F>(ctx, d_points, n, d_scalars32, mont != 0, d_out, form, &bad, g_each_ms);
    if (rc) return rc;
    if (bad != NONE) return zkc_fail(ctx, ZKC_ERR_FORMAT, std::string(name) + ": element " + std::to_string(bad) + " has a coordinate >= q, a point off the " + GroupOf<F>::curve + " or a scalar >= r");
    return ZKC_OK;
}

// ---- scalars on the host ----
// a^e for a secret a; the running square is cleared, the result is the caller's to clear
void fr_pow_u64(Fr& r, const Fr& a, uint64_t e) { SecretFr b; b.f = a; r = Fr::one(); for (; e; e >>= 1) { if (e & 1) r = r * b.f; b.f = b.f * b.f; } }
// k * p by double-and-add (xyzz_mul's loop, zkc_curve.h).  secret: the accumulator, whose path through the group spells the scalar, is cleared before the stack frame goes
template <class F> Affine<F> host_mul(const Affine<F>& p, const uint32_t k[8], bool secret = true) {
    XYZZ<F> r = xyzz_mul(XYZZ<F>::from_affine(p), k);
    const Affine<F> out = xyzz_to_affine(r);
    if (secret) Secret::wipe(&r, sizeof r);
    return out;
}

// the three secrets of a contribution and what the chunks need of them
struct Waste {
    Secret std[3];                               // tau', alpha', beta', standard form
    SecretFr m[3];                               // ... Montgomery form
    Fr pw[POW_ROWS + MULT_ROWS];                 // tau'^(2^k), then 1, alpha', beta'
    ~Waste() { Secret::wipe(pw, sizeof pw); }
};
// the table zkc_tau_scalars reads, from the Montgomery forms of W: of a contribution, and of the hook zkc_debug_tau_scalars_dev (whose multiplier sits in alpha's row)
void fill_power_table(Waste& W) {
    W.pw[0] = W.m[0].f; for (int k = 1; k < POW_ROWS; k++) W.pw[k] = W.pw[k - 1] * W.pw[k - 1];
    W.pw[POW_ROWS] = Fr::one(); W.pw[POW_ROWS + 1] = W.m[1].f; W.pw[POW_ROWS + 2] = W.m[2].f;
}

int fail(zkc_ctx* ctx, char* err, size_t errlen, int code, const std::string& m) { if (ctx) zkc_fail(ctx, code, m); return err_out(err, errlen, code, m); }

// ---- the record ----
// the five points and the three proofs of knowledge of a record as a hash takes them: U(tauG1) U(tauG2) U(alphaG1) U(betaG1) U(betaG2), then per key U(g1_s) U(g1_sx)
// U(g2_spx), then the transcript: 1280 bytes.  false: a coordinate >= q
constexpr size_t PUBKEY = 64 + 128 + 64 + 64 + 128 + 3 * 256 + 64;
struct FivePoints { G1Affine tauG1; G2Affine tauG2; G1Affine alphaG1, betaG1; G2Affine betaG2; };
struct Pok { G1Affine s, sx; G2Affine spx; };
bool rd_five(FivePoints& f, const uint8_t* p) { return rd_g1_mont(f.tauG1, p) & rd_g2_mont(f.tauG2, p + 64) & rd_g1_mont(f.alphaG1, p + 192) & rd_g1_mont(f.betaG1, p + 256) & rd_g2_mont(f.betaG2, p + 320); }
void wr_five(uint8_t* p, const FivePoints& f) { wr_g1_mont(p, f.tauG1); wr_g2_mont(p + 64, f.tauG2); wr_g1_mont(p + 192, f.alphaG1); wr_g1_mont(p + 256, f.betaG1); wr_g2_mont(p + 320, f.betaG2); }
bool rd_pok(Pok& k, const uint8_t* p) { return rd_g1_mont(k.s, p) & rd_g1_mont(k.sx, p + 64) & rd_g2_mont(k.spx, p + 128); }
void pubkey_of(uint8_t out[PUBKEY], const FivePoints& f, const Pok k[3], const uint8_t transcript[64]) {
    unc_g1(out, f.tauG1); unc_g2(out + 64, f.tauG2); unc_g1(out + 192, f.alphaG1); unc_g1(out + 256, f.betaG1); unc_g2(out + 320, f.betaG2);
    for (int i = 0; i < 3; i++) { uint8_t* q = out + 448 + 256 * i; unc_g1(q, k[i].s); unc_g1(q + 64, k[i].sx); unc_g2(q + 128, k[i].spx); }
    memcpy(out + 448 + 768, transcript, 64);
}
bool pubkey_bytes(const parse::PcRecord& r, uint8_t out[PUBKEY]) {
    FivePoints f; Pok k[3];
    if (!rd_five(f, r.tauG1) || !rd_pok(k[0], r.pok[0]) || !rd_pok(k[1], r.pok[1]) || !rd_pok(k[2], r.pok[2])) return false;
    pubkey_of(out, f, k, r.transcript);
    return true;
}
// H("zkc-ptau" || power as u32 || pubkey_0 .. pubkey_(k - 1)) left open, for the transcript of record k or the hash of a contribution
bool hash_prefix(parse::Blake2b& h, uint32_t power, const parse::PcSection& s, size_t k) {
    h.update("zkc-ptau", 8); h.update(&power, 4);
    for (size_t j = 0; j < k; j++) { uint8_t pk[PUBKEY]; if (!pubkey_bytes(s.rec[j], pk)) return false; h.update(pk, PUBKEY); }
    return true;
}
// ... closed over the three (g1_s, g1_sx) of the record being made or checked
void transcript_close(parse::Blake2b& h, const Pok k[3], uint8_t out[64]) {
    for (int i = 0; i < 3; i++) { uint8_t u[64]; unc_g1(u, k[i].s); h.update(u, 64); unc_g1(u, k[i].sx); h.update(u, 64); }
    h.final(out);
}
// the G2 challenge of key i (0 tau, 1 alpha, 2 beta): the hash to G2 of phase 2 (zkc_debug_phase2_challenge_g2) on BLAKE2b(transcript || i)
G2Affine challenge_of(const uint8_t transcript[64], int i) {
    uint8_t in[65], t[64], out[128]; memcpy(in, transcript, 64); in[64] = (uint8_t)i;
    parse::blake2b512(in, 65, t);
    zkc_debug_phase2_challenge_g2(t, out);
    G2Affine p; (void)rd_g2_std(p, out);
    return p;
}

// a file's header, records and five points
struct Chain {
    parse::Ptau pt; std::vector<uint8_t> sec7; parse::PcSection pc; FivePoints five;
};
bool read_section7(const parse::Ptau& pt, std::vector<uint8_t>& sec7, parse::PcSection& pc, std::string& why) {
    if (!pt.have[7]) { sec7.assign(4, 0); return parse::ptau_contrib_section(sec7.data(), 4, pc, why); }       // a file without the section has no contribution
    if (pt.len[7] > (1ull << 30)) { why = "ptau: section 7 is larger than 1 GiB"; return false; }
    sec7.resize((size_t)pt.len[7]);
    if (sec7.size() && !parse::ptau_pread(pt, sec7.data(), sec7.size(), pt.off[7])) { why = "ptau: short read in section 7"; return false; }
    return parse::ptau_contrib_section(sec7.data(), sec7.size(), pc, why);
}
bool read_five(const parse::Ptau& pt, FivePoints& f, std::string& why) {
    uint8_t b[128];
    if (!parse::ptau_read(pt, 2, 1, 1, b, why)) return false; bool ok = rd_g1_mont(f.tauG1, b);
    if (!parse::ptau_read(pt, 3, 1, 1, b, why)) return false; ok &= rd_g2_mont(f.tauG2, b);
    if (!parse::ptau_read(pt, 4, 0, 1, b, why)) return false; ok &= rd_g1_mont(f.alphaG1, b);
    if (!parse::ptau_read(pt, 5, 0, 1, b, why)) return false; ok &= rd_g1_mont(f.betaG1, b);
    if (!parse::ptau_read(pt, 6, 0, 1, b, why)) return false; ok &= rd_g2_mont(f.betaG2, b);
    if (!ok) why = "ptau: tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0] or betaG2 has a coordinate >= q";
    return ok;
}
bool read_chain(const char* path, Chain& c, std::string& why) {
    return parse::ptau_open(path, c.pt, why, false) && read_section7(c.pt, c.sec7, c.pc, why) && read_five(c.pt, c.five, why);
}
template <class A> bool same_point(const A& a, const A& b) { return a.x == b.x && a.y == b.y; }

// ---- one section of a contribution ----
template <class F> uint32_t first_infinity(const Affine<F>* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i].is_inf()) return (uint32_t)i; return NONE; }

struct DevWaste {                                 // the device's copy of the power table, and the chunk's scalars: cleared on the stream before they are released
    zkc_ctx* ctx = nullptr; DevBuf pw, ks; size_t ks_bytes = 0;
    ~DevWaste() {
        if (!ctx) return;
        if (pw.p) (void)hipMemsetAsync(pw.p, 0, sizeof(Fr) * (POW_ROWS + MULT_ROWS), ctx->stream);
        if (ks.p) (void)hipMemsetAsync(ks.p, 0, ks_bytes, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

// d_ks[i] = (mult < 0 ? 1 : multiplier `mult` of the table) * tau'^(first + i), i < np, from the uploaded table d_pw, on the context's stream: the one launch of
// zkc_tau_scalars, for a chunk of a contribution and for the hook.  first + np <= 2^32 is the caller's to keep.  false: the launch failed
bool launch_tau_scalars(zkc_ctx* ctx, const void* d_pw, int mult, uint64_t first, uint32_t np, void* d_ks) {
    hipLaunchKernelGGL(zkc_tau_scalars, dim3((np + 255) / 256), dim3(256), 0, ctx->stream, (const Fr*)d_pw, (uint32_t)(POW_ROWS + (mult < 0 ? 0 : mult)), first, np, (uint32_t*)d_ks);
    return hipGetLastError() == hipSuccess;
}

// section `sec` of the input times mult * tau'^i, appended to the output.  keep[j] (j < nkeep) = the new point of index keep_idx[j].  rc != 0: err is written
template <class F>
int section_pass(zkc_ctx* ctx, const parse::Ptau& pt, parse::PtauOut& o, int sec, const Waste& W, int mult /* -1: none, 1: alpha', 2: beta' */, bool tau_powers, uint32_t chunk, int form,
                 DevWaste& dw, Affine<F>* keep, const uint64_t* keep_idx, int nkeep, char* err, size_t errlen) {
    typedef GroupOf<F> G;
    constexpr size_t PT = sizeof(Affine<F>);
    const uint64_t npts = parse::ptau_section_points(sec, pt.power);
    const uint32_t cap = (uint32_t)std::min<uint64_t>(chunk, npts);
    std::vector<Affine<F>> buf(cap);
    DevBuf d_pts; int rc; std::string why;
    if (ctx && (rc = d_pts.alloc(ctx, (size_t)cap * PT))) return err_out(err, errlen, rc, zkc_last_error(ctx));
    if (!parse::ptau_out_section_head(o, sec, npts * PT, why)) return fail(ctx, err, errlen, ZKC_ERR_GENERIC, why);
    SecretFr mul; mul.f = mult < 0 ? Fr::one() : W.m[mult].f;
    SecretFr unit_tau; unit_tau.f = tau_powers ? W.m[0].f : Fr::one();
    for (uint64_t c0 = 0; c0 < npts; c0 += chunk) {
        const uint32_t np = (uint32_t)std::min<uint64_t>(chunk, npts - c0);
        clk::time_point t0 = clk::now();
        if (!parse::ptau_read(pt, sec, c0, np, buf.data(), why)) return fail(ctx, err, errlen, ZKC_ERR_FORMAT, why);
        g_con_ms[0] += ms_since(t0);
        t0 = clk::now();
        uint32_t bad = first_infinity<F>(buf.data(), np);
        if (ctx) {
            if (hipMemcpy(d_pts.p, buf.data(), (size_t)np * PT, hipMemcpyHostToDevice) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_contribute: upload"), zkc_last_error(ctx));
            if (!launch_tau_scalars(ctx, dw.pw.p, mult, tau_powers ? c0 : 0ull, np, dw.ks.p)) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_contribute: scalar kernel"), zkc_last_error(ctx));
            g_con_ms[1] += ms_since(t0);
            double kms[2] = {0, 0}; uint32_t kbad = NONE;
            if ((rc = scale_each_dev<F>(ctx, d_pts.p, np, dw.ks.p, true, d_pts.p, form, &kbad, kms))) return err_out(err, errlen, rc, zkc_last_error(ctx));
            g_con_ms[G::g2 ? 3 : 2] += kms[0];
            bad = std::min(bad, kbad);
            t0 = clk::now();
            if (bad == NONE && hipMemcpy(buf.data(), d_pts.p, (size_t)np * PT, hipMemcpyDeviceToHost) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_contribute: download"), zkc_last_error(ctx));
            g_con_ms[4] += kms[1] + ms_since(t0);
        } else {
            bad = std::min(bad, host_first_bad<F>(buf.data(), np));
            g_con_ms[1] += ms_since(t0);
            t0 = clk::now();
            if (bad == NONE)
                par_chunks(np, 16, [&](size_t a, size_t b) {
                    SecretFr s, pw; fr_pow_u64(pw.f, unit_tau.f, c0 + a); s.f = mul.f * pw.f;
                    for (size_t i = a; i < b; i++) { Secret k; fp_to_std<FrParams>(k.v, s.f); buf[i] = host_mul(buf[i], k.v); s.f = s.f * unit_tau.f; }
                });
            g_con_ms[G::g2 ? 3 : 2] += ms_since(t0);
        }
        if (bad != NONE)
            return fail(ctx, err, errlen, ZKC_ERR_FORMAT, "ptau: section " + std::to_string(sec) + " point " + std::to_string(c0 + bad) + " has a coordinate >= q, is not on the " + G::curve +
                        " or is at infinity");
        for (int j = 0; j < nkeep; j++) if (keep_idx[j] >= c0 && keep_idx[j] < c0 + np) keep[j] = buf[keep_idx[j] - c0];
        t0 = clk::now();
        if (!parse::ptau_out_bytes(o, buf.data(), (size_t)np * PT, why)) return fail(ctx, err, errlen, ZKC_ERR_GENERIC, why);
        g_con_ms[5] += ms_since(t0);
    }
    return ZKC_OK;
}

// the body of zkc_ptau_contribute and of the hook
int contribute(const char* fn, zkc_ctx* ctx, const char* src_path, const char* dst_path, const uint8_t* secrets96, const char* name, uint32_t chunk, int form, uint8_t* hash64,
               char* err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!src_path || !dst_path || form < 0 || form > 1) return fail(ctx, err, errlen, ZKC_ERR_BAD_ARG, std::string(fn) + ": bad argument");
    for (double& m : g_con_ms) m = 0;
    if (!chunk) chunk = CHUNK;
    Waste W;
    if (secrets96) for (int i = 0; i < 3; i++) memcpy(W.std[i].v, secrets96 + 32 * i, 32);
    else for (int i = 0; i < 3; i++) do zkc_random_scalars((uint8_t*)W.std[i].v, 1); while (std_is_zero(W.std[i]));
    for (int i = 0; i < 3; i++) {
        if (std_is_zero(W.std[i]) || !fp_std_lt_p<FrParams>(W.std[i])) return fail(ctx, err, errlen, ZKC_ERR_BAD_ARG, std::string(fn) + ": tau', alpha' and beta' must be in [1, r)");
        W.m[i].f = fp_from_std<FrParams>(W.std[i].v);
    }
    fill_power_table(W);
    clk::time_point t0 = clk::now();
    Chain in; std::string why;
    if (!read_chain(src_path, in, why)) return fail(ctx, err, errlen, ZKC_ERR_FORMAT, std::string(fn) + ": " + why);
    g_con_ms[0] += ms_since(t0);
    const size_t name_len = name ? std::min<size_t>(strlen(name), 64) : 0;
    const size_t params_len = name_len ? 2 + name_len : 0, rec_len = parse::PC_FIXED + params_len;
    parse::PtauOut o;
    if (!parse::ptau_out_open(dst_path, 7, o, why)) return fail(ctx, err, errlen, ZKC_ERR_GENERIC, why);
    { uint8_t s1[44];
      if (!parse::ptau_pread(in.pt, s1, 44, in.pt.off[1])) return fail(ctx, err, errlen, ZKC_ERR_FORMAT, "ptau: cannot read section 1");
      if (!parse::ptau_out_section_head(o, 1, 44, why) || !parse::ptau_out_bytes(o, s1, 44, why)) return fail(ctx, err, errlen, ZKC_ERR_GENERIC, why); }
    FivePoints after; G1Affine k2[1]; G2Affine k3[1], k6[1]; G1Affine k4[1], k5[1];
    const uint64_t one_idx[1] = {1}, zero_idx[1] = {0};
    int rc;
    {
        DevWaste dw;
        std::unique_lock<std::recursive_mutex> lock;
        if (ctx) {
            lock = std::unique_lock<std::recursive_mutex>(ctx->mu);
            if (hipSetDevice(ctx->device) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, std::string(fn) + ": hipSetDevice"), zkc_last_error(ctx));
            dw.ctx = ctx; dw.ks_bytes = (size_t)std::min<uint64_t>(chunk, 2ull << in.pt.power) * 32;
            if ((rc = dw.pw.alloc(ctx, sizeof(Fr) * (POW_ROWS + MULT_ROWS))) || (rc = dw.ks.alloc(ctx, dw.ks_bytes))) return err_out(err, errlen, rc, zkc_last_error(ctx));
            if (hipMemcpy(dw.pw.p, W.pw, sizeof(Fr) * (POW_ROWS + MULT_ROWS), hipMemcpyHostToDevice) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, std::string(fn) + ": upload"), zkc_last_error(ctx));
        }
        if ((rc = section_pass<Fq>(ctx, in.pt, o, 2, W, -1, true, chunk, form, dw, k2, one_idx, 1, err, errlen)) ||
            (rc = section_pass<Fq2>(ctx, in.pt, o, 3, W, -1, true, chunk, form, dw, k3, one_idx, 1, err, errlen)) ||
            (rc = section_pass<Fq>(ctx, in.pt, o, 4, W, 1, true, chunk, form, dw, k4, zero_idx, 1, err, errlen)) ||
            (rc = section_pass<Fq>(ctx, in.pt, o, 5, W, 2, true, chunk, form, dw, k5, zero_idx, 1, err, errlen)) ||
            (rc = section_pass<Fq2>(ctx, in.pt, o, 6, W, 2, false, chunk, form, dw, k6, zero_idx, 1, err, errlen))) return rc;
    }
    after.tauG1 = k2[0]; after.tauG2 = k3[0]; after.alphaG1 = k4[0]; after.betaG1 = k5[0]; after.betaG2 = k6[0];
    // ---- the record: three proofs of knowledge, the transcript, the hash ----
    t0 = clk::now();
    Pok pok[3];
    uint8_t prefix[64];
    { parse::Blake2b h; if (!hash_prefix(h, in.pt.power, in.pc, in.pc.rec.size())) return fail(ctx, err, errlen, ZKC_ERR_FORMAT, std::string(fn) + ": a recorded point has a coordinate >= q"); h.final(prefix); }
    for (int i = 0; i < 3; i++) {
        // the scalar of g1_s: drawn from the secrets and the records so far, so that given secrets give one contribution; it is as hidden as they are
        Secret s; uint8_t d[64];
        { parse::Blake2b h; h.update("zkc-ptau-pok", 12); for (int j = 0; j < 3; j++) h.update(W.std[j].v, 32); const uint8_t ib = (uint8_t)i; h.update(&ib, 1); h.update(prefix, 64); h.final(d); }
        memcpy(s.v, d, 32); Secret::wipe(d, 64);
        s.v[7] &= 0x1fffffffu;                                  // below 2^253 < r
        if (std_is_zero(s)) s.v[0] = 1;
        pok[i].s = host_mul(g1_generator(), s.v); pok[i].sx = host_mul(pok[i].s, W.std[i].v);
    }
    uint8_t transcript[64];
    { parse::Blake2b h; (void)hash_prefix(h, in.pt.power, in.pc, in.pc.rec.size()); transcript_close(h, pok, transcript); }
    for (int i = 0; i < 3; i++) pok[i].spx = host_mul(challenge_of(transcript, i), W.std[i].v);
    std::vector<uint8_t> sec7(in.sec7.size() + rec_len);
    memcpy(sec7.data(), in.sec7.data(), in.sec7.size());
    const uint32_t cnt = in.pc.n + 1; memcpy(sec7.data(), &cnt, 4);
    uint8_t* r = sec7.data() + in.sec7.size();
    wr_five(r, after);
    for (int i = 0; i < 3; i++) { uint8_t* q = r + parse::PC_POINTS + parse::PC_POK * (size_t)i; wr_g1_mont(q, pok[i].s); wr_g1_mont(q + 64, pok[i].sx); wr_g2_mont(q + 128, pok[i].spx); }
    uint8_t* tr = r + parse::PC_POINTS + 3 * parse::PC_POK; memcpy(tr, transcript, 64);
    const uint32_t type = parse::PC_TYPE_PLAIN, pl = (uint32_t)params_len; memcpy(tr + 64, &type, 4); memcpy(tr + 68, &pl, 4);
    if (name_len) { tr[72] = 0x01; tr[73] = (uint8_t)name_len; memcpy(tr + 74, name, name_len); }
    if (!parse::ptau_out_section(o, 7, sec7.data(), sec7.size(), why) || !parse::ptau_out_commit(o, why)) return fail(ctx, err, errlen, ZKC_ERR_GENERIC, why);
    if (hash64) {
        parse::Blake2b h; (void)hash_prefix(h, in.pt.power, in.pc, in.pc.rec.size());
        uint8_t pk[PUBKEY]; pubkey_of(pk, after, pok, transcript); h.update(pk, PUBKEY); h.final(hash64);
    }
    g_con_ms[5] += ms_since(t0);
    return ZKC_OK;
}

}  // namespace

extern "C" int zkc_g1_scale_each_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out) {
    return scale_each_entry<Fq>("zkc_g1_scale_each_dev", ctx, d_points, n, d_scalars32, mont, d_out, 0);
}
extern "C" int zkc_g2_scale_each_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out) {
    return scale_each_entry<Fq2>("zkc_g2_scale_each_dev", ctx, d_points, n, d_scalars32, mont, d_out, 0);
}
extern "C" int zkc_debug_scale_each_dev(zkc_ctx* ctx, int g2, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out, int form) {
    return g2 ? scale_each_entry<Fq2>("zkc_debug_scale_each_dev", ctx, d_points, n, d_scalars32, mont, d_out, form)
              : scale_each_entry<Fq>("zkc_debug_scale_each_dev", ctx, d_points, n, d_scalars32, mont, d_out, form);
}
extern "C" int zkc_debug_scale_each_stats(double ms[2]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    ms[0] = g_each_ms[0]; ms[1] = g_each_ms[1];
    return ZKC_OK;
}
extern "C" uint64_t zkc_debug_scale_each_work_bytes(int g2, uint32_t n, int form) {
    return g2 ? scale_each_work_bytes<Fq2>(n, form) : scale_each_work_bytes<Fq>(n, form);
}

extern "C" int zkc_ptau_new(const char* path, uint32_t power, char* err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!path) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_ptau_new: bad argument");
    if (power < 1 || power > parse::PTAU_MAX_PREPARE_POWER) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_ptau_new: power " + std::to_string(power) + " outside [1, 27]");
    parse::PtauOut o; std::string why;
    if (!parse::ptau_out_open(path, 7, o, why)) return err_out(err, errlen, ZKC_ERR_GENERIC, why);
    uint8_t s1[44]; const uint32_t n8 = 32; memcpy(s1, &n8, 4); memcpy(s1 + 4, parse::kFqP, 32); memcpy(s1 + 36, &power, 4); memcpy(s1 + 40, &power, 4);
    if (!parse::ptau_out_section(o, 1, s1, 44, why)) return err_out(err, errlen, ZKC_ERR_GENERIC, why);
    constexpr size_t PIECE = 1u << 20;
    std::vector<uint8_t> g1(PIECE), g2(PIECE);
    wr_g1_mont(g1.data(), g1_generator()); wr_g2_mont(g2.data(), g2_generator());
    for (size_t at = 64; at < PIECE; at += 64) memcpy(&g1[at], g1.data(), 64);
    for (size_t at = 128; at < PIECE; at += 128) memcpy(&g2[at], g2.data(), 128);
    for (int sec = 2; sec <= 6; sec++) {
        const bool two = parse::ptau_point_bytes(sec) == 128;
        uint64_t left = parse::ptau_section_points(sec, power) * parse::ptau_point_bytes(sec);
        if (!parse::ptau_out_section_head(o, sec, left, why)) return err_out(err, errlen, ZKC_ERR_GENERIC, why);
        while (left) { const size_t k = (size_t)std::min<uint64_t>(PIECE, left); if (!parse::ptau_out_bytes(o, (two ? g2 : g1).data(), k, why)) return err_out(err, errlen, ZKC_ERR_GENERIC, why); left -= k; }
    }
    const uint32_t none = 0;
    if (!parse::ptau_out_section(o, 7, &none, 4, why) || !parse::ptau_out_commit(o, why)) return err_out(err, errlen, ZKC_ERR_GENERIC, why);
    return ZKC_OK;
}

extern "C" int zkc_ptau_contribute(zkc_ctx* ctx, const char* src_path, const char* dst_path, const uint8_t* secrets96, const char* name, uint8_t* hash64, char* err, size_t errlen) {
    return contribute("zkc_ptau_contribute", ctx, src_path, dst_path, secrets96, name, 0, 0, hash64, err, errlen);
}
extern "C" int zkc_debug_ptau_contribute(zkc_ctx* ctx, const char* src_path, const char* dst_path, const uint8_t* secrets96, const char* name, uint32_t chunk_points, int form,
                                         uint8_t* hash64, char* err, size_t errlen) {
    return contribute("zkc_debug_ptau_contribute", ctx, src_path, dst_path, secrets96, name, chunk_points, form, hash64, err, errlen);
}

// the scalars of a chunk on their own: the table of fill_power_table with mult in alpha's row, the launch of launch_tau_scalars, a copy to the caller's buffer; the table
// and the work copy of the scalars are cleared on the stream as a contribution's are (DevWaste)
extern "C" int zkc_debug_tau_scalars_dev(zkc_ctx* ctx, const uint8_t* tau32, const uint8_t* mult32, uint64_t first, uint32_t n, void* d_out) {
    const char* const fn = "zkc_debug_tau_scalars_dev";
    if (!ctx || !tau32 || !mult32 || !d_out || n == 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, std::string(fn) + ": bad argument");
    if (first > (1ull << 32) || first + n > (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, std::string(fn) + ": first + n exceeds 2^32, the exponents the power table serves");
    Waste W;
    memcpy(W.std[0].v, tau32, 32); memcpy(W.std[1].v, mult32, 32); W.std[2].v[0] = 1;
    for (int i = 0; i < 3; i++) {
        if (std_is_zero(W.std[i]) || !fp_std_lt_p<FrParams>(W.std[i])) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, std::string(fn) + ": tau and mult must be in [1, r)");
        W.m[i].f = fp_from_std<FrParams>(W.std[i].v);
    }
    fill_power_table(W);
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevWaste dw; int rc;
    dw.ctx = ctx; dw.ks_bytes = (size_t)n * 32;
    if ((rc = dw.pw.alloc(ctx, sizeof(Fr) * (POW_ROWS + MULT_ROWS))) || (rc = dw.ks.alloc(ctx, dw.ks_bytes))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpy(dw.pw.p, W.pw, sizeof(Fr) * (POW_ROWS + MULT_ROWS), hipMemcpyHostToDevice));
    if (!launch_tau_scalars(ctx, dw.pw.p, 1, first, n, dw.ks.p)) return zkc_fail(ctx, ZKC_ERR_HIP, std::string(fn) + ": scalar kernel");
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_out, dw.ks.p, dw.ks_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKC_OK;
}

extern "C" int zkc_ptau_contribute_stats(double ms[6]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 6; i++) ms[i] = g_con_ms[i];
    return ZKC_OK;
}

extern "C" int zkc_ptau_contributions(const char* path, uint32_t* n, void* records_out, size_t* records_len, char* err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!path || !n || !records_len) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_ptau_contributions: bad argument");
    parse::Ptau pt; std::vector<uint8_t> sec7; parse::PcSection pc; std::string why;
    if (!parse::ptau_open(path, pt, why, false) || !read_section7(pt, sec7, pc, why)) return err_out(err, errlen, ZKC_ERR_FORMAT, why);
    *n = pc.n;
    const size_t room = *records_len; *records_len = pc.records_len;
    if (!records_out) return ZKC_OK;
    if (room < pc.records_len) return err_out(err, errlen, ZKC_ERR_SHORT_BUFFER, "zkc_ptau_contributions: records buffer too short");
    if (pc.records_len) memcpy(records_out, pc.records, pc.records_len);
    return ZKC_OK;
}

extern "C" int zkc_ptau_verify_contributions(zkc_ctx* ctx, const char* prev_path, const char* next_path, const uint8_t* seed32, uint32_t* n_new, char* err, size_t errlen) {
    if (n_new) *n_new = 0;
    if (err && errlen) err[0] = 0;
    if (!next_path) return err_out(err, errlen, -ZKC_ERR_BAD_ARG, "zkc_ptau_verify_contributions: bad argument");
    auto invalid = [&](const std::string& m) { return err_out(err, errlen, 0, m); };
    // ---- 1 ----
    Chain A, B; std::string why;
    if (!read_chain(next_path, B, why)) return invalid("check 1: the next file does not parse: " + why);
    if (prev_path) {
        if (!read_chain(prev_path, A, why)) return invalid("check 1: the previous file does not parse: " + why);
        if (A.pt.power != B.pt.power) return invalid("check 1: the files have different powers (" + std::to_string(A.pt.power) + " and " + std::to_string(B.pt.power) + ")");
    } else {
        A.five.tauG1 = A.five.alphaG1 = A.five.betaG1 = g1_generator(); A.five.tauG2 = A.five.betaG2 = g2_generator();
    }
    // ---- 2 ----
    if (B.pc.n < A.pc.n || B.pc.records_len < A.pc.records_len) return invalid("check 2: the next file has fewer contributions than the previous file");
    {
        size_t alen = 0; for (uint32_t k = 0; k < A.pc.n; k++) alen += B.pc.rec[k].rec_len;
        if (alen != A.pc.records_len || (alen && memcmp(A.pc.records, B.pc.records, alen))) return invalid("check 2: the previous file's contributions are not a prefix of the next file's");
    }
    if (n_new) *n_new = B.pc.n - A.pc.n;
    // ---- 3 ----
    FivePoints cur = A.five;
    if (!pairing::g1_on_curve(cur.tauG1) || !pairing::g1_on_curve(cur.alphaG1) || !pairing::g1_on_curve(cur.betaG1) || !pairing::g2_in_subgroup(cur.tauG2) || !pairing::g2_in_subgroup(cur.betaG2) ||
        cur.tauG1.is_inf() || cur.alphaG1.is_inf() || cur.betaG1.is_inf() || cur.tauG2.is_inf() || cur.betaG2.is_inf())
        return invalid("check 3: a point the chain starts from (the previous file's tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0], betaG2) is not in its group");
    const G1Affine G1 = g1_generator(); const G2Affine G2 = g2_generator();
    static const char* const KEY[3] = {"tau", "alpha", "beta"};
    for (uint32_t k = A.pc.n; k < B.pc.n; k++) {
        const parse::PcRecord& r = B.pc.rec[k]; const std::string at = "check 3, contribution " + std::to_string(k) + ": ";
        FivePoints f; Pok pok[3];
        if (!rd_five(f, r.tauG1) || !rd_pok(pok[0], r.pok[0]) || !rd_pok(pok[1], r.pok[1]) || !rd_pok(pok[2], r.pok[2])) return invalid(at + "a coordinate >= q");
        // 3.1
        const struct { const G1Affine* p; const char* name; } g1s[3] = {{&f.tauG1, "tauG1"}, {&f.alphaG1, "alphaG1"}, {&f.betaG1, "betaG1"}};
        for (const auto& e : g1s) if (e.p->is_inf() || !pairing::g1_on_curve(*e.p)) return invalid(at + e.name + " is at infinity or not on the curve");
        const struct { const G2Affine* p; const char* name; } g2s[2] = {{&f.tauG2, "tauG2"}, {&f.betaG2, "betaG2"}};
        for (const auto& e : g2s) if (e.p->is_inf() || !pairing::g2_in_subgroup(*e.p)) return invalid(at + e.name + " is at infinity or not in G2");
        for (int i = 0; i < 3; i++) {
            if (pok[i].s.is_inf() || !pairing::g1_on_curve(pok[i].s)) return invalid(at + "g1_s of " + KEY[i] + " is at infinity or not on the curve");
            if (pok[i].sx.is_inf() || !pairing::g1_on_curve(pok[i].sx)) return invalid(at + "g1_sx of " + KEY[i] + " is at infinity or not on the curve");
            if (pok[i].spx.is_inf() || !pairing::g2_in_subgroup(pok[i].spx)) return invalid(at + "g2_spx of " + KEY[i] + " is at infinity or not in G2");
        }
        // 3.2
        uint8_t tr[64];
        { parse::Blake2b h; if (!hash_prefix(h, B.pt.power, B.pc, k)) return invalid(at + "an earlier record holds a coordinate >= q"); transcript_close(h, pok, tr); }
        if (memcmp(tr, r.transcript, 64)) return invalid(at + "the stored transcript is not the recomputed one");
        // 3.3, 3.4
        const G1Affine* before[3] = {&cur.tauG1, &cur.alphaG1, &cur.betaG1}; const G1Affine* after[3] = {&f.tauG1, &f.alphaG1, &f.betaG1};
        G2Affine sp[3];
        for (int i = 0; i < 3; i++) {
            sp[i] = challenge_of(tr, i);
            if (!pairing::same_ratio(pok[i].s, pok[i].sx, sp[i], pok[i].spx)) return invalid(at + "the proof of knowledge of " + KEY[i] + " fails: sameRatio(g1_s, g1_sx; g2_sp, g2_spx)");
        }
        for (int i = 0; i < 3; i++)
            if (!pairing::same_ratio(*before[i], *after[i], sp[i], pok[i].spx)) return invalid(at + "the chain step of " + KEY[i] + " fails: sameRatio(" + KEY[i] + "G1 before, after; g2_sp, g2_spx)");
        // 3.5
        if (!pairing::same_ratio(G1, f.tauG1, G2, f.tauG2)) return invalid(at + "tauG1 and tauG2 hold different tau: sameRatio(G1, tauG1; G2, tauG2) fails");
        if (!pairing::same_ratio(G1, f.betaG1, G2, f.betaG2)) return invalid(at + "betaG1 and betaG2 hold different beta: sameRatio(G1, betaG1; G2, betaG2) fails");
        cur = f;
    }
    // ---- 4 ----
    if (!same_point(cur.tauG1, B.five.tauG1) || !same_point(cur.tauG2, B.five.tauG2) || !same_point(cur.alphaG1, B.five.alphaG1) || !same_point(cur.betaG1, B.five.betaG1) ||
        !same_point(cur.betaG2, B.five.betaG2))
        return invalid(B.pc.n > A.pc.n ? "check 4: the last contribution's points are not the next file's tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0], betaG2"
                                       : "check 4: no new contribution, but the next file's tauG1[1], tauG2[1], alphaTauG1[0], betaTauG1[0] or betaG2 differs from the chain's start");
    // ---- 5 ----
    char verr[512]; verr[0] = 0;
    const int rc = zkc_ptau_verify(ctx, next_path, seed32, nullptr, nullptr, nullptr, verr, sizeof verr);
    if (rc < 0) return err_out(err, errlen, rc, std::string("zkc_ptau_verify_contributions: ") + verr);
    if (rc == 0) return invalid(std::string("check 5: ") + verr);
    return 1;
}
