// zkc_phase2.hip -- the phase-2 ceremony of a Groth16 key (include/zkcensus_phase2.h): the batch product k * P_i for n points and ONE scalar on the GPU (product code), and
// the host side built on it: zkc_zkey_contribute (snarkjs `zkey contribute`) and zkc_zkey_verify_contributions (the ceremony part of `zkey verify`).
//
// The kernel.  A contribution multiplies every point of sections 8 and 9 by the same 1 / delta': many bases, one scalar -- the opposite of every other batch product of
// the library (one base, many scalars: zkc_g1_mul_batch_dev, zkc_fixedbase_dev.hip).  One lane per point.  The scalar is recoded once on the host into its non-adjacent
// form (digits -1, 0, +1, no two neighbours non-zero, one in three non-zero on average) and reaches the kernel as two 256-bit masks in the launch arguments: the digits
// are wave-uniform, so is every branch on them, and no lane extracts a digit.  From the leading digit down: f29_acc_dbl on the accumulator, and on a non-zero digit the
// mixed addition f29_madd of +P_i or -P_i (negating an affine point is free: -y is computed once per lane).  No per-lane table: accumulator 36 registers, the point 27
// (x, y, -y).  Results leave as canonical XYZZ and become affine through the batched inversion of the fixed-base products (fixed_affine<Fq>).  The point check, the
// accumulator and the handling of the addition's exceptional cases are those of every kernel over the points of a file: zkc_point_ops.h.
//
// Why the incomplete addition is enough, and where it is not.  Write the recoding of k (0 < k < r) as digits d_t .. d_0 with d_t = +1, and m_j = sum_{i >= j} d_i 2^(i - j)
// for its prefixes: m_t = 1, m_0 = k, and |k - m_j 2^j| < 2^(j + 1) / 3 (a tail of a non-adjacent form is below two thirds of its leading power), so 0 < m_j < k / 2^j + 1.
// When digit d_j != 0 (j < t) is added the accumulator holds 2 m_(j+1) P_i, set at the leading digit and never added to there, and the addend is d_j P_i = +-P_i.  P_i has
// order r (the curve has prime order), so the addition is exceptional only if 2 m_(j+1) = +-1 or 0 (mod r).  2 m_(j+1) = m_j - d_j is even, positive and at most
// m_j + 1 <= k / 2^j + 2: for j >= 1 that is below r - 1, for j = 0 it is at most r.  An even number in (0, r] is neither 0 nor 1 mod r (r is odd), and it is -1 mod r only
// as r - 1 itself: j = 0, k - d_0 = r - 1, i.e. k = r - 2 with d_0 = -1 (r = 1 mod 4, so r - 2 = 3 mod 4 and its last digit IS -1).  So exactly one scalar below r meets
// the exceptional case, at its last digit, where the accumulator holds (r - 1) P = -P and -P is added: a doubling.  f29_madd's `false` return is handled for every digit
// (same point: double the accumulator; opposite points: infinity), which covers it; tests/test_gpu_phase2_scale.py has k = r - 2.
// A doubling never meets infinity: the group has odd order.  Inputs are checked for being on the curve, which on a curve of prime order is all there is to check.
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "zkc_prover.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_f29.h"
#include "zkc_f29_g1.h"
#include "zkc_point_ops.h"
#include "zkc_verify_host.h"
#include "zkc_phase2_parse.h"
#include "../../include/zkcensus_phase2.h"

using namespace zkc;

namespace {

// the non-adjacent form of the scalar: bit j of pos / neg = digit j is +1 / -1; top = the index of the leading digit (+1 for a positive scalar)
struct ScaleDigits { uint32_t pos[8], neg[8]; int top; };

// out[i] = k * pts[i] as canonical XYZZ (infinity: all zero).  *bad (initialised to 0xffffffff) = the smallest index of a point with a coordinate >= q or off the curve: the
// check of zkc_point_ops.h, fused here so that a contribution makes one pass over its points.
__global__ void __launch_bounds__(64)
zkc_p2_scale_g1(const uint32_t* __restrict__ pts, uint32_t n, ScaleDigits d, int mont, XYZZ<Fq>* __restrict__ out, uint32_t* __restrict__ bad) {
    typedef G1Ops G;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[16]; load_words<16>(w, pts + 16 * (size_t)i);
    XYZZ<Fq> o = XYZZ<Fq>::inf();
    if (all_zero<16>(w)) { out[i] = o; return; }
    if (!coords_below_q<G>(w)) { atomicMin(bad, i); out[i] = o; return; }
    if (!mont) {
        const Fq X = fp_from_std<FqParams>(w), Y = fp_from_std<FqParams>(w + 8);
#pragma unroll
        for (int k = 0; k < 8; k++) { w[k] = X.v[k]; w[8 + k] = Y.v[k]; }
    }
    if (!on_curve<G>(w, fp_from_u32<FqParams>(3))) { atomicMin(bad, i); out[i] = o; return; }
    // x is entered once and y twice, as y and -y (below 1.2 p each: well inside what f29_madd takes, below 32 p), and the digit picks between the two.  Not G::enter for
    // P and again for -P: that form takes 245 registers and leaves two waves per SIMD where this one leaves three
    const Fq nY = fp_neg(fq_of(w + 8));
    G::Pt p; uint32_t py[9], pny[9];
    f29_enter_fq(p.x, w); f29_enter_fq(py, w + 8); f29_enter_fq(pny, nY.v);
#pragma unroll
    for (int k = 0; k < 9; k++) p.y[k] = py[k];
    G::Acc acc; G::set(acc, p);
    bool inf = false;
    for (int j = d.top - 1; j >= 0; j--) {
        G::dbl(acc);
        const uint32_t sh = (uint32_t)j & 31u;
        const bool plus = (d.pos[j >> 5] >> sh) & 1u, minus = (d.neg[j >> 5] >> sh) & 1u;      // wave-uniform
        if (plus | minus) {
#pragma unroll
            for (int k = 0; k < 9; k++) p.y[k] = minus ? pny[k] : py[k];
            add_point<G>(acc, inf, p);                      // exceptional for k = r - 2 at its last digit (see above) and for no other scalar below r
            if (inf) break;                                 // ... where the product is infinity
        }
    }
    if (!inf) o = G::leave(acc);
    out[i] = o;
}

// n affine points, Montgomery coordinates (a .zkey section) -> standard form in place, what zkc_msm_g1_load_dev takes.  *bad |= 1 for a coordinate >= q.
__global__ void __launch_bounds__(256)
zkc_p2_mont_to_std(uint32_t* __restrict__ pts, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[16]; load_words<16>(w, pts + 16 * (size_t)i);
    if (!coords_below_q<G1Ops>(w)) { atomicOr(bad, 1u); return; }
    uint32_t xs[8], ys[8];
    fp_to_std<FqParams>(xs, fq_of(w)); fp_to_std<FqParams>(ys, fq_of(w + 8));
    uint4* q = reinterpret_cast<uint4*>(pts + 16 * (size_t)i);
    q[0] = make_uint4(xs[0], xs[1], xs[2], xs[3]); q[1] = make_uint4(xs[4], xs[5], xs[6], xs[7]);
    q[2] = make_uint4(ys[0], ys[1], ys[2], ys[3]); q[3] = make_uint4(ys[4], ys[5], ys[6], ys[7]);
}

thread_local double g_p2_ms[9] = {0};

// Secret, a scalar cleared on every way out of its scope, and std_is_zero: zkc_host_util.h

// k (standard form, 0 < k < 2^255) -> its non-adjacent form
ScaleDigits recode_naf(const uint32_t k_in[8]) {
    ScaleDigits d{}; d.top = -1;
    uint32_t k[9]; memcpy(k, k_in, 32); k[8] = 0;
    auto nonzero = [&] { uint32_t o = 0; for (int i = 0; i < 9; i++) o |= k[i]; return o != 0; };
    for (int j = 0; nonzero() && j < 256; j++) {
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) { d.pos[j >> 5] |= 1u << (j & 31); k[0] -= 1; }
            else { d.neg[j >> 5] |= 1u << (j & 31); uint64_t c = 1; for (int i = 0; i < 9 && c; i++) { c += k[i]; k[i] = (uint32_t)c; c >>= 32; } }
            d.top = j;
        }
        for (int i = 0; i < 8; i++) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
        k[8] >>= 1;
    }
    return d;
}


// the body of zkc_g1_scale_dev: the lock is held and the device is set.  ms (may be NULL): [0] the scale kernel, [1] the conversion to affine
int scale_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const uint32_t k[8], bool mont, void* d_out, double* ms) {
    if (std_is_zero(k)) {
        ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, (size_t)n * 64, ctx->stream));
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return ZKC_OK;
    }
    const ScaleDigits dg = recode_naf(k);
    DevBuf sum, flag;
    int rca;
    if ((rca = sum.alloc(ctx, (size_t)n * sizeof(G1XYZZ))) || (rca = flag.alloc(ctx, 4))) return rca;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(flag.p, 0xff, 4, ctx->stream));
    const clk::time_point t0 = clk::now();
    hipLaunchKernelGGL(zkc_p2_scale_g1, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, (const uint32_t*)d_points, n, dg, mont ? 1 : 0, (G1XYZZ*)sum.p, (uint32_t*)flag.p);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    uint32_t bad = 0;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const clk::time_point t1 = clk::now();
    if (bad != 0xffffffffu) return zkc_fail(ctx, ZKC_ERR_FORMAT, "zkc_g1_scale_dev: point " + std::to_string(bad) + " has a coordinate >= q or is not on the curve");
    const int rc = fixed_affine<Fq>(ctx, (const G1XYZZ*)sum.p, n, d_out, mont);
    if (ms) { ms[0] = ms_since(t0, t1); ms[1] = ms_since(t1); }
    return rc;
}

// ---- points of a .zkey on the host: rd_*_mont / wr_*_mont (zkc_host_util.h) ----
// the uncompressed form of a point as a hash takes it: unc_g1 / unc_g2 (zkc_host_util.h)
template <class F> Affine<F> host_mul(const Affine<F>& p, const uint32_t k[8]) { return xyzz_to_affine(xyzz_mul(XYZZ<F>::from_affine(p), k)); }

// a square root in Fq2 = Fq[u] / (u^2 + 1), q = 3 mod 4, by the complex method (Adj, Rodriguez-Henriquez, "Square root computation over even extension fields", alg. 9):
// a1 = a^((q - 3) / 4), alpha = a1^2 a = a^((q - 1) / 2), x0 = a1 a; alpha = -1: the root is u x0; otherwise (1 + alpha)^((q - 1) / 2) x0.  The caller squares the result.
Fq2 fq2_sqrt_candidate(const Fq2& a) {
    uint32_t e34[8], e12[8];                                   // (q - 3) / 4 and (q - 1) / 2
    for (int i = 0; i < 8; i++) e34[i] = e12[i] = FqParams::p[i];
    e34[0] -= 3; e12[0] -= 1;                                  // q = ...47 hex: no borrow
    for (int i = 0; i < 8; i++) { e34[i] = (e34[i] >> 2) | (i < 7 ? e34[i + 1] << 30 : 0); e12[i] = (e12[i] >> 1) | (i < 7 ? e12[i + 1] << 31 : 0); }
    const Fq2 a1 = pairing::fq2_pow(a, e34, 256), x0 = a1 * a, alpha = a1 * x0;
    const Fq2 minus1 = fp_neg(Fq2::one());
    if (alpha == minus1) return Fq2{fp_neg(x0.c1), x0.c0};     // u x0
    return pairing::fq2_pow(Fq2::one() + alpha, e12, 256) * x0;
}

// THE ONE PLACE that says how the G2 challenge of a contribution is derived from its transcript.  It must be a hash to G2 with UNKNOWN discrete logarithm: a multiple
// of the generator by a hashed scalar would let anyone compute g2_spx = x g2_sp from g1_sx without knowing x, and the proof of knowledge would prove nothing.
//   for ctr = 0, 1, ...: stream = SHA-256(transcript || ctr as u32 little endian || j) for j = 0, 1, 2, 3 (a byte), back to back: 128 bytes
//     c0 = stream[0..32) and c1 = stream[32..64) as big-endian integers, masked to 254 bits; either >= q: next ctr (rejection, no reduction: no bias)
//     x = c0 + c1 u; y^2 = x^3 + 3 / (9 + u); no root in Fq2: next ctr
//     y = whichever of +-y has the lexicographically smaller (c1, c0) as standard-form integers, negated when bit 0 of stream[127] is set
//     multiply (x, y) by the cofactor 2q - r of the twist; infinity: next ctr; otherwise that is the challenge.
// This is NOT snarkjs' derivation (it drives G2.fromRng from a ChaCha stream keyed by the transcript, which cannot be restated here without its source): whoever has
// snarkjs at hand aligns this function, and nothing else (include/zkcensus_phase2.h).  tests/test_phase2_cpu.py restates it in Python integers.
G2Affine phase2_challenge_g2(const uint8_t transcript[64]) {
    const pairing::Consts& C = pairing::consts();
    uint32_t cof[8];                                           // 2q - r
    { uint64_t c = 0; int64_t br = 0;
      for (int i = 0; i < 8; i++) { c += 2ull * FqParams::p[i]; const int64_t v = (int64_t)(c & 0xffffffffull) - (int64_t)FrParams::p[i] - br; br = v < 0; cof[i] = (uint32_t)v; c >>= 32; } }
    for (uint32_t ctr = 0;; ctr++) {
        uint8_t stream[128];
        for (uint8_t j = 0; j < 4; j++) { parse::Sha256 h; h.update(transcript, 64); h.update(&ctr, 4); h.update(&j, 1); h.final(stream + 32 * j); }
        uint32_t c[2][8];
        for (int w = 0; w < 2; w++) { for (int i = 0; i < 8; i++) { const uint8_t* b = stream + 32 * w + 4 * (7 - i); c[w][i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]; } c[w][7] &= 0x3fffffffu; }
        if (!fp_std_lt_p<FqParams>(c[0]) || !fp_std_lt_p<FqParams>(c[1])) continue;
        const Fq2 x{fp_from_std<FqParams>(c[0]), fp_from_std<FqParams>(c[1])};
        const Fq2 rhs = fp_sqr(x) * x + C.twist_b;
        Fq2 y = fq2_sqrt_candidate(rhs);
        if (!(fp_sqr(y) == rhs)) continue;
        const Fq2 ny = fp_neg(y);
        uint32_t a[2][8], b[2][8];
        fp_to_std<FqParams>(a[0], y.c0); fp_to_std<FqParams>(a[1], y.c1); fp_to_std<FqParams>(b[0], ny.c0); fp_to_std<FqParams>(b[1], ny.c1);
        const bool neg_smaller = std_less(b[1], a[1]) || (!std_less(a[1], b[1]) && std_less(b[0], a[0]));
        if (neg_smaller != ((stream[127] & 1) != 0)) y = ny;   // take the smaller, then negate on the sign bit
        const G2Affine p = host_mul(G2Affine{x, y}, cof);
        if (!p.is_inf()) return p;
    }
}

using pairing::same_ratio;                                  // e(a, d) == e(b, c): zkc_pairing.h

// pubkey_j of a record: U(deltaAfter) U(g1_s) U(g1_sx) U(g2_spx) transcript, 384 bytes.  false: a coordinate >= q
bool pubkey_bytes(const parse::P2Record& r, uint8_t out[384]) {
    G1Affine a, s, sx; G2Affine spx;
    if (!rd_g1_mont(a, r.deltaAfter) || !rd_g1_mont(s, r.g1_s) || !rd_g1_mont(sx, r.g1_sx) || !rd_g2_mont(spx, r.g2_spx)) return false;
    unc_g1(out, a); unc_g1(out + 64, s); unc_g1(out + 128, sx); unc_g2(out + 192, spx); memcpy(out + 320, r.transcript, 64);
    return true;
}
// H(csHash || pubkey_0 .. pubkey_(k - 1)) left open, for the transcript of record k or the hash of a contribution
bool hash_prefix(parse::Blake2b& h, const parse::P2Section& s, size_t k) {
    h.update(s.csHash, 64);
    for (size_t j = 0; j < k; j++) { uint8_t pk[384]; if (!pubkey_bytes(s.rec[j], pk)) return false; h.update(pk, 384); }
    return true;
}

// a whole image: sections, header checks (without the coefficient scan: the loader's), section 10
struct Image { parse::BinSections bs; parse::ZkeyHeader zh; parse::P2Section p2; };
bool read_image(const void* buf, size_t len, Image& im, std::string& why) {
    if (!buf) { why = "no image"; return false; }
    if (!parse::binfile_sections((const uint8_t*)buf, len, "zkey", 1, im.bs, why) || !parse::zkey_check(im.bs, im.zh, why, false)) return false;
    if (!im.bs.sec[10]) { why = "zkey: missing section 10"; return false; }
    return parse::phase2_section(im.bs.sec[10], im.bs.ssz[10], im.p2, why);
}
constexpr size_t OFF_ALPHA1 = 84, OFF_DELTA1 = 468, OFF_DELTA2 = 532;      // inside section 2: n8q q n8r r nVars nPub domainSize | alpha1 beta1 beta2 gamma2 | delta1 delta2

}  // namespace

extern "C" int zkc_g1_scale_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const uint8_t k[32], int mont, void* d_out) {
    if (!ctx || !d_points || !k || !d_out || n == 0) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_scale_dev: bad argument");
    uint32_t ks[8]; memcpy(ks, k, 32);
    if (!fp_std_lt_p<FrParams>(ks)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_g1_scale_dev: scalar >= r");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return scale_dev(ctx, d_points, n, ks, mont != 0, d_out, nullptr);
}

extern "C" void zkc_blake2b512(const void* data, size_t len, uint8_t out[64]) { parse::blake2b512(data, len, out); }

extern "C" int zkc_zkey_contributions(const void* zkey, size_t len, uint8_t csHash[64], uint32_t* n, void* records_out, size_t* records_len, char* err, size_t errlen) {
    if (!zkey || !n || !records_len) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_zkey_contributions: bad argument");
    parse::BinSections bs; parse::P2Section s; std::string why;
    if (!parse::phase2_of_zkey((const uint8_t*)zkey, len, bs, s, why)) return err_out(err, errlen, ZKC_ERR_FORMAT, why);
    if (csHash) memcpy(csHash, s.csHash, 64);
    *n = s.n;
    const size_t room = *records_len; *records_len = s.records_len;
    if (!records_out) return ZKC_OK;
    if (room < s.records_len) return err_out(err, errlen, ZKC_ERR_SHORT_BUFFER, "zkc_zkey_contributions: records buffer too short");
    if (s.records_len) memcpy(records_out, s.records, s.records_len);
    return ZKC_OK;
}

extern "C" int zkc_zkey_contribute(zkc_ctx* ctx, const void* zkey, size_t len, const uint8_t delta[32], const char* name, void* out, size_t* out_len, uint8_t hash[64]) {
    if (!ctx || !zkey || !out_len) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_zkey_contribute: bad argument");
    const clk::time_point t0 = clk::now();
    Image im; std::string why;
    if (!read_image(zkey, len, im, why)) return zkc_fail(ctx, ZKC_ERR_FORMAT, "zkc_zkey_contribute: " + why);
    const size_t name_len = name ? std::min<size_t>(strlen(name), 64) : 0;
    const size_t params_len = name_len ? 2 + name_len : 0, rec_len = parse::P2_FIXED + params_len, need = len + rec_len;
    if (!out) { *out_len = need; return ZKC_OK; }
    if (*out_len < need) { *out_len = need; return zkc_fail(ctx, ZKC_ERR_SHORT_BUFFER, "zkc_zkey_contribute: output buffer too short"); }
    Secret d, s, dinv;                                         // delta, the scalar of g1_s, 1 / delta
    if (delta) memcpy(d.v, delta, 32); else zkc_random_scalars((uint8_t*)d.v, 1);
    if (std_is_zero(d) || !fp_std_lt_p<FrParams>(d)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_zkey_contribute: delta must be in [1, r)");
    do zkc_random_scalars((uint8_t*)s.v, 1); while (std_is_zero(s));
    fp_to_std<FrParams>(dinv.v, fp_inv<FrParams>(fp_from_std<FrParams>(d.v)));
    // ---- the host's handful of points: delta1, delta2 and the proof of knowledge ----
    const uint8_t* hdr = im.bs.sec[2];
    G1Affine delta1; G2Affine delta2;
    if (!rd_g1_mont(delta1, hdr + OFF_DELTA1) || !rd_g2_mont(delta2, hdr + OFF_DELTA2) || !pairing::g1_on_curve(delta1) || !pairing::g2_on_curve(delta2))
        return zkc_fail(ctx, ZKC_ERR_FORMAT, "zkc_zkey_contribute: delta1 / delta2 is not a point of its curve");
    const G1Affine delta1n = host_mul(delta1, d), g1_s = host_mul(g1_generator(), s), g1_sx = host_mul(g1_s, d);
    const G2Affine delta2n = host_mul(delta2, d);
    uint8_t transcript[64], u[128];
    { parse::Blake2b h; if (!hash_prefix(h, im.p2, im.p2.rec.size())) return zkc_fail(ctx, ZKC_ERR_FORMAT, "zkc_zkey_contribute: a recorded point has a coordinate >= q");
      unc_g1(u, g1_s); h.update(u, 64); unc_g1(u, g1_sx); h.update(u, 64); h.final(transcript); }
    const G2Affine g2_spx = host_mul(phase2_challenge_g2(transcript), d);
    const clk::time_point t1 = clk::now();
    // ---- sections 8 and 9 times 1 / delta on the GPU, as one batch ----
    const size_t n8 = (size_t)(im.bs.ssz[8] / 64), n9 = (size_t)(im.bs.ssz[9] / 64), npts = n8 + n9;
    if (npts > 0xffffffffull) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_zkey_contribute: key too large");
    uint8_t* o = (uint8_t*)out; const uint8_t* in = (const uint8_t*)zkey;
    const size_t cut = (size_t)(im.bs.sec[10] - in) + (size_t)im.bs.ssz[10];              // the record goes where section 10 ends
    memcpy(o, in, cut); memcpy(o + cut + rec_len, in + cut, len - cut);
    // whatever follows section 10 in the file moved by rec_len
    auto at = [&](const uint8_t* p) { const size_t off = (size_t)(p - in); return o + (off >= cut ? off + rec_len : off); };
    double kms[2] = {0, 0}; clk::time_point t2 = t1, t3 = t1;
    {
        ZKC_LOCK(ctx);
        ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        DevBuf pts; int rca;
        if ((rca = pts.alloc(ctx, npts * 64))) return rca;
        ZKC_HIP_CHECK(ctx, hipMemcpy(pts.p, im.bs.sec[8], n8 * 64, hipMemcpyHostToDevice));
        ZKC_HIP_CHECK(ctx, hipMemcpy((uint8_t*)pts.p + n8 * 64, im.bs.sec[9], n9 * 64, hipMemcpyHostToDevice));
        t2 = clk::now();
        const int rc = scale_dev(ctx, pts.p, (uint32_t)npts, dinv, true, pts.p, kms); if (rc) return rc;
        t3 = clk::now();
        ZKC_HIP_CHECK(ctx, hipMemcpy(at(im.bs.sec[8]), pts.p, n8 * 64, hipMemcpyDeviceToHost));
        ZKC_HIP_CHECK(ctx, hipMemcpy(at(im.bs.sec[9]), (uint8_t*)pts.p + n8 * 64, n9 * 64, hipMemcpyDeviceToHost));
    }
    const clk::time_point t4 = clk::now();
    // ---- header, record, hash ----
    wr_g1_mont(at(hdr + OFF_DELTA1), delta1n); wr_g2_mont(at(hdr + OFF_DELTA2), delta2n);
    uint8_t* sec10 = at(im.bs.sec[10]);
    const uint64_t newsz = im.bs.ssz[10] + rec_len; memcpy(sec10 - 8, &newsz, 8);
    const uint32_t cnt = im.p2.n + 1; memcpy(sec10 + 64, &cnt, 4);
    uint8_t* r = o + cut;
    wr_g1_mont(r, delta1n); wr_g1_mont(r + 64, g1_s); wr_g1_mont(r + 128, g1_sx); wr_g2_mont(r + 192, g2_spx); memcpy(r + 320, transcript, 64);
    const uint32_t type = parse::P2_TYPE_PLAIN, pl = (uint32_t)params_len; memcpy(r + 384, &type, 4); memcpy(r + 388, &pl, 4);
    if (name_len) { r[392] = 0x01; r[393] = (uint8_t)name_len; memcpy(r + 394, name, name_len); }
    *out_len = need;
    {
        parse::Blake2b h; (void)hash_prefix(h, im.p2, im.p2.rec.size());
        uint8_t pk[384]; unc_g1(pk, delta1n); unc_g1(pk + 64, g1_s); unc_g1(pk + 128, g1_sx); unc_g2(pk + 192, g2_spx); memcpy(pk + 320, transcript, 64);
        h.update(pk, 384);
        uint8_t hh[64]; h.final(hh); if (hash) memcpy(hash, hh, 64);
    }
    const clk::time_point t5 = clk::now();
    g_p2_ms[0] = ms_since(t0, t1); g_p2_ms[1] = ms_since(t1, t2); g_p2_ms[2] = kms[0]; g_p2_ms[3] = kms[1]; g_p2_ms[4] = ms_since(t3, t4); g_p2_ms[5] = ms_since(t4, t5);
    return ZKC_OK;
}

namespace {

// sum_i w_i P_i over one section of a key (Montgomery points of the image) on the GPU: upload, standard form, resident window tables, one MSM.
// 0 ok; 1: the section holds a coordinate >= q or a point off the curve (why set); < 0: -ZKC_ERR_*
int section_msm(zkc_ctx* ctx, const uint8_t* sec, uint32_t n, const uint8_t* weights, uint8_t out[64], std::string& why, double ms[2]) {
    memset(out, 0, 64);
    if (n == 0) return 0;
    ZKC_LOCK(ctx);
    if (hipSetDevice(ctx->device) != hipSuccess) return -ZKC_ERR_HIP;
    const clk::time_point t0 = clk::now();
    DevBuf pts, w, flag; uint32_t bad = 0;
    if (hipMalloc(&pts.p, (size_t)n * 64) != hipSuccess || hipMalloc(&w.p, (size_t)n * 32) != hipSuccess || hipMalloc(&flag.p, 4) != hipSuccess ||
        hipMemcpy(pts.p, sec, (size_t)n * 64, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(w.p, weights, (size_t)n * 32, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemsetAsync(flag.p, 0, 4, ctx->stream) != hipSuccess) { zkc_fail(ctx, ZKC_ERR_HIP, "zkc_zkey_verify_contributions: device buffers"); return -ZKC_ERR_HIP; }
    hipLaunchKernelGGL(zkc_p2_mont_to_std, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (uint32_t*)pts.p, n, (uint32_t*)flag.p);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        zkc_fail(ctx, ZKC_ERR_HIP, "zkc_zkey_verify_contributions: conversion kernel"); return -ZKC_ERR_HIP; }
    if (bad) { why = "a coordinate >= q"; return 1; }
    zkc_msm* m = nullptr;
    int rc = zkc_msm_g1_load_dev(ctx, pts.p, n, &m);
    if (rc == ZKC_ERR_FORMAT) { why = "a point off the curve"; return 1; }
    if (rc) return -rc;
    const clk::time_point t1 = clk::now();
    rc = zkc_msm_g1_dev(m, w.p, out);
    zkc_msm_g1_free(m);
    ms[0] += ms_since(t0, t1); ms[1] += ms_since(t1);
    return rc ? -rc : 0;
}

}  // namespace

extern "C" int zkc_zkey_verify_contributions(zkc_ctx* ctx, const void* init, size_t init_len, const void* final_, size_t final_len, const uint8_t* seed32, uint32_t* n_new,
                                             char* err, size_t errlen) {
    if (!ctx || !init || !final_) return err_out(err, errlen, -ZKC_ERR_BAD_ARG, "zkc_zkey_verify_contributions: bad argument");
    if (n_new) *n_new = 0;
    if (err && errlen) err[0] = 0;
    auto invalid = [&](const std::string& m) { return err_out(err, errlen, 0, m); };
    // ---- (a) ----
    Image A, B; std::string why;
    if (!read_image(init, init_len, A, why)) return invalid("check (a): the initial key does not parse: " + why);
    if (!read_image(final_, final_len, B, why)) return invalid("check (a): the final key does not parse: " + why);
    if (A.zh.nVars != B.zh.nVars || A.zh.nPub != B.zh.nPub || A.zh.n != B.zh.n) return invalid("check (a): nVars, nPublic or domainSize differ");
    if (memcmp(A.bs.sec[2] + OFF_ALPHA1, B.bs.sec[2] + OFF_ALPHA1, OFF_DELTA1 - OFF_ALPHA1)) return invalid("check (a): alpha1, beta1, beta2 or gamma2 differ");
    for (int s = 3; s <= 7; s++)
        if (A.bs.ssz[s] != B.bs.ssz[s] || memcmp(A.bs.sec[s], B.bs.sec[s], (size_t)A.bs.ssz[s])) return invalid("check (a): section " + std::to_string(s) + " differs");
    if (memcmp(A.p2.csHash, B.p2.csHash, 64)) return invalid("check (a): the circuit hashes differ");      // after the sections: a key of another circuit is told by the section that shows it
    // ---- (b) ----
    if (B.p2.n < A.p2.n || B.p2.records_len < A.p2.records_len) return invalid("check (b): the final key has fewer contributions than the initial key");
    {
        size_t alen = 0; for (uint32_t k = 0; k < A.p2.n; k++) alen += B.p2.rec[k].rec_len;
        if (alen != A.p2.records_len || memcmp(A.p2.records, B.p2.records, alen)) return invalid("check (b): the initial key's contributions are not a prefix of the final key's");
    }
    if (n_new) *n_new = B.p2.n - A.p2.n;
    // ---- (c) ----
    const clk::time_point tp0 = clk::now();
    G1Affine delta; G2Affine delta2A, delta2B; G1Affine delta1B;
    if (!rd_g1_mont(delta, A.bs.sec[2] + OFF_DELTA1) || !rd_g2_mont(delta2A, A.bs.sec[2] + OFF_DELTA2) || !pairing::g1_on_curve(delta) || delta.is_inf() ||
        !pairing::g2_in_subgroup(delta2A) || delta2A.is_inf()) return invalid("check (c): the initial key's delta1 / delta2 is no point of its group");
    for (uint32_t k = A.p2.n; k < B.p2.n; k++) {
        const parse::P2Record& r = B.p2.rec[k]; const std::string at = "check (c), contribution " + std::to_string(k) + ": ";
        if (r.type != parse::P2_TYPE_PLAIN) return invalid(at + "a beacon contribution (type 1) cannot be verified: its delta comes from snarkjs' random stream");
        G1Affine after, s, sx; G2Affine spx;
        if (!rd_g1_mont(after, r.deltaAfter) || !rd_g1_mont(s, r.g1_s) || !rd_g1_mont(sx, r.g1_sx) || !rd_g2_mont(spx, r.g2_spx)) return invalid(at + "a coordinate >= q");
        if (after.is_inf() || s.is_inf() || sx.is_inf() || spx.is_inf() || !pairing::g1_on_curve(after) || !pairing::g1_on_curve(s) || !pairing::g1_on_curve(sx) ||
            !pairing::g2_in_subgroup(spx)) return invalid(at + "a point is at infinity or not in its group");
        uint8_t tr[64], u[64];
        { parse::Blake2b h; if (!hash_prefix(h, B.p2, k)) return invalid(at + "an earlier record holds a coordinate >= q");
          unc_g1(u, s); h.update(u, 64); unc_g1(u, sx); h.update(u, 64); h.final(tr); }
        if (memcmp(tr, r.transcript, 64)) return invalid(at + "the stored transcript is not the recomputed one");
        const G2Affine sp = phase2_challenge_g2(tr);
        if (!same_ratio(s, sx, sp, spx)) return invalid(at + "sameRatio(g1_s, g1_sx; g2_sp, g2_spx) fails");
        if (!same_ratio(delta, after, sp, spx)) return invalid(at + "sameRatio(delta, deltaAfter; g2_sp, g2_spx) fails");
        delta = after;
    }
    // ---- (d) ----
    if (!rd_g1_mont(delta1B, B.bs.sec[2] + OFF_DELTA1) || !rd_g2_mont(delta2B, B.bs.sec[2] + OFF_DELTA2)) return invalid("check (d): a coordinate of delta1 / delta2 >= q");
    if (!(delta.x == delta1B.x && delta.y == delta1B.y)) return invalid("check (d): the final key's delta1 is not the last contribution's deltaAfter");
    if (delta2B.is_inf() || !pairing::g2_in_subgroup(delta2B)) return invalid("check (d): the final key's delta2 is not in G2");
    if (!same_ratio(g1_generator(), delta1B, g2_generator(), delta2B)) return invalid("check (d): sameRatio(G1, delta1; G2, delta2) fails");
    double pair_ms = ms_since(tp0);
    // ---- (e), which is (f) too: with nothing new the sums and the deltas are equal ----
    const uint32_t n8 = (uint32_t)(A.bs.ssz[8] / 64), n9 = (uint32_t)(A.bs.ssz[9] / 64);
    std::vector<uint8_t> w((size_t)(n8 + n9) * 32);
    if (seed32) { const std::vector<uint32_t> rho = verify_weights(seed32, (size_t)n8 + n9); memcpy(w.data(), rho.data(), w.size()); }
    else zkc_random_scalars(w.data(), (size_t)n8 + n9);
    double ms[2] = {0, 0};
    const struct { int sec; uint32_t n; size_t woff; const char* name; } parts[2] = {{8, n8, 0, "C"}, {9, n9, (size_t)n8 * 32, "H"}};
    for (const auto& p : parts) {
        uint8_t sa[64], sb[64]; G1Affine SA, SB;
        const struct { const Image* im; uint8_t* out; const char* which; } sides[2] = {{&A, sa, "initial"}, {&B, sb, "final"}};
        for (const auto& sd : sides) {
            const int rc = section_msm(ctx, sd.im->bs.sec[p.sec], p.n, w.data() + p.woff, sd.out, why, ms);
            if (rc < 0) return err_out(err, errlen, rc, std::string("zkc_zkey_verify_contributions: ") + zkc_last_error(ctx));
            if (rc) return invalid(std::string("check (e), section ") + std::to_string(p.sec) + " (" + p.name + ") of the " + sd.which + " key: " + why);
        }
        const clk::time_point tq = clk::now();
        if (!rd_g1_std(SA, sa) || !rd_g1_std(SB, sb)) return err_out(err, errlen, -ZKC_ERR_GENERIC, "zkc_zkey_verify_contributions: MSM result out of range");
        const bool ok = same_ratio(SA, SB, delta2B, delta2A);                       // e(SA, delta2A) == e(SB, delta2B)
        pair_ms += ms_since(tq);
        if (!ok) return invalid(std::string("check (e): the ") + p.name + " points (section " + std::to_string(p.sec) + ") are not the initial key's times one scalar 1 / delta");
    }
    g_p2_ms[6] = ms[0]; g_p2_ms[7] = ms[1]; g_p2_ms[8] = pair_ms;
    return 1;
}

extern "C" int zkc_phase2_stats(double ms[9]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 9; i++) ms[i] = g_p2_ms[i];
    return ZKC_OK;
}

// measurement hook (tools/phase2_bench.py): the products of zkc_g1_scale_dev on host threads, with the variable-base multiplication of zkc_curve.h (xyzz_mul) and one
// inversion per point (xyzz_to_affine).  Montgomery coordinates in and out; the points are taken as on the curve.  *ms = wall time of the threads.
extern "C" int zkc_debug_phase2_host_scale(const void* points, uint32_t n, const uint8_t k[32], int threads, void* out, double* ms) {
    if (!points || !k || !out || n == 0 || threads < 1 || threads > 256) return ZKC_ERR_BAD_ARG;
    uint32_t ks[8]; memcpy(ks, k, 32);
    if (!fp_std_lt_p<FrParams>(ks)) return ZKC_ERR_BAD_ARG;
    const uint8_t* in = (const uint8_t*)points; uint8_t* o = (uint8_t*)out;
    const clk::time_point t0 = clk::now();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([=] {
            const uint32_t lo = (uint32_t)((uint64_t)n * t / threads), hi = (uint32_t)((uint64_t)n * (t + 1) / threads);
            for (uint32_t i = lo; i < hi; i++) {
                G1Affine p; memcpy(p.x.v, in + 64 * (size_t)i, 32); memcpy(p.y.v, in + 64 * (size_t)i + 32, 32);
                wr_g1_mont(o + 64 * (size_t)i, p.is_inf() ? p : host_mul(p, ks));
            }
        });
    for (auto& th : pool) th.join();
    if (ms) *ms = ms_since(t0);
    return ZKC_OK;
}

extern "C" int zkc_debug_phase2_challenge_g2(const uint8_t transcript[64], uint8_t out[128]) {
    if (!transcript || !out) return ZKC_ERR_BAD_ARG;
    const G2Affine p = phase2_challenge_g2(transcript);
    wr_g2_std(out, p);
    return ZKC_OK;
}
