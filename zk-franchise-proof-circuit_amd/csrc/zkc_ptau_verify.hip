// zkc_ptau_verify.hip -- is a powers-of-tau file the powers of one tau?  (include/zkcensus_ptau_verify.h): the point checks of `snarkjs powersoftau verify`
// (circuit/circuit-compiler.sh:67, :73) over sections 2 .. 6, and the engine under them, one weighted PAIR of sums over consecutive points.  Product code: host stages
// around one new kernel.
//
// The sums.  A section M_0 .. M_(n-1) holds the powers of one tau exactly when M_(i+1) = tau M_i for every i, and with random weights r_i that is, up to 2^-128,
// lo = sum_(i<n-1) r_i M_i and hi = sum_(i<n-1) r_i M_(i+1) being in the ratio tau: one pairing check per section.  The work is the two sums:
//   masks   one lane per (segment, bit): the 128-bit weights of a segment of SEG = 16 consecutive terms transposed to 128 words, word b holding bit b of every weight of
//           the segment -- the lanes of the sum kernel then read one word per bit step, neighbouring lanes neighbouring words
//   sum     one lane per segment and per sum (blockIdx.y = 0: lo, 1: hi -- the same kernel with the points taken one further on): the 128 bits from the top, ONE doubling
//           of the lane's accumulator per bit (G::dbl), then a mixed addition (add_point, zkc_point_ops.h: every exceptional case handled) of each point of the segment
//           whose weight has that bit.  The doubling chain is shared by the SEG points of the segment, not paid per point as in zkc_ptau_scale, and no array of n products
//           is written: a lane's only store is its partial sum.  The points are re-read through the cache at every bit step (64 / 128 B per ~11 / ~33 field products):
//           the G1 kernel takes 128 registers and the G2 kernel 224 without scratch, four and two waves per SIMD, and a segment's points held in registers or LDS
//           would cost the occupancy that hides these loads.  lo and hi are two lanes, not two accumulators in one: the G2 accumulator alone is 72 registers.
//           SEG was chosen on the GPU among 8, 16 and 32 (profiles/ptau_verify_2p20.json: 2^21 points of G1 in 39 / 35 / 46 ms, 2^20 of G2 in 52 / 47 / 77 ms).  The
//           kernel is bound by the vector units and, inside a wave, by the lane with the most set bits: every bit step lasts as long as the fullest of the wave's 64
//           masks, about 13 additions for a mean of 8 at SEG = 16.  Longer segments even that out but leave fewer lanes than the device has room for below 2^22 terms.
//   reduce  the 2 x nseg partial sums to 2 sums with the reduction kernel of zkc_setup_ptau.hip (zkc_point_red.h), then affine (fixed_affine).
// Every loop is bounded by a constant or by a count the host computed (the walk over the set bits of a mask word: at most SEG turns); nothing waits on a flag.
//
// The file.  One pass over sections 2, 3, 4, 5 in chunks of at most CHUNK terms (a chunk of t terms is t + 1 points: neighbouring chunks share one point), per chunk:
// read, upload, check the points (points_check_dev; infinity is refused on the host), for section 3 the membership kernel of zkc_pairing_dev.hip, then the two sums, which
// are added to the section's on the host.  The device holds one chunk and its work space, never a section.  With ctx = NULL the same steps run on the threads of par_chunks
// with zkc_curve.h; both paths leave canonical affine points, so verdict and sums agree.  Then the order of the checks decides what is reported (the header says which).
#include <cstring>
#include <string>
#include <vector>
#include "zkc_prover.h"
#include "zkc_ecntt.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_point_ops.h"
#include "zkc_point_red.h"
#include "zkc_host_util.h"
#include "zkc_pairing.h"
#include "zkc_pairing_dev.h"
#include "zkc_file_points.h"
#include "zkc_ptau_parse.h"
#include "zkc_setup_write.h"
#include "zkc_verify_host.h"
#include "../../include/zkcensus_ptau_verify.h"

using namespace zkc;

namespace {

constexpr uint32_t SEG = 16;                     // terms per lane of the sum kernel, at most the 32 bits of a mask word: 16 measured best of 8, 16, 32 (see above)
constexpr uint32_t CHUNK = 1u << 22;             // terms per chunk of a section: 512 MB of G2 points, 64 MB of weights and as much of masks on the device
constexpr uint32_t HOST_SEG = 256;               // ctx = NULL: terms per unit of work of a host thread
constexpr uint32_t NONE = 0xffffffffu;

// ================================================================ device ================================================================

// mask[b * nseg + s] = bit b of the weights of the terms s SEG .. s SEG + SEG - 1 (bit t: term s SEG + t; terms from nterms on: 0).  w: 4 words per weight
__global__ void __launch_bounds__(256)
zkc_wsum_masks(const uint32_t* __restrict__ w, uint32_t nterms, uint32_t nseg, uint32_t* __restrict__ mask) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)128 * nseg) return;
    const uint32_t b = (uint32_t)(g / nseg), s = (uint32_t)(g - (size_t)b * nseg);
    uint32_t m = 0;
    for (uint32_t t = 0; t < SEG; t++) {
        const uint32_t term = s * SEG + t;
        if (term < nterms) m |= ((w[4 * (size_t)term + (b >> 5)] >> (b & 31)) & 1u) << t;
    }
    mask[g] = m;
}

// part[off * nseg + s] = sum over the terms t of segment s of weight_t * pts[s SEG + t + off], off = blockIdx.y: canonical XYZZ, infinity all zero
template <class G> __global__ void __launch_bounds__(64)
zkc_wsum(const uint32_t* __restrict__ pts, uint32_t npts, const uint32_t* __restrict__ mask, uint32_t nseg, XYZZ<typename G::F>* __restrict__ part) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x, off = blockIdx.y;
    if (s >= nseg) return;
    const uint32_t first = s * SEG + off;
    typename G::Acc acc; bool inf = true;
    for (int b = 127; b >= 0; b--) {
        if (!inf) G::dbl(acc);                   // a doubling never meets infinity: curve and twist have odd order
        uint32_t m = mask[(size_t)b * nseg + s];
        while (m) {                              // at most SEG turns
            const uint32_t idx = first + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            if (idx >= npts) continue;           // the masks name no such term
            uint32_t w[G::W]; load_words<G::W>(w, pts + (size_t)G::W * idx);
            if (all_zero<G::W>(w)) continue;
            const typename G::Pt p = G::enter(w, false);
            add_point<G>(acc, inf, p);
        }
    }
    XYZZ<typename G::F> o = XYZZ<typename G::F>::inf();
    if (!inf) o = G::leave(acc);
    part[(size_t)off * nseg + s] = o;
}

// ================================================================ host ================================================================

thread_local double g_ver_ms[6] = {0, 0, 0, 0, 0, 0};

// The pair of sums of n >= 2 checked points on the device (Montgomery words) under the n - 1 weights at d_w16: out[0] = lo, out[1] = hi, affine, Montgomery form.  The
// context's lock is held and the device is set; has synchronised and freed its work space on return.
template <class F>
int wsum_dev(zkc_ctx* ctx, const void* d_pts, uint32_t n, const void* d_w16, Affine<F> out[2]) {
    typedef typename GroupOf<F>::Ops G;
    const uint32_t nterms = n - 1, nseg = (nterms + SEG - 1) / SEG;
    DevBuf mask, part, aff; int rc;
    if ((rc = mask.alloc(ctx, (size_t)128 * nseg * 4)) || (rc = part.alloc(ctx, (size_t)2 * nseg * sizeof(XYZZ<F>))) || (rc = aff.alloc(ctx, 2 * sizeof(Affine<F>)))) return rc;
    const size_t nmask = (size_t)128 * nseg;
    hipLaunchKernelGGL(zkc_wsum_masks, dim3((unsigned)((nmask + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_w16, nterms, nseg, mask.as<uint32_t>());
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(zkc_wsum<G>, dim3((nseg + 63) / 64, 2), dim3(64), 0, ctx->stream, (const uint32_t*)d_pts, n, mask.as<uint32_t>(), nseg, part.as<XYZZ<F>>());
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = point_reduce<F>(ctx, part, std::vector<uint32_t>{nseg, nseg})) || (rc = fixed_affine<F>(ctx, part.as<XYZZ<F>>(), 2, aff.p, true))) return rc;      // both synchronise
    ZKC_HIP_CHECK(ctx, hipMemcpy((void*)out, aff.p, 2 * sizeof(Affine<F>), hipMemcpyDeviceToHost));
    return ZKC_OK;
}

// ... and on host threads: lo += , hi += the sums of the n - 1 terms (w16: 16 B per weight)
template <class F>
void wsum_host(const Affine<F>* pts, uint32_t n, const uint8_t* w16, XYZZ<F>& lo, XYZZ<F>& hi) {
    const uint32_t nterms = n - 1, nseg = (nterms + HOST_SEG - 1) / HOST_SEG;
    std::vector<XYZZ<F>> part((size_t)2 * nseg);
    par_chunks((size_t)2 * nseg, 1, [&](size_t a, size_t b) {
        for (size_t j = a; j < b; j++) {
            const uint32_t s = (uint32_t)(j >> 1), off = (uint32_t)(j & 1), t0 = s * HOST_SEG, t1 = std::min(nterms, t0 + HOST_SEG);
            XYZZ<F> acc = XYZZ<F>::inf();
            for (int bit = 127; bit >= 0; bit--) {
                acc = xyzz_dbl(acc);
                for (uint32_t t = t0; t < t1; t++)
                    if ((w16[16 * (size_t)t + (bit >> 3)] >> (bit & 7)) & 1) acc = xyzz_add_affine(acc, pts[t + off]);      // complete
            }
            part[j] = acc;
        }
    });
    for (uint32_t s = 0; s < nseg; s++) { lo = xyzz_add(lo, part[2 * (size_t)s]); hi = xyzz_add(hi, part[2 * (size_t)s + 1]); }
}

// the smallest index of an all-zero point, NONE when there is none
template <class F> uint32_t first_infinity(const Affine<F>* p, size_t n) {
    std::atomic<uint32_t> first{NONE};
    par_chunks(n, 1u << 16, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) if (p[i].is_inf()) { uint32_t cur = first.load(); while ((uint32_t)i < cur && !first.compare_exchange_weak(cur, (uint32_t)i)) {} break; }
    });
    return first.load();
}
uint32_t host_first_outside_g2(const G2Affine* p, size_t n) {
    std::atomic<uint32_t> first{NONE};
    par_chunks(n, 16, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) if (!pairing::g2_in_subgroup(p[i])) { uint32_t cur = first.load(); while ((uint32_t)i < cur && !first.compare_exchange_weak(cur, (uint32_t)i)) {} break; }
    });
    return first.load();
}

struct Verdict { uint32_t check = ZKC_PTAU_CHECK_NONE, section = 0; uint64_t index = 0; std::string text; bool failed() const { return check != ZKC_PTAU_CHECK_NONE; } };
Verdict refuse(uint32_t check, uint32_t section, uint64_t index, const std::string& text) { Verdict v; v.check = check; v.section = section; v.index = index; v.text = text; return v; }

// what the pass over one section leaves
template <class F> struct Section {
    XYZZ<F> lo = XYZZ<F>::inf(), hi = XYZZ<F>::inf();          // the sums, when `summed`
    Affine<F> p0, p1;                                           // points 0 and 1
    bool summed = false;
};

// One section.  point: set (and the pass ended) at the first bad point; subgroup: set at the first point of section 3 outside G2 -- from then on, as when it arrives set,
// only the points are checked (nothing later in the order of the checks is reported once it is).  rc != 0: err is written
template <class F>
int section_pass(zkc_ctx* ctx, const parse::Ptau& pt, int sec, const uint8_t* w16, uint32_t chunk, Section<F>& S, Verdict& point, Verdict& subgroup, char* err, size_t errlen) {
    typedef GroupOf<F> G;
    constexpr size_t PT = sizeof(Affine<F>);
    const uint64_t npts = parse::ptau_section_points(sec, pt.power), nterms = npts - 1;      // power >= 1: at least two points
    const uint32_t cap = (uint32_t)std::min<uint64_t>(chunk, nterms) + 1;
    std::vector<Affine<F>> buf(cap);
    DevBuf d_pts, d_w; int rc; std::string why;
    if (ctx && ((rc = d_pts.alloc(ctx, (size_t)cap * PT)) || (rc = d_w.alloc(ctx, (size_t)(cap - 1) * 16)))) return err_out(err, errlen, rc, zkc_last_error(ctx));
    double* sum_ms = &g_ver_ms[G::g2 ? 4 : 3];
    for (uint64_t c0 = 0; c0 < nterms; c0 += chunk) {
        const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, nterms - c0), np = nt + 1;
        clk::time_point t0 = clk::now();
        if (!parse::ptau_read(pt, sec, c0, np, buf.data(), why)) return setup_fail(err, errlen, why);
        g_ver_ms[0] += ms_since(t0);
        // ---- the points ----
        t0 = clk::now();
        uint32_t bad = NONE;
        if (ctx) {
            if (hipMemcpy(d_pts.p, buf.data(), (size_t)np * PT, hipMemcpyHostToDevice) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_verify: upload"), zkc_last_error(ctx));
            if ((rc = points_check_dev<F>(ctx, d_pts.p, np, &bad))) return err_out(err, errlen, rc, zkc_last_error(ctx));
        } else bad = host_first_bad<F>(buf.data(), np);
        bad = std::min(bad, first_infinity<F>(buf.data(), np));
        g_ver_ms[1] += ms_since(t0);
        if (bad != NONE) {
            point = refuse(ZKC_PTAU_CHECK_POINT, (uint32_t)sec, c0 + bad, "ptau: section " + std::to_string(sec) + " point " + std::to_string(c0 + bad) +
                           " has a coordinate >= q, is not on the " + G::curve + " or is at infinity");
            return ZKC_OK;
        }
        if (c0 == 0) { S.p0 = buf[0]; S.p1 = buf[1]; }
        if (subgroup.failed()) continue;
        // ---- section 3: in G2 ----
        if (sec == 3) {
            t0 = clk::now();
            if (ctx) { if ((rc = g2_membership_first_bad(ctx, (const G2Affine*)d_pts.p, np, &bad))) return err_out(err, errlen, rc, zkc_last_error(ctx)); }
            else bad = host_first_outside_g2((const G2Affine*)buf.data(), np);
            g_ver_ms[2] += ms_since(t0);
            if (bad != NONE) {
                subgroup = refuse(ZKC_PTAU_CHECK_G2_SUBGROUP, 3, c0 + bad, "ptau: section 3 point " + std::to_string(c0 + bad) + " is not in G2, the order-r subgroup of the twist");
                continue;
            }
        }
        // ---- the two sums of the chunk ----
        t0 = clk::now();
        if (ctx) {
            Affine<F> out[2];
            if (hipMemcpy(d_w.p, w16 + 16 * c0, (size_t)nt * 16, hipMemcpyHostToDevice) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_verify: upload"), zkc_last_error(ctx));
            if ((rc = wsum_dev<F>(ctx, d_pts.p, np, d_w.p, out))) return err_out(err, errlen, rc, zkc_last_error(ctx));
            S.lo = xyzz_add_affine(S.lo, out[0]); S.hi = xyzz_add_affine(S.hi, out[1]);
        } else wsum_host<F>(buf.data(), np, w16 + 16 * c0, S.lo, S.hi);
        *sum_ms += ms_since(t0);
    }
    S.summed = !subgroup.failed();
    return ZKC_OK;
}

// the whole check.  w16: 2N - 2 weights of 16 B.  Returns 1 / 0 / -ZKC_ERR_*; v: the failing check when 0.  sums (640 B, may be NULL): see the header
int verify_file(zkc_ctx* ctx, const parse::Ptau& pt, const uint8_t* w16, uint32_t chunk, Verdict& v, uint8_t* sums, char* err, size_t errlen) {
    if (sums) memset(sums, 0, 640);
    Section<Fq> T, A, B; Section<Fq2> U;
    Verdict point, subgroup; int rc;
    if ((rc = section_pass<Fq>(ctx, pt, 2, w16, chunk, T, point, subgroup, err, errlen))) return -rc;
    if (!point.failed() && (rc = section_pass<Fq2>(ctx, pt, 3, w16, chunk, U, point, subgroup, err, errlen))) return -rc;
    if (!point.failed() && (rc = section_pass<Fq>(ctx, pt, 4, w16, chunk, A, point, subgroup, err, errlen))) return -rc;
    if (!point.failed() && (rc = section_pass<Fq>(ctx, pt, 5, w16, chunk, B, point, subgroup, err, errlen))) return -rc;
    G2Affine beta2; std::string why;
    if (!point.failed()) {
        const clk::time_point t0 = clk::now();
        if (!parse::ptau_read(pt, 6, 0, 1, &beta2, why)) return -setup_fail(err, errlen, why);
        g_ver_ms[0] += ms_since(t0);
        if (!host_point_ok<Fq2>(beta2) || beta2.is_inf()) point = refuse(ZKC_PTAU_CHECK_POINT, 6, 0, "ptau: section 6 point 0 has a coordinate >= q, is not on the twist or is at infinity");
    }
    if (point.failed()) { v = point; return 0; }
    if (!subgroup.failed() && !pairing::g2_in_subgroup(beta2)) subgroup = refuse(ZKC_PTAU_CHECK_G2_SUBGROUP, 6, 0, "ptau: section 6 point 0 is not in G2, the order-r subgroup of the twist");
    if (subgroup.failed()) { v = subgroup; return 0; }
    // ---- the sums, affine ----
    const G1Affine R1 = xyzz_to_affine_gcd(T.lo), R2 = xyzz_to_affine_gcd(T.hi), A1 = xyzz_to_affine_gcd(A.lo), A2 = xyzz_to_affine_gcd(A.hi), B1 = xyzz_to_affine_gcd(B.lo),
                   B2 = xyzz_to_affine_gcd(B.hi);
    const G2Affine S1 = xyzz_to_affine_gcd(U.lo), S2 = xyzz_to_affine_gcd(U.hi);
    if (sums) { wr_g1_std(sums, R1); wr_g1_std(sums + 64, R2); wr_g2_std(sums + 128, S1); wr_g2_std(sums + 256, S2); wr_g1_std(sums + 384, A1); wr_g1_std(sums + 448, A2);
                wr_g1_std(sums + 512, B1); wr_g1_std(sums + 576, B2); }
    // ---- the checks on a handful of points ----
    const clk::time_point t0 = clk::now();
    const G1Affine G1 = g1_generator(); const G2Affine G2 = g2_generator();
    auto same = [](const auto& a, const auto& b) { return a.x == b.x && a.y == b.y; };
    auto ratio = [&](const G1Affine& lo, const G1Affine& hi) { return !lo.is_inf() && !hi.is_inf() && pairing::same_ratio(lo, hi, G2, U.p1); };
    if (!same(T.p0, G1)) v = refuse(ZKC_PTAU_CHECK_GENERATORS, 2, 0, "ptau: section 2 point 0 is not the G1 generator");
    else if (!same(U.p0, G2)) v = refuse(ZKC_PTAU_CHECK_GENERATORS, 3, 0, "ptau: section 3 point 0 is not the G2 generator");
    else if (!pairing::same_ratio(G1, T.p1, G2, U.p1)) v = refuse(ZKC_PTAU_CHECK_TAU_G1_G2, 3, 1, "ptau: tauG1[1] and tauG2[1] hold different tau: sameRatio(G1, tauG1[1]; G2, tauG2[1]) fails");
    else if (!ratio(R1, R2)) v = refuse(ZKC_PTAU_CHECK_TAU_G1, 2, 0, "ptau: section 2 is not the powers of one tau: sameRatio(R1, R2; G2, tauG2[1]) fails");
    else if (S1.is_inf() || S2.is_inf() || !pairing::same_ratio(G1, T.p1, S1, S2)) v = refuse(ZKC_PTAU_CHECK_TAU_G2, 3, 0, "ptau: section 3 is not the powers of one tau: sameRatio(G1, tauG1[1]; S1, S2) fails");
    else if (!ratio(A1, A2)) v = refuse(ZKC_PTAU_CHECK_ALPHA_TAU_G1, 4, 0, "ptau: section 4 is not alpha times the powers of one tau: sameRatio(A1, A2; G2, tauG2[1]) fails");
    else if (!ratio(B1, B2)) v = refuse(ZKC_PTAU_CHECK_BETA_TAU_G1, 5, 0, "ptau: section 5 is not beta times the powers of one tau: sameRatio(B1, B2; G2, tauG2[1]) fails");
    else if (!pairing::same_ratio(G1, B.p0, G2, beta2)) v = refuse(ZKC_PTAU_CHECK_BETA_G1_G2, 6, 0, "ptau: betaTauG1[0] and betaG2 hold different beta: sameRatio(G1, betaTauG1[0]; G2, betaG2) fails");
    g_ver_ms[5] += ms_since(t0);
    return v.failed() ? 0 : 1;
}

// open, lock, run, report: the body of zkc_ptau_verify and of the hook.  weights: n_weights x 16 B when given, else drawn from seed32 (NULL: the OS)
int verify_entry(const char* name, zkc_ctx* ctx, const char* path, const uint8_t* seed32, const uint8_t* weights16, uint64_t n_weights, bool given, uint32_t chunk, uint8_t* sums,
                 uint32_t* check, uint32_t* section, uint64_t* index, char* err, size_t errlen) {
    if (check) *check = ZKC_PTAU_CHECK_NONE;
    if (section) *section = 0;
    if (index) *index = 0;
    if (err && errlen) err[0] = 0;
    if (!path || (given && !weights16)) return -err_out(err, errlen, ZKC_ERR_BAD_ARG, std::string(name) + ": bad argument");
    for (double& m : g_ver_ms) m = 0;
    const clk::time_point t0 = clk::now();
    parse::Ptau pt; std::string why;
    if (!parse::ptau_open(path, pt, why, false)) return -setup_fail(err, errlen, why);      // sections 2 .. 6 are there and of the power's lengths; power >= 1
    g_ver_ms[0] += ms_since(t0);
    const uint64_t nw = 2 * (1ull << pt.power) - 2;
    if (given && n_weights != nw) return -err_out(err, errlen, ZKC_ERR_BAD_ARG, std::string(name) + ": a file of power " + std::to_string(pt.power) + " takes " + std::to_string(nw) + " weights");
    std::vector<uint8_t> drawn;
    if (!given) {                                               // the file is fixed (it is open) before the weights are drawn
        drawn.resize(16 * (size_t)nw);
        const std::vector<uint32_t> rho = verify_weights(seed32, (size_t)nw);
        for (size_t i = 0; i < nw; i++) memcpy(&drawn[16 * i], &rho[8 * i], 16);
        weights16 = drawn.data();
    }
    if (!chunk) chunk = CHUNK;
    Verdict v; int res;
    if (ctx) {
        ZKC_LOCK(ctx);
        if (hipSetDevice(ctx->device) != hipSuccess) return -err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, std::string(name) + ": hipSetDevice"), zkc_last_error(ctx));
        res = verify_file(ctx, pt, weights16, chunk, v, sums, err, errlen);
    } else res = verify_file(nullptr, pt, weights16, chunk, v, sums, err, errlen);
    if (res == 0) {
        if (check) *check = v.check;
        if (section) *section = v.section;
        if (index) *index = v.index;
        err_out(err, errlen, 0, v.text);
    }
    return res;
}

// the body of the two engines
template <class F>
int wsum_entry(zkc_ctx* ctx, const void* d_points, uint32_t n, int mont, const void* d_weights16, uint8_t* out_lo, uint8_t* out_hi) {
    const std::string name = GroupOf<F>::g2 ? "zkc_g2_wsum_pair_dev" : "zkc_g1_wsum_pair_dev";
    if (!ctx || !d_points || !d_weights16 || !out_lo || !out_hi || n < 2) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, name + ": bad argument");
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    constexpr size_t PT = sizeof(Affine<F>);
    DevBuf conv; int rc;
    const void* src = d_points;
    if (!mont) {
        if ((rc = conv.alloc(ctx, (size_t)n * PT)) || (rc = coords_to_mont(ctx, d_points, conv.p, (size_t)n * (PT / 32)))) return rc;
        src = conv.p;
    }
    uint32_t bad = 0;
    if ((rc = points_check_dev<F>(ctx, src, n, &bad))) return rc;
    if (bad != NONE) return zkc_fail(ctx, ZKC_ERR_FORMAT, name + ": point " + std::to_string(bad) + " has a coordinate >= q or is not on the " + GroupOf<F>::curve);
    Affine<F> out[2];
    if ((rc = wsum_dev<F>(ctx, src, n, d_weights16, out))) return rc;
    if constexpr (GroupOf<F>::g2) { wr_g2_std(out_lo, out[0]); wr_g2_std(out_hi, out[1]); }
    else { wr_g1_std(out_lo, out[0]); wr_g1_std(out_hi, out[1]); }
    return ZKC_OK;
}

}  // namespace

extern "C" int zkc_g1_wsum_pair_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, int mont, const void* d_weights16, uint8_t out_lo[64], uint8_t out_hi[64]) {
    return wsum_entry<Fq>(ctx, d_points, n, mont, d_weights16, out_lo, out_hi);
}
extern "C" int zkc_g2_wsum_pair_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, int mont, const void* d_weights16, uint8_t out_lo[128], uint8_t out_hi[128]) {
    return wsum_entry<Fq2>(ctx, d_points, n, mont, d_weights16, out_lo, out_hi);
}

extern "C" int zkc_ptau_verify(zkc_ctx* ctx, const char* ptau_path, const uint8_t* seed32, uint32_t* check, uint32_t* section, uint64_t* index, char* err, size_t errlen) {
    return verify_entry("zkc_ptau_verify", ctx, ptau_path, seed32, nullptr, 0, false, 0, nullptr, check, section, index, err, errlen);
}

extern "C" int zkc_debug_ptau_verify(zkc_ctx* ctx, const char* ptau_path, const uint8_t* weights16, uint64_t n_weights, uint32_t chunk_terms, uint8_t* sums_out, uint32_t* check,
                                     uint32_t* section, uint64_t* index, char* err, size_t errlen) {
    return verify_entry("zkc_debug_ptau_verify", ctx, ptau_path, nullptr, weights16, n_weights, true, chunk_terms, sums_out, check, section, index, err, errlen);
}

extern "C" int zkc_ptau_verify_stats(double ms[6]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 6; i++) ms[i] = g_ver_ms[i];
    return ZKC_OK;
}
