// zkc_setup_ptau.hip -- Groth16 keys from a prepared powers-of-tau file (include/zkcensus_ptau.h): `snarkjs groth16 setup` and the whole of `snarkjs zkey verify`
// (circuit/circuit-compiler.sh:99-136).  Product code: host stages around one new kind of kernel, a sparse matrix times a vector of POINTS.
//
// The key of zkc_setup.hip is scalars times one generator, because the generator knows tau, alpha, beta.  Here nobody does: they exist only as the Lagrange-basis points
// L_c = L_c(tau) G1, La_c = alpha L_c(tau) G1, Lb_c = beta L_c(tau) G1, L2_c = L_c(tau) G2 of the file, and every point of the key is a sum of coefficient x point over
// one wire's column of the constraint matrices (the formulas: zkcensus_ptau.h).  Stages:
//   1 (host)  read the .r1cs whole and, of the .ptau, the section table and the five ranges the circuit needs (zkc_ptau_parse.h: pread, 64-bit offsets)
//   2 (host)  transpose to rows by wire.  G1 group: 3 nWires + 3 rows (A | B1 | K | the three partition-of-unity sums) over the points L | La | Lb | H; G2 group:
//             nWires + 1 rows (B2 | sum) over L2.  A term is a 32-bit word: the index of its point, bit 31 = subtract.  Coefficients +1 and r - 1 are such a word as
//             they are.  Any other coefficient k becomes a SCALE JOB (min(k, r - k), point) whose product is appended to the group's points, and the term names that;
//             the jobs are sorted by scalar, so the lanes of a wave walk bit strings of the same length and largely the same bits.  Rows are ordered by decreasing
//             length (jds_layout, zkc_jds.h: neighbouring lanes get equal work) and cut into SEGMENTS of at most SEG terms.
//   3 (GPU, or host threads with ctx = NULL)
//             check      one lane per point read: coordinates < q, on the curve; the smallest bad index comes back (the file is not trusted; points_check_dev)
//             scale      one lane per job: double-and-add from the scalar's leading bit, f29_acc_dbl / f29_madd (G2: f29g2_pt_dbl / f29g2_madd_lean) as zkc_p2_scale_g1;
//                        the products become affine through the batched inversion of the fixed-base engine and land behind the points read
//             accumulate one lane per segment: mixed additions of +-P into an XYZZ partial sum
//             reduce     one lane per up to RED partial sums of one row (full additions), repeated until every row has one: rows of more than SEG x RED terms -- the
//                        partition-of-unity sums from domain 2^11 on, wire 0 of a large circuit -- take a second, and from 32 769 terms a third
//             then affine again, and home in row order.
//   4 (host)  the sanity checks, csHash, and the shared writer (zkc_setup_write.h).
// Every loop of every kernel is bounded by a count the host computed; nothing waits on a flag.  SEG, RED are the only tunables.
//
// The additions: every exceptional case is handled, and the head of zkc_point_ops.h names the test that reaches each, per group.  Here K_s adds alpha L_c and beta L_c,
// which are EQUAL when alpha = beta and OPPOSITE when alpha = -beta (G1 only: tests/test_gpu_ptau_setup.py).  A wire named twice in one linear combination stays two terms
// (zkc_r1cs_parse.h), so a row can hold one point many times: tests/test_gpu_ptau_setup_repeats.py makes such rows and through them reaches, in G1 and in G2, equal and
// opposite points in the accumulation, equal and opposite partial sums at the first, second and third reduction step, and rows at each side of the third step.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "zkc_prover.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_f29.h"
#include "zkc_f29_g1.h"
#include "zkc_f29_g2.h"
#include "zkc_point_ops.h"
#include "zkc_point_red.h"
#include "zkc_pairing.h"
#include "zkc_file_points.h"
#include "zkc_jds.h"
#include "zkc_phase2_parse.h"
#include "zkc_ptau_parse.h"
#include "zkc_setup_write.h"
#include "../../include/zkcensus_phase2.h"
#include "../../include/zkcensus_ptau.h"

using namespace zkc;

namespace {

constexpr uint32_t SEG = 32;                     // terms per lane of the accumulation
// RED, the partial sums per lane of a reduction step: POINT_RED (zkc_point_red.h)
constexpr uint32_t T_NEG = 0x80000000u, T_IDX = 0x7fffffffu;

// ================================================================ device ================================================================

// load_words, all_zero, shl1_out, the two groups behind one interface (G1Ops, G2Ops) and add_point: zkc_point_ops.h

// ---- scale: out[j] = k_j * pts[src_j] as canonical XYZZ (infinity: all zero).  k_j: 8 words, standard form, 1 < k_j <= (r - 1) / 2 ----
template <class G> __global__ void __launch_bounds__(64)
zkc_ptau_scale(const uint32_t* __restrict__ pts, uint32_t npts, const uint32_t* __restrict__ ks, const uint32_t* __restrict__ src, uint32_t njobs, XYZZ<typename G::F>* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    XYZZ<typename G::F> o = XYZZ<typename G::F>::inf();
    const uint32_t idx = src[j];
    uint32_t k[8]; load_words<8>(k, ks + 8 * (size_t)j);
    uint32_t w[G::W];
    if (idx >= npts) { out[j] = o; return; }
    load_words<G::W>(w, pts + (size_t)G::W * idx);
    if (all_zero<G::W>(w) || all_zero<8>(k)) { out[j] = o; return; }
    const typename G::Pt p = G::enter(w, false);
    typename G::Acc acc; bool inf = true, started = false;
    // 256 steps from the top bit; the words move up one bit per step, so no register is indexed by the loop counter.  Until the leading one a step is eight shifts.
    for (int it = 0; it < 256; it++) {
        const uint32_t bit = shl1_out(k);
        if (!started) { if (bit) { G::set(acc, p); inf = false; started = true; } continue; }
        if (!inf) G::dbl(acc);                   // a doubling never meets infinity: the group has odd order
        if (bit) add_point<G>(acc, inf, p);
    }
    if (!inf) o = G::leave(acc);
    out[j] = o;
}

// ---- accumulate: part[s] = sum of the terms [seg_start[s], seg_start[s + 1]) (at most SEG of them), each +-pts[index] ----
template <class G> __global__ void __launch_bounds__(64)
zkc_ptau_acc(const uint32_t* __restrict__ pts, uint32_t npts, const uint32_t* __restrict__ terms, const uint32_t* __restrict__ seg_start, uint32_t nseg, XYZZ<typename G::F>* __restrict__ part) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint32_t t0 = seg_start[s]; uint32_t t1 = seg_start[s + 1];
    if (t1 - t0 > SEG) t1 = t0 + SEG;            // the host never makes a longer one
    typename G::Acc acc; bool inf = true;
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t word = terms[t], idx = word & T_IDX;
        if (idx >= npts) continue;
        uint32_t w[G::W]; load_words<G::W>(w, pts + (size_t)G::W * idx);
        if (all_zero<G::W>(w)) continue;
        const typename G::Pt p = G::enter(w, (word & T_NEG) != 0);
        add_point<G>(acc, inf, p);
    }
    XYZZ<typename G::F> o = XYZZ<typename G::F>::inf();
    if (!inf) o = G::leave(acc);
    part[s] = o;
}

// ---- reduce: zkc_ptau_red, shared with zkc_ptau_verify.hip (zkc_point_red.h) ----

// ================================================================ host ================================================================

thread_local double g_ptau_ms[6] = {0, 0, 0, 0, 0, 0};

// par_chunks (at most HOST_THREADS threads): zkc_host_util.h

// ---- stage 2: the rows of one group ----
struct GenTerm { uint32_t row, word; uint32_t k[8]; };          // word: the SOURCE point (and the sign) until the jobs are numbered
struct Builder {
    uint32_t nbase = 0, nrows = 0;
    std::vector<std::pair<uint32_t, uint32_t>> unit;            // (row, word)
    std::vector<GenTerm> gen;
    Fr one = Fr::one(), minus_one = fp_neg(Fr::one());
    uint32_t half[8];                                           // (r - 1) / 2
    Builder() { for (int i = 0; i < 8; i++) half[i] = (FrParams::p[i] >> 1) | (i < 7 ? FrParams::p[i + 1] << 31 : 0); }
    void add(uint32_t row, const Fr& coef, uint32_t src) {
        if (coef.is_zero()) return;
        if (coef == one) { unit.emplace_back(row, src); return; }
        if (coef == minus_one) { unit.emplace_back(row, src | T_NEG); return; }
        GenTerm g; g.row = row; g.word = src;
        fp_to_std<FrParams>(g.k, coef);
        if (std_less(half, g.k)) { fp_to_std<FrParams>(g.k, fp_neg(coef)); g.word |= T_NEG; }       // k > (r - 1) / 2: -(r - k) P, the shorter chain for -2, -3, ...
        gen.push_back(g);
    }
};
struct Plan {
    uint32_t nbase = 0, nrows = 0, nseg = 0;
    std::vector<uint32_t> jobk, jobsrc;                         // scale jobs, sorted by scalar: 8 words each, and the source point
    std::vector<uint32_t> perm;                                 // sorted position -> row
    std::vector<uint32_t> terms, seg_start, rowseg;             // rowseg[p] .. rowseg[p + 1]: the segments of the row at sorted position p
    uint64_t nunit = 0, ngen = 0;
    uint32_t njobs() const { return (uint32_t)jobsrc.size(); }
};
bool make_plan(Builder& B, Plan& P, std::string& why) {
    P.nbase = B.nbase; P.nrows = B.nrows; P.nunit = B.unit.size(); P.ngen = B.gen.size();
    if ((uint64_t)B.nbase + B.gen.size() > T_IDX || (uint64_t)B.unit.size() + B.gen.size() > 0xfffffff0ull) { why = "circuit too large for 32-bit term words"; return false; }
    std::stable_sort(B.gen.begin(), B.gen.end(), [](const GenTerm& a, const GenTerm& b) { return std_less(a.k, b.k); });
    const size_t nj = B.gen.size();
    P.jobk.resize(8 * nj); P.jobsrc.resize(nj);
    std::vector<uint32_t> len(B.nrows, 0);
    for (auto& u : B.unit) len[u.first]++;
    for (size_t j = 0; j < nj; j++) { memcpy(&P.jobk[8 * j], B.gen[j].k, 32); P.jobsrc[j] = B.gen[j].word & T_IDX; len[B.gen[j].row]++; }
    const JdsLayout J = jds_layout(B.nrows, [&](uint32_t r) { return len[r]; }, SEG);
    P.perm = J.perm;
    std::vector<uint32_t> fill(B.nrows);                        // by ROW: where its next term goes
    P.rowseg.assign((size_t)B.nrows + 1, 0);
    uint32_t at = 0;
    for (uint32_t p = 0; p < B.nrows; p++) {
        fill[J.perm[p]] = at;
        const uint32_t l = J.rowlen[p], ns = (l + SEG - 1) / SEG;
        for (uint32_t s = 0; s < ns; s++) P.seg_start.push_back(at + s * SEG);
        P.rowseg[p + 1] = P.rowseg[p] + ns;
        at += l;
    }
    P.seg_start.push_back(at); P.nseg = P.rowseg[B.nrows];
    P.terms.resize(at);
    for (auto& u : B.unit) P.terms[fill[u.first]++] = u.second;
    for (size_t j = 0; j < nj; j++) P.terms[fill[B.gen[j].row]++] = (B.nbase + (uint32_t)j) | (B.gen[j].word & T_NEG);
    B.unit.clear(); B.unit.shrink_to_fit(); B.gen.clear(); B.gen.shrink_to_fit();
    return true;
}

// the reduction steps of a plan (reduction_steps, zkc_point_red.h): the partial sums of the row at sorted position p are its segments
std::vector<uint32_t> row_counts(const Plan& P) {
    std::vector<uint32_t> cnt(P.nrows);
    for (uint32_t p = 0; p < P.nrows; p++) cnt[p] = P.rowseg[p + 1] - P.rowseg[p];
    return cnt;
}

// ---- stage 3 on host threads (zkc_curve.h), over the same plan ----
// host_first_bad: zkc_file_points.h
template <class F>
void run_host(const Plan& P, std::vector<Affine<F>>& pts, std::vector<Affine<F>>& rows, uint32_t& bad, double ms[3]) {
    bad = host_first_bad<F>(pts.data(), P.nbase);
    if (bad != 0xffffffffu) return;
    const clk::time_point t0 = clk::now();
    pts.resize((size_t)P.nbase + P.njobs());
    par_chunks(P.njobs(), 16, [&](size_t a, size_t b) {
        for (size_t j = a; j < b; j++) pts[P.nbase + j] = xyzz_to_affine_gcd(xyzz_mul(XYZZ<F>::from_affine(pts[P.jobsrc[j]]), &P.jobk[8 * j]));
    });
    const clk::time_point t1 = clk::now();
    std::vector<XYZZ<F>> part(P.nseg);
    par_chunks(P.nseg, 64, [&](size_t a, size_t b) {
        for (size_t s = a; s < b; s++) {
            XYZZ<F> acc = XYZZ<F>::inf();
            for (uint32_t t = P.seg_start[s]; t < P.seg_start[s + 1]; t++) {
                const Affine<F>& p = pts[P.terms[t] & T_IDX];
                acc = xyzz_add_affine(acc, (P.terms[t] & T_NEG) ? affine_neg(p) : p);       // complete; the negative of the all-zero point is the all-zero point
            }
            part[s] = acc;
        }
    });
    std::vector<Affine<F>> sorted(P.nrows);
    par_chunks(P.nrows, 256, [&](size_t a, size_t b) {
        for (size_t p = a; p < b; p++) {
            XYZZ<F> acc = XYZZ<F>::inf();
            for (uint32_t s = P.rowseg[p]; s < P.rowseg[p + 1]; s++) acc = xyzz_add(acc, part[s]);
            sorted[p] = xyzz_to_affine_gcd(acc);
        }
    });
    rows.resize(P.nrows);
    for (uint32_t p = 0; p < P.nrows; p++) rows[P.perm[p]] = sorted[p];
    ms[0] = 0; ms[1] = ms_since(t0, t1); ms[2] = ms_since(t1);
}

// ---- stage 3 on the device.  The context's lock is held and the device is set.  ms: upload, scale, accumulate and reduce ----
template <class F>
int run_dev(zkc_ctx* ctx, const Plan& P, const std::vector<Affine<F>>& base, std::vector<Affine<F>>& rows, uint32_t& bad, double ms[3]) {
    typedef typename GroupOf<F>::Ops G;
    constexpr size_t PT = sizeof(Affine<F>);
    const uint32_t nj = P.njobs(), npts = P.nbase + nj;
    int rc;
    const clk::time_point t0 = clk::now();
    DevBuf pts, terms, seg;
    if ((rc = pts.alloc(ctx, (size_t)npts * PT)) || (rc = terms.alloc(ctx, P.terms.size() * 4)) || (rc = seg.alloc(ctx, P.seg_start.size() * 4))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpy(pts.p, base.data(), (size_t)P.nbase * PT, hipMemcpyHostToDevice));
    if (!P.terms.empty()) ZKC_HIP_CHECK(ctx, hipMemcpy(terms.p, P.terms.data(), P.terms.size() * 4, hipMemcpyHostToDevice));
    ZKC_HIP_CHECK(ctx, hipMemcpy(seg.p, P.seg_start.data(), P.seg_start.size() * 4, hipMemcpyHostToDevice));
    if ((rc = points_check_dev<F>(ctx, pts.p, P.nbase, &bad))) return rc;
    if (bad != 0xffffffffu) return ZKC_OK;                     // the caller names the point
    const clk::time_point t1 = clk::now();
    if (nj) {
        DevBuf ks, src, prod;
        if ((rc = ks.alloc(ctx, (size_t)nj * 32)) || (rc = src.alloc(ctx, (size_t)nj * 4)) || (rc = prod.alloc(ctx, (size_t)nj * sizeof(XYZZ<F>)))) return rc;
        ZKC_HIP_CHECK(ctx, hipMemcpy(ks.p, P.jobk.data(), (size_t)nj * 32, hipMemcpyHostToDevice));
        ZKC_HIP_CHECK(ctx, hipMemcpy(src.p, P.jobsrc.data(), (size_t)nj * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(zkc_ptau_scale<G>, dim3((nj + 63) / 64), dim3(64), 0, ctx->stream, pts.as<uint32_t>(), P.nbase, ks.as<uint32_t>(), src.as<uint32_t>(), nj, prod.as<XYZZ<F>>());
        ZKC_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = fixed_affine<F>(ctx, prod.as<XYZZ<F>>(), nj, (uint8_t*)pts.p + (size_t)P.nbase * PT, true))) return rc;      // synchronises
    }
    const clk::time_point t2 = clk::now();
    DevBuf cur;
    if ((rc = cur.alloc(ctx, (size_t)P.nseg * sizeof(XYZZ<F>)))) return rc;
    if (P.nseg) {
        hipLaunchKernelGGL(zkc_ptau_acc<G>, dim3((P.nseg + 63) / 64), dim3(64), 0, ctx->stream, pts.as<uint32_t>(), npts, terms.as<uint32_t>(), seg.as<uint32_t>(), P.nseg, cur.as<XYZZ<F>>());
        ZKC_HIP_CHECK(ctx, hipGetLastError());
    }
    if ((rc = point_reduce<F>(ctx, cur, row_counts(P)))) return rc;
    // cur: one sum per sorted row
    DevBuf aff;
    if ((rc = aff.alloc(ctx, (size_t)P.nrows * PT)) || (rc = fixed_affine<F>(ctx, cur.as<XYZZ<F>>(), P.nrows, aff.p, true))) return rc;
    std::vector<Affine<F>> sorted(P.nrows);
    ZKC_HIP_CHECK(ctx, hipMemcpy(sorted.data(), aff.p, (size_t)P.nrows * PT, hipMemcpyDeviceToHost));
    rows.resize(P.nrows);
    for (uint32_t p = 0; p < P.nrows; p++) rows[P.perm[p]] = sorted[p];
    ms[0] = ms_since(t0, t1); ms[1] = ms_since(t1, t2); ms[2] = ms_since(t2);
    return ZKC_OK;
}

template <class F> bool same_point(const Affine<F>& a, const Affine<F>& b) { return a.x == b.x && a.y == b.y; }

// csHash of the initial key: the serialisation of zkcensus_ptau.h
void circuit_hash(const SetupScalars& S, const SetupPoints& P, uint8_t out[64]) {
    parse::Blake2b h; uint8_t u[128];
    auto g1 = [&](const G1Affine& p) { unc_g1(u, p); h.update(u, 64); };
    auto g2 = [&](const G2Affine& p) { unc_g2(u, p); h.update(u, 128); };
    auto count = [&](size_t n) { const uint8_t b[4] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n}; h.update(b, 4); };
    g1(P.alpha1); g1(P.beta1); g2(P.beta2); g2(P.gamma2); g1(P.delta1); g2(P.delta2);
    count(S.nPub + 1); for (uint32_t i = 0; i <= S.nPub; i++) g1(P.pC[i]);
    count(P.pH.size()); for (auto& p : P.pH) g1(p);
    count(S.nWires - S.nPub - 1); for (uint32_t i = S.nPub + 1; i < S.nWires; i++) g1(P.pC[i]);
    count(P.pA.size()); for (auto& p : P.pA) g1(p);
    count(P.pB1.size()); for (auto& p : P.pB1) g1(p);
    count(P.pB2.size()); for (auto& p : P.pB2) g2(p);
    h.final(out);
}

// stages 1 to 4 without the writing: the initial key of (r1cs, ptau).  ctx = NULL: host threads
int derive_key(zkc_ctx* ctx, const char* r1cs_path, const char* ptau_path, SetupScalars& S, SetupPoints& K, uint8_t cs_hash[64], char* err, size_t errlen) {
    for (double& m : g_ptau_ms) m = 0;
    // ---- 1: read ----
    const clk::time_point t0 = clk::now();
    std::vector<uint8_t> buf; int rc;
    if ((rc = read_file(r1cs_path, buf, err, errlen)) || (rc = setup_circuit(buf, S, err, errlen))) return rc;
    buf.clear(); buf.shrink_to_fit();
    const uint32_t nW = S.nWires, nPub = S.nPub, nCons = S.nCons, n = S.n;
    uint32_t logn = 0; while ((1u << logn) < n) logn++;
    if (nW > 0x20000000u) return setup_fail(err, errlen, "zkc_setup_from_ptau: circuit too large");
    parse::Ptau pt; std::string why;
    if (!parse::ptau_open(ptau_path, pt, why) || !parse::ptau_fits(pt, logn, why)) return setup_fail(err, errlen, why);
    std::vector<G1Affine> pts1((size_t)4 * n);                  // L | La | Lb | H
    std::vector<G2Affine> pts2(n);                              // L2
    G1Affine alpha1, beta1; G2Affine beta2;
    {
        std::vector<G1Affine> big((size_t)2 * n);
        if (!parse::ptau_read_lagrange(pt, 12, logn, pts1.data(), why) || !parse::ptau_read_lagrange(pt, 14, logn, pts1.data() + n, why) ||
            !parse::ptau_read_lagrange(pt, 15, logn, pts1.data() + 2 * (size_t)n, why) || !parse::ptau_read_lagrange(pt, 12, logn + 1, big.data(), why) ||
            !parse::ptau_read_lagrange(pt, 13, logn, pts2.data(), why) || !parse::ptau_read(pt, 4, 0, 1, &alpha1, why) || !parse::ptau_read(pt, 5, 0, 1, &beta1, why) ||
            !parse::ptau_read(pt, 6, 0, 1, &beta2, why)) return setup_fail(err, errlen, why);
        for (uint32_t i = 0; i < n; i++) pts1[3 * (size_t)n + i] = big[2 * (size_t)i + 1];
    }
    if (!host_point_ok<Fq>(alpha1) || alpha1.is_inf()) return setup_fail(err, errlen, "ptau: section 4 point 0 (alpha G1) has a coordinate >= q, is off the curve or at infinity");
    if (!host_point_ok<Fq>(beta1) || beta1.is_inf()) return setup_fail(err, errlen, "ptau: section 5 point 0 (beta G1) has a coordinate >= q, is off the curve or at infinity");
    if (!host_point_ok<Fq2>(beta2) || beta2.is_inf() || !pairing::g2_in_subgroup(beta2)) return setup_fail(err, errlen, "ptau: section 6 point 0 (beta G2) has a coordinate >= q, is not in G2 or at infinity");
    // ---- 2: rows by wire ----
    const clk::time_point t1 = clk::now();
    Plan P1, P2;
    {
        Builder B1, B2;
        B1.nbase = 4 * n; B1.nrows = 3 * nW + 3; B2.nbase = n; B2.nrows = nW + 1;
        for (uint32_t k = 0; k < nCons; k++) {
            for (auto& t : S.cons[k].a) { B1.add(t.wire, t.coef, k); B1.add(2 * nW + t.wire, t.coef, 2 * n + k); }
            for (auto& t : S.cons[k].b) { B1.add(nW + t.wire, t.coef, k); B1.add(2 * nW + t.wire, t.coef, n + k); B2.add(t.wire, t.coef, k); }
            for (auto& t : S.cons[k].c) B1.add(2 * nW + t.wire, t.coef, k);
        }
        for (uint32_t i = 0; i <= nPub; i++) { B1.add(i, B1.one, nCons + i); B1.add(2 * nW + i, B1.one, 2 * n + nCons + i); }      // snarkjs' extra rows A[nCons + i][i] = 1
        for (uint32_t c = 0; c < n; c++) { B1.add(3 * nW, B1.one, c); B1.add(3 * nW + 1, B1.one, n + c); B1.add(3 * nW + 2, B1.one, 2 * n + c); B2.add(nW, B2.one, c); }
        if (!make_plan(B1, P1, why) || !make_plan(B2, P2, why)) return setup_fail(err, errlen, "zkc_setup_from_ptau: " + why);
    }
    // ---- 3: the sums ----
    const clk::time_point t2 = clk::now();
    std::vector<G1Affine> r1; std::vector<G2Affine> r2;
    uint32_t bad1 = 0xffffffffu, bad2 = 0xffffffffu; double m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0};
    if (ctx) {
        ZKC_LOCK(ctx);
        if (hipSetDevice(ctx->device) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_setup_from_ptau: hipSetDevice"), zkc_last_error(ctx));
        if ((rc = run_dev<Fq>(ctx, P1, pts1, r1, bad1, m1)) || (bad1 == 0xffffffffu && (rc = run_dev<Fq2>(ctx, P2, pts2, r2, bad2, m2)))) return err_out(err, errlen, rc, zkc_last_error(ctx));
    } else {
        run_host<Fq>(P1, pts1, r1, bad1, m1);
        if (bad1 == 0xffffffffu) run_host<Fq2>(P2, pts2, r2, bad2, m2);
    }
    if (bad1 != 0xffffffffu) {
        const uint32_t blk = bad1 / n, i = bad1 % n; const int sec = blk == 1 ? 14 : blk == 2 ? 15 : 12;
        const uint64_t at = blk == 3 ? (2ull * n - 1) + 2ull * i + 1 : (uint64_t)(n - 1) + i;
        return setup_fail(err, errlen, "ptau: section " + std::to_string(sec) + " point " + std::to_string(at) + " has a coordinate >= q or is not on the curve");
    }
    if (bad2 != 0xffffffffu) return setup_fail(err, errlen, "ptau: section 13 point " + std::to_string((uint64_t)(n - 1) + bad2) + " has a coordinate >= q or is not on the twist");
    // ---- 4: checks ----
    const clk::time_point t3 = clk::now();
    const G1Affine G1 = g1_generator(); const G2Affine G2 = g2_generator();
    if (!same_point(r1[3 * (size_t)nW], G1)) return setup_fail(err, errlen, "ptau: the tau G1 Lagrange basis of size 2^" + std::to_string(logn) + " (section 12) does not sum to the G1 generator");
    if (!same_point(r2[nW], G2)) return setup_fail(err, errlen, "ptau: the tau G2 Lagrange basis of size 2^" + std::to_string(logn) + " (section 13) does not sum to the G2 generator");
    if (!same_point(r1[3 * (size_t)nW + 1], alpha1)) return setup_fail(err, errlen, "ptau: the alpha tau G1 Lagrange basis of size 2^" + std::to_string(logn) + " (section 14) does not sum to alphaTauG1[0]");
    if (!same_point(r1[3 * (size_t)nW + 2], beta1)) return setup_fail(err, errlen, "ptau: the beta tau G1 Lagrange basis of size 2^" + std::to_string(logn) + " (section 15) does not sum to betaTauG1[0]");
    if (!pairing::same_ratio(G1, beta1, G2, beta2)) return setup_fail(err, errlen, "ptau: sameRatio(G1, betaTauG1[0]; G2, betaG2) fails");
    K.pA.assign(r1.begin(), r1.begin() + nW); K.pB1.assign(r1.begin() + nW, r1.begin() + 2 * (size_t)nW); K.pC.assign(r1.begin() + 2 * (size_t)nW, r1.begin() + 3 * (size_t)nW);
    K.pH.assign(pts1.begin() + 3 * (size_t)n, pts1.begin() + 4 * (size_t)n); K.pB2.assign(r2.begin(), r2.begin() + nW);
    K.alpha1 = alpha1; K.beta1 = beta1; K.beta2 = beta2; K.delta1 = G1; K.gamma2 = G2; K.delta2 = G2;
    circuit_hash(S, K, cs_hash);
    g_ptau_ms[0] = ms_since(t0, t1); g_ptau_ms[1] = ms_since(t1, t2); g_ptau_ms[2] = m1[0] + m2[0]; g_ptau_ms[3] = m1[1] + m2[1]; g_ptau_ms[4] = m1[2] + m2[2];
    g_ptau_ms[5] = ms_since(t3);
    return ZKC_OK;
}

}  // namespace

extern "C" int zkc_setup_from_ptau(zkc_ctx* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen) {
    if (!r1cs_path || !ptau_path || !zkey_path) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_setup_from_ptau: bad argument");
    SetupScalars S; SetupPoints K; uint8_t cs[64];
    int rc = derive_key(ctx, r1cs_path, ptau_path, S, K, cs, err, errlen); if (rc) return rc;
    const clk::time_point t0 = clk::now();
    rc = setup_write(S, K, zkey_path, vkey_json_path, err, errlen, cs);
    g_ptau_ms[5] += ms_since(t0);
    return rc;
}

extern "C" int zkc_zkey_verify_circuit(zkc_ctx* ctx, const char* r1cs_path, const char* ptau_path, const void* final_, size_t final_len, const uint8_t* seed32, uint32_t* n_new,
                                       char* err, size_t errlen) {
    if (n_new) *n_new = 0;
    if (!ctx || !r1cs_path || !ptau_path || !final_) return err_out(err, errlen, -ZKC_ERR_BAD_ARG, "zkc_zkey_verify_circuit: bad argument");
    SetupScalars S; SetupPoints K; uint8_t cs[64];
    const int rc = derive_key(ctx, r1cs_path, ptau_path, S, K, cs, err, errlen);
    if (rc) return -rc;
    const std::vector<uint8_t> init = setup_image(S, K, cs);
    return zkc_zkey_verify_contributions(ctx, init.data(), init.size(), final_, final_len, seed32, n_new, err, errlen);
}

extern "C" int zkc_setup_ptau_stats(double ms[6]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 6; i++) ms[i] = g_ptau_ms[i];
    return ZKC_OK;
}
