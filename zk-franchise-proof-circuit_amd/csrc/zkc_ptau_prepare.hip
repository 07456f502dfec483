// zkc_ptau_prepare.hip -- a powers-of-tau file prepared for phase 2 (include/zkcensus_ptau_prepare.h): `snarkjs powersoftau prepare phase2`
// (circuit/circuit-compiler.sh:71), and the check that the Lagrange sections of a prepared file are the transforms of its monomial sections.  Product code: host stages
// around the transform over points of zkc_ecntt.hip.
//
// Both entry points are one walk over the four families (12 from 2, 13 from 3, 14 from 4, 15 from 5).  Per family:
//   1 (host)  read the monomial section whole (zkc_ptau_parse.h).  Section 2 is one point short of its largest block, 2^(power+1): the missing point is left all zero,
//             infinity -- the padded top block of zkcensus_ptau_prepare.h
//   2         check every point read: coordinates < q, on its curve (GPU: upload, points_check_dev; ctx = NULL: host_first_bad on host threads); the smallest bad index is named
//   3         for p = 0 .. power (section 12: power + 1) the transform of the first 2^p points: on the GPU ecntt<F> over the section resident on the device,
//             one block at a time and each downloaded as it is done; with ctx = NULL the same butterflies with zkc_curve.h on at most HOST_THREADS threads
//   4 (host)  prepare: the block goes into the section's image, which is written when the family is done (zkc_ptau_write.h); check_prepared: the block is compared with
//             the stored one and the walk ends at the first point that differs.
// Host and device leave canonical affine bytes, so the two paths write the same file.
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "zkc_prover.h"
#include "zkc_ecntt.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_point_ops.h"
#include "zkc_host_util.h"
#include "zkc_pairing.h"
#include "zkc_file_points.h"
#include "zkc_ptau_parse.h"
#include "zkc_ptau_write.h"
#include "zkc_setup_write.h"
#include "../../include/zkcensus_ptau_prepare.h"

using namespace zkc;

namespace {

thread_local double g_prep_ms[6] = {0, 0, 0, 0, 0, 0};

// ---- stage 3 on host threads: out[c] = 1/n sum_i w^(-c i) in[i], n = 2^logn, as zkc_ecntt.hip computes it (1/n at the input, decimation in time, unit twiddles free) ----
template <class F>
void host_lagrange(const Affine<F>* in, uint32_t logn, Affine<F>* out) {
    const uint32_t n = 1u << logn;                              // logn <= 28: ptau_open has refused power 28, whose top block would need a 2^29-th root
    uint32_t ninv[8]; fp_to_std<FrParams>(ninv, fp_inv<FrParams>(fp_from_u32<FrParams>(n)));
    std::vector<XYZZ<F>> v(n);
    auto brev = [&](uint32_t i) { uint32_t r = 0; for (uint32_t b = 0; b < logn; b++) r |= ((i >> b) & 1u) << (logn - 1 - b); return r; };
    par_chunks(n, 8, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) v[brev((uint32_t)i)] = xyzz_mul(XYZZ<F>::from_affine(in[i]), ninv); });
    std::vector<uint32_t> tw;                                   // w^-k, k < n / 2, standard form
    if (logn >= 2) {
        tw.resize((size_t)8 * (n / 2));
        const Fr wi = fp_inv<FrParams>(fr_root_of_unity((int)logn)); Fr x = Fr::one();
        for (uint32_t k = 0; k < n / 2; k++) { fp_to_std<FrParams>(&tw[8 * (size_t)k], x); x = x * wi; }
    }
    for (uint32_t s = 0; s < logn; s++) {
        const uint32_t half = 1u << s;
        par_chunks(n / 2, 8, [&](size_t j0, size_t j1) {
            for (size_t j = j0; j < j1; j++) {
                const uint32_t k = (uint32_t)j & (half - 1);
                const size_t a = ((j >> s) << (s + 1)) | k, b = a + half;
                const XYZZ<F> P = v[a], Q = k ? xyzz_mul(v[b], &tw[8 * ((size_t)k << (logn - 1 - s))]) : v[b];
                v[a] = xyzz_add(P, Q); v[b] = xyzz_add(P, xyzz_neg(Q));
            }
        });
    }
    par_chunks(n, 64, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) out[i] = xyzz_to_affine_gcd(v[i]); });
}

// what the walk hands over: block p of section `sec`, 2^p points of PT bytes.  false ends the walk (the walk then returns ZKC_OK: the callback has kept its verdict)
typedef std::function<bool(int sec, uint32_t p, const uint8_t* bytes, size_t nbytes)> BlockFn;

// one family.  The context's lock is held and the device is set when ctx != NULL.  d_tw: ecntt_twiddles of tw_logn = power + 1.  *go = false: the callback ended the walk
template <class F>
int family(zkc_ctx* ctx, const parse::Ptau& pt, int sec, const Fr* d_tw, uint32_t tw_logn, const BlockFn& fn, bool* go, char* err, size_t errlen) {
    typedef GroupOf<F> G;
    constexpr size_t PT = sizeof(Affine<F>);
    const int mono = parse::ptau_monomial_of(sec);
    const uint32_t last = parse::ptau_last_block(sec, pt.power);
    const uint64_t npts = parse::ptau_section_points(mono, pt.power), nmax = 1ull << last;      // npts = nmax, or nmax - 1 for section 2
    int rc; std::string why;
    // ---- 1 ----
    clk::time_point t0 = clk::now();
    std::vector<Affine<F>> in(nmax);
    memset((void*)in.data(), 0, nmax * PT);
    if (!parse::ptau_read(pt, mono, 0, npts, in.data(), why)) return setup_fail(err, errlen, why);
    g_prep_ms[0] += ms_since(t0);
    // ---- 2 ----
    t0 = clk::now();
    uint32_t bad = 0xffffffffu;
    DevBuf d_in, d_out;
    if (ctx) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_prepare: hipMemGetInfo"), zkc_last_error(ctx));
        const uint64_t need = 2 * nmax * PT + ecntt_work_bytes(last, G::g2) + (64u << 20);
        if (need > free_b) return setup_fail(err, errlen, "ptau: the size-2^" + std::to_string(last) + " block of section " + std::to_string(sec) + " does not fit the device's free memory (" +
                                             std::to_string(need >> 20) + " MB needed, " + std::to_string(free_b >> 20) + " MB free)");
        if ((rc = d_in.alloc(ctx, nmax * PT)) || (rc = d_out.alloc(ctx, nmax * PT))) return err_out(err, errlen, rc, zkc_last_error(ctx));
        if (hipMemcpy(d_in.p, in.data(), nmax * PT, hipMemcpyHostToDevice) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_prepare: upload"), zkc_last_error(ctx));
        if ((rc = points_check_dev<F>(ctx, d_in.p, (uint32_t)nmax, &bad))) return err_out(err, errlen, rc, zkc_last_error(ctx));
    } else bad = host_first_bad<F>(in.data(), npts);
    g_prep_ms[1] += ms_since(t0);
    if (bad != 0xffffffffu) return setup_fail(err, errlen, "ptau: section " + std::to_string(mono) + " point " + std::to_string(bad) + " has a coordinate >= q or is not on the " + G::curve);
    // ---- 3, 4 ----
    std::vector<Affine<F>> blk(nmax);
    double* tms = &g_prep_ms[G::g2 ? 3 : 2];
    for (uint32_t p = 0; p <= last && *go; p++) {
        const size_t n = (size_t)1 << p;
        if (ctx) {
            double ms[2] = {0, 0};
            if ((rc = ecntt<F>(ctx, d_in.p, p, d_tw, tw_logn, d_out.p, true, ms))) return err_out(err, errlen, rc, zkc_last_error(ctx));
            t0 = clk::now();
            if (hipMemcpy((void*)blk.data(), d_out.p, n * PT, hipMemcpyDeviceToHost) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_prepare: download"), zkc_last_error(ctx));
            *tms += ms[0]; g_prep_ms[4] += ms[1] + ms_since(t0);
        } else {
            t0 = clk::now();
            host_lagrange<F>(in.data(), p, blk.data());
            *tms += ms_since(t0);
        }
        t0 = clk::now();
        *go = fn(sec, p, (const uint8_t*)blk.data(), n * PT);
        g_prep_ms[5] += ms_since(t0);
    }
    return ZKC_OK;
}

// the four families in the order 12, 13, 14, 15
int walk(zkc_ctx* ctx, const parse::Ptau& pt, const BlockFn& fn, const std::function<bool(int sec)>& after, char* err, size_t errlen) {
    DevBuf tw; int rc; bool go = true;
    if (ctx && (rc = ecntt_twiddles(ctx, pt.power + 1, (Fr**)&tw.p))) return err_out(err, errlen, rc, zkc_last_error(ctx));
    for (int sec = 12; sec <= 15 && go; sec++) {
        rc = sec == 13 ? family<Fq2>(ctx, pt, sec, tw.as<Fr>(), pt.power + 1, fn, &go, err, errlen) : family<Fq>(ctx, pt, sec, tw.as<Fr>(), pt.power + 1, fn, &go, err, errlen);
        if (rc) return rc;
        if (go && !after(sec)) return ZKC_ERR_FORMAT;           // the callback has set err
    }
    return ZKC_OK;
}

}  // namespace

extern "C" int zkc_ptau_prepare(zkc_ctx* ctx, const char* in_path, const char* out_path, char* err, size_t errlen) {
    if (!in_path || !out_path) return err_out(err, errlen, ZKC_ERR_BAD_ARG, "zkc_ptau_prepare: bad argument");
    for (double& m : g_prep_ms) m = 0;
    clk::time_point t0 = clk::now();
    parse::Ptau pt; std::string why;
    if (!parse::ptau_open(in_path, pt, why, false, parse::PTAU_MAX_PREPARE_POWER)) return setup_fail(err, errlen, why);
    for (int id = 12; id <= 15; id++)
        if (pt.have[id]) return setup_fail(err, errlen, "ptau: the file is already prepared (it has section " + std::to_string(id) + ")");
    g_prep_ms[0] += ms_since(t0);
    t0 = clk::now();
    parse::PtauOut out;
    if (!parse::ptau_out_begin(pt, out_path, out, why)) return setup_fail(err, errlen, why);
    g_prep_ms[5] += ms_since(t0);
    std::vector<uint8_t> body;
    auto block = [&](int sec, uint32_t p, const uint8_t* bytes, size_t nbytes) {
        if (p == 0) body.assign((size_t)(parse::ptau_section_points(sec, pt.power) * parse::ptau_point_bytes(sec)), 0);
        memcpy(body.data() + parse::ptau_block_first(p) * parse::ptau_point_bytes(sec), bytes, nbytes);      // block `last` ends where the section ends
        return true;
    };
    auto after = [&](int sec) {
        const clk::time_point t = clk::now();
        const bool ok = parse::ptau_out_section(out, sec, body.data(), body.size(), why);
        if (!ok) setup_fail(err, errlen, why);
        g_prep_ms[5] += ms_since(t);
        return ok;
    };
    int rc;
    if (ctx) {
        ZKC_LOCK(ctx);
        if (hipSetDevice(ctx->device) != hipSuccess) return err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_prepare: hipSetDevice"), zkc_last_error(ctx));
        rc = walk(ctx, pt, block, after, err, errlen);
    } else rc = walk(nullptr, pt, block, after, err, errlen);
    if (rc) return rc;
    t0 = clk::now();
    if (!parse::ptau_out_commit(out, why)) return setup_fail(err, errlen, why);
    g_prep_ms[5] += ms_since(t0);
    return ZKC_OK;
}

extern "C" int zkc_ptau_check_prepared(zkc_ctx* ctx, const char* ptau_path, uint32_t* section, uint64_t* index, char* err, size_t errlen) {
    if (section) *section = 0;
    if (index) *index = 0;
    if (err && errlen) err[0] = 0;
    if (!ptau_path) return err_out(err, errlen, -ZKC_ERR_BAD_ARG, "zkc_ptau_check_prepared: bad argument");
    for (double& m : g_prep_ms) m = 0;
    const clk::time_point t0 = clk::now();
    parse::Ptau pt; std::string why;
    if (!parse::ptau_open(ptau_path, pt, why, true, parse::PTAU_MAX_PREPARE_POWER)) return -setup_fail(err, errlen, why);
    g_prep_ms[0] += ms_since(t0);
    bool differs = false, io_fail = false;
    std::vector<uint8_t> stored;
    auto block = [&](int sec, uint32_t p, const uint8_t* bytes, size_t nbytes) {
        stored.resize(nbytes);
        if (!parse::ptau_read_lagrange(pt, sec, p, stored.data(), why)) { io_fail = true; return false; }
        if (memcmp(stored.data(), bytes, nbytes) == 0) return true;
        const size_t w = parse::ptau_point_bytes(sec); size_t i = 0;
        while (memcmp(stored.data() + i * w, bytes + i * w, w) == 0) i++;
        const uint64_t at = parse::ptau_block_first(p) + i;
        if (section) *section = (uint32_t)sec;
        if (index) *index = at;
        err_out(err, errlen, 0, "ptau: section " + std::to_string(sec) + " point " + std::to_string(at) + " is not the transform of section " + std::to_string(parse::ptau_monomial_of(sec)));
        differs = true;
        return false;
    };
    auto after = [](int) { return true; };
    int rc;
    if (ctx) {
        ZKC_LOCK(ctx);
        if (hipSetDevice(ctx->device) != hipSuccess) return -err_out(err, errlen, zkc_fail(ctx, ZKC_ERR_HIP, "zkc_ptau_check_prepared: hipSetDevice"), zkc_last_error(ctx));
        rc = walk(ctx, pt, block, after, err, errlen);
    } else rc = walk(nullptr, pt, block, after, err, errlen);
    if (rc) return -rc;
    if (io_fail) return -setup_fail(err, errlen, why);
    return differs ? 0 : 1;
}

extern "C" int zkc_ptau_prepare_stats(double ms[6]) {
    if (!ms) return ZKC_ERR_BAD_ARG;
    for (int i = 0; i < 6; i++) ms[i] = g_prep_ms[i];
    return ZKC_OK;
}
