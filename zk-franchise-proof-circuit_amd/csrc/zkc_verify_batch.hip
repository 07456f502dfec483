// zkc_verify_batch.hip -- f4: the batch verifiers, everything of the verifier that takes a context: zkc_verify_batch (one verdict), zkc_verify_batch_each (a verdict per
// proof) and the test hook zkc_debug_pairing_dev.  Host code that drives the kernels of zkc_msm.hip (fold) and zkc_pairing_dev.hip (Miller loops, G2 membership); the
// single-proof verifier, the prepared keys and the error text are zkc_verify.hip's (zkc_verify_host.h).
//
// Batch verification (the step on the other side of the path, zk_census_test.go:103-124 run per vote): N proofs under one key are folded into one
// pairing-product check with random 128-bit weights rho_i:
//     prod_i e(-rho_i A_i, B_i) * e((sum rho_i) alpha, beta) * e(sum_i rho_i vk_x_i, gamma) * e(sum_i rho_i C_i, delta) == 1
// i.e. N + 3 Miller loops and ONE final exponentiation instead of 4 N and N.  The G1 work (rho_i A_i for every proof and the MSM
// sum rho_i C_i) runs on the GPU with the prover's double-and-add / group-sum kernels; so do the N Miller loops and the membership tests of the B_i from 128
// proofs on (zkc_pairing_dev.hip: one lane per pair writes its lines, a product tree per loop step, the host finishes the accumulator); smaller batches keep them on
// host threads, sixteen pairs per shared accumulator.
// A cheating prover passes with probability about 2^-128 provided the weights are unpredictable to it: `seed32` must be fresh
// randomness (NULL: std::random_device).  Each B_i is checked to lie in the order-r subgroup of the twist (G2 has a cofactor), as
// zkc_verify_bin does.
#include <cstdio>
#include <ctime>
#include <cstring>
#include <string>
#include <vector>
#include <random>
#include <thread>
#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include "zkc_verify_host.h"
#include "zkc_pairing_dev.h"

using namespace zkc;
using namespace zkc::pairing;

namespace {
struct Xoshiro { uint64_t s[4]; uint64_t next() { auto rotl = [](uint64_t x, int k) { return (x << k) | (x >> (64 - k)); };
    const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17; s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45); return r; } };
}  // namespace
// n weights of 128 bits (n x 8 words, the top four zero) from the one generator: what every batch check of the library draws its weights with (zkc_verify_host.h)
std::vector<uint32_t> zkc::verify_weights(const uint8_t* seed32, size_t n) {
    Xoshiro rng;
    if (seed32) memcpy(rng.s, seed32, 32); else { std::random_device rd; for (auto& x : rng.s) x = ((uint64_t)rd() << 32) | rd(); }
    if (!(rng.s[0] | rng.s[1] | rng.s[2] | rng.s[3])) rng.s[0] = 1;
    std::vector<uint32_t> rho(8 * n, 0);
    for (size_t i = 0; i < n; i++) {
        uint32_t* r = rho.data() + 8 * i;
        const uint64_t lo = rng.next(), hi = rng.next(); r[0] = (uint32_t)lo; r[1] = (uint32_t)(lo >> 32); r[2] = (uint32_t)hi; r[3] = (uint32_t)(hi >> 32);
    }
    return rho;
}
namespace {
// the weights of a call, all from the one generator before anything is parsed (the same whatever the number of parsing threads): rho[i] for A_i and again at rho[N + i] for C_i
std::vector<uint32_t> draw_weights(const uint8_t* seed32, int N) {
    std::vector<uint32_t> rho = verify_weights(seed32, (size_t)N);
    rho.resize(8 * 2 * (size_t)N);
    std::copy(rho.begin(), rho.begin() + 8 * (size_t)N, rho.begin() + 8 * (size_t)N);
    return rho;
}

// The members of a call as the first pass takes them: pts = the A_i, then the C_i; verdict[i] = the class of member i (ZKC_PROOF_*); rsum / xsum = the sums of rho_i and
// of rho_i x_ij over the members that are still ZKC_PROOF_VALID.
struct Batch {
    const uint8_t *pubs, *proofs; int N, nPublic; int32_t* verdict;
    std::vector<uint32_t> rho; std::vector<G1Affine> pts; std::vector<G2Affine> Bs;
    std::vector<Fr> xsum; Fr rsum;
    Batch(const uint8_t* pubs_, const uint8_t* proofs_, int N_, int nPublic_, const uint8_t* seed32, int32_t* verdict_)
        : pubs(pubs_), proofs(proofs_), N(N_), nPublic(nPublic_), verdict(verdict_), rho(draw_weights(seed32, N_)), pts(2 * (size_t)N_), Bs(N_) {}
    // member i read into pts and Bs: coordinates below q, points on their curves, public signals below r
    int32_t read(int i) {
        const uint8_t* pr = proofs + 256 * (size_t)i;
        if (!rd_g1_std(pts[i], pr) || !rd_g2_std(Bs[i], pr + 64) || !rd_g1_std(pts[N + i], pr + 192) ||
            !g1_on_curve(pts[i]) || !g1_on_curve(pts[N + i]) || !g2_on_curve(Bs[i])) return ZKC_PROOF_MALFORMED;
        for (int j = 0; j < nPublic; j++) {
            uint32_t k[8]; memcpy(k, pubs + 32 * ((size_t)i * nPublic + j), 32);
            if (!fp_std_lt_p<FrParams>(k)) return ZKC_PROOF_PUBLIC_RANGE;
        }
        return ZKC_PROOF_VALID;
    }
    // a member that is out of the batch: A, B, C at infinity, no share in the sums of weights
    void neutral(int i, int32_t why) { verdict[i] = why; pts[i] = pts[(size_t)N + i] = G1Affine::inf(); Bs[i] = G2Affine::inf(); }
    // rs += rho_i, xs[j] += rho_i x_ij when member i is still in the batch
    void add(int i, Fr* xs, Fr& rs) const {
        if (verdict[i] != ZKC_PROOF_VALID) return;
        const Fr rm = fp_from_std<FrParams>(rho.data() + 8 * (size_t)i); rs = rs + rm;
        for (int j = 0; j < nPublic; j++) { uint32_t k[8]; memcpy(k, pubs + 32 * ((size_t)i * nPublic + j), 32); xs[j] = xs[j] + rm * fp_from_std<FrParams>(k); }
    }
    // rsum and xsum over all members, on threads from a few thousand proofs on (a microsecond per proof).  parse: every member is read and classified first; one that is not
    // valid is made neutral, or with stop_at_bad ends its thread's share.  Returns whether every member read was valid.
    bool sum(bool parse, bool stop_at_bad) {
        const unsigned np = N >= 4096 ? std::max(1u, std::min({std::thread::hardware_concurrency(), N >= 32768 ? 16u : 8u})) : 1u;
        std::vector<std::vector<Fr>> xs(np, std::vector<Fr>(nPublic, Fr::zero())); std::vector<Fr> rs(np, Fr::zero()); std::vector<char> okp(np, 1);
        std::vector<std::thread> th;
        auto run = [&](unsigned t) {
            for (int i = (int)((size_t)N * t / np), hi = (int)((size_t)N * (t + 1) / np); i < hi; i++) {
                if (parse && (verdict[i] = read(i)) != ZKC_PROOF_VALID) { okp[t] = 0; if (stop_at_bad) return; neutral(i, verdict[i]); }
                add(i, xs[t].data(), rs[t]);
            }
        };
        for (unsigned t = 1; t < np; t++) th.emplace_back(run, t);
        run(0); for (auto& x : th) x.join();
        xsum.assign(nPublic, Fr::zero()); rsum = Fr::zero(); bool ok = true;
        for (unsigned t = 0; t < np; t++) { ok = ok && okp[t]; rsum = rsum + rs[t]; for (int j = 0; j < nPublic; j++) xsum[j] = xsum[j] + xs[t][j]; }
        return ok;
    }
};
// the Miller loops and membership tests on the GPU from 128 proofs on, unless $ZKC_VERIFY_BATCH_GPU says otherwise
bool miller_on_gpu(int N) { const int gpu_env = (int)sw::value<sw::ZKC_VERIFY_BATCH_GPU>(-1); return gpu_env < 0 ? N >= 128 : gpu_env != 0; }
// the verifier's work space is given back at the end of a call that grew it past 256 MB
struct Trim { zkc_ctx* c; ~Trim() { zkc_verify_ws_trim(c, (size_t)256 << 20); } };

// The device pass of every entry point, under the caller's lock and on the caller's device.  The points are folded with their weights (rho: 8 words per point) in groups:
// nsingle singletons (rho_i A_i), then the rest (the rho_i C_i) in runs of 64 -- a group is summed by ONE lane, and one lane adding all N of them was 100 ms at N = 8192;
// gout gets the group sums.  With on_gpu the Q_i go up first and *product = prod_i f_{Q_i}(-gout[i]) over the singletons, *bad != 0 when some Q_i is outside G2, tops (may be
// NULL) as miller_product_dev fills it.  `then` (may be empty) runs last, while the Q_i and the lines are still resident.  Buffers from the context's verifier work space
// (kept between calls while small: zkc_internal.h).
int fold_pass(zkc_ctx* ctx, const std::vector<G1Affine>& pts, const std::vector<uint32_t>& rho, uint32_t nsingle, const G2Affine* Qs, bool on_gpu, std::vector<G1XYZZ>& gout,
              Fq12* product, int* bad, std::vector<Fq12>* tops, const std::function<int()>& then = nullptr) {
    const uint32_t npts = (uint32_t)pts.size(), rest = npts - nsingle, ncg = (rest + 63) / 64, ngroups = nsingle + ncg;
    std::vector<uint32_t> idx(npts), gs((size_t)ngroups + 1);
    for (uint32_t i = 0; i < npts; i++) idx[i] = i;
    for (uint32_t i = 0; i < nsingle; i++) gs[i] = i;
    for (uint32_t g = 0; g <= ncg; g++) gs[(size_t)nsingle + g] = nsingle + std::min(64 * g, rest);
    gout.resize(ngroups);
    void *d_pts, *d_rho, *d_idx, *d_gs, *d_tmp, *d_gout; int e;
    if ((e = zkc_vws(ctx, zkc_ctx::VWS_PTS, pts.size() * sizeof(G1Affine), &d_pts)) || (e = zkc_vws(ctx, zkc_ctx::VWS_RHO, rho.size() * 4, &d_rho)) ||
        (e = zkc_vws(ctx, zkc_ctx::VWS_IDX, idx.size() * 4, &d_idx)) || (e = zkc_vws(ctx, zkc_ctx::VWS_GS, gs.size() * 4, &d_gs)) ||
        (e = zkc_vws(ctx, zkc_ctx::VWS_FOLD_TMP, pts.size() * sizeof(G1XYZZ), &d_tmp)) || (e = zkc_vws(ctx, zkc_ctx::VWS_FOLD_OUT, (size_t)ngroups * sizeof(G1XYZZ), &d_gout))) return e;
    if (on_gpu && (e = miller_membership_begin(ctx, Qs, nsingle))) return e;       // the Q_i go up; their membership tests (second stream) and the lines of their Miller loops (third) start beside all that follows
    struct Join { zkc_ctx* c; bool armed; ~Join() { if (armed) miller_join(c); } } join{ctx, on_gpu};      // whatever happens below, that kernel is through before the buffers can be trimmed
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_pts, pts.data(), pts.size() * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_rho, rho.data(), rho.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_gs, gs.data(), gs.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((e = fold_group_sums_g1_ws(ctx, (const G1Affine*)d_pts, (const uint32_t*)d_rho, (const uint32_t*)d_idx, npts, (const uint32_t*)d_gs, ngroups,
                                   (G1XYZZ*)d_tmp, (G1XYZZ*)d_gout, gout.data()))) return e;
    if (tops) tops->clear();
    if (on_gpu && (e = miller_product_dev(ctx, (const G1XYZZ*)d_gout, nsingle, product, bad, tops))) return e;
    return then ? then() : (int)ZKC_OK;
}
// sum_i rho_i C_i from the group sums of a verifier's pass
G1XYZZ c_sum(const std::vector<G1XYZZ>& gout, int N) { G1XYZZ s = G1XYZZ::inf(); for (size_t g = (size_t)N; g < gout.size(); g++) s = xyzz_add(s, gout[g]); return s; }

// prod_i f_{B_i}(-gout[i]) on host threads: a thread's pairs share one accumulator, sixteen at a time.  check_membership: every B_i is tested to lie in G2 first, and the
// first one that does not ends its thread and sets *bad (the product is meaningless then).
Fq12 host_miller_product(const std::vector<G2Affine>& Bs, const std::vector<G1XYZZ>& gout, int N, bool check_membership, int* bad) {
    const unsigned nthr = std::max(1u, std::min({std::thread::hardware_concurrency(), 32u, ((unsigned)N + 7) / 8}));
    std::vector<Fq12> part(nthr, one12()); std::vector<int> badt(nthr, 0);
    auto work = [&](unsigned t) {
        constexpr int CH = 16;
        const int lo = (int)((size_t)N * t / nthr), hi = (int)((size_t)N * (t + 1) / nthr);
        Fq12 f = one12(); G2Prepared prep[CH]; Pair pairs[CH];
        for (int i0 = lo; i0 < hi; i0 += CH) {
            const int n = std::min(CH, hi - i0);
            for (int k = 0; k < n; k++) {
                const int i = i0 + k;
                if (check_membership && !g2_in_subgroup(Bs[i])) { badt[t] = 1; return; }
                prep[k] = prepare_g2(Bs[i]);
                pairs[k] = {affine_neg(xyzz_to_affine_gcd(gout[i])), &prep[k]};
            }
            f = f * multi_miller(pairs, (size_t)n);
        }
        part[t] = f;
    };
    std::vector<std::thread> th; for (unsigned t = 1; t < nthr; t++) th.emplace_back(work, t);
    work(0); for (auto& x : th) x.join();
    Fq12 f = one12();
    for (unsigned t = 0; t < nthr; t++) { f = f * part[t]; if (badt[t]) *bad = 1; }
    return f;
}
// the host tail on any set of members: their Miller value, the sums of their weights and weighted signals, the sum of their rho_i C_i.  vk_x side:
// (sum rho) IC0 + sum_j (sum_i rho_i x_ij) IC_j
bool tail_ok(const VkReady& V, const Fq12& miller_value, const Fr& rs, const Fr* xs, const G1XYZZ& csum) {
    const int nPublic = V.nPublic;
    std::vector<std::array<uint32_t, 8>> ks((size_t)nPublic + 1);
    fp_to_std<FrParams>(ks[0].data(), rs);
    for (int j = 0; j < nPublic; j++) fp_to_std<FrParams>(ks[j + 1].data(), xs[j]);
    const G1XYZZ vx = g1_sum_of_products(V.ic.data(), (const uint32_t (*)[8])ks.data(), nPublic + 1);
    const G1Affine ralpha = xyzz_to_affine_gcd(g1_sum_of_products(&V.alpha, (const uint32_t (*)[8])ks.data(), 1));
    const Pair tail[3] = {{ralpha, &V.pbeta}, {xyzz_to_affine_gcd(vx), &V.pgamma}, {xyzz_to_affine_gcd(csum), &V.pdelta}};
    return is_one12(final_exp(multi_miller(tail, 3) * miller_value));
}
}  // namespace

// Returns 1 all valid / 0 at least one invalid / <0 = -ZKC_ERR_*.  The context's lock is held around the device pass only: parsing, host Miller loops and the host tail of
// concurrent calls on one context run side by side.
extern "C" int zkc_verify_batch(zkc_ctx* ctx, const uint8_t* vk, int nPublic, const uint8_t* pubs, const uint8_t* proofs, int N, const uint8_t* seed32) {
    verify_error().clear();
    if (!ctx || !vk || !pubs || !proofs || nPublic < 0 || nPublic > 4096 || N <= 0) return vfail(-ZKC_ERR_BAD_ARG, "zkc_verify_batch: bad argument");
    int code = 0;
    const std::shared_ptr<const VkReady> V = vk_ready(vk, nPublic, &code);
    if (!V) return code;
    const bool vtrace = sw::on<sw::ZKC_VERIFY_TRACE>();
    auto vnow = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    const double vt0 = vnow();
    std::vector<int32_t> cls(N);
    Batch batch(pubs, proofs, N, nPublic, seed32, cls.data());
    if (!batch.sum(true, true)) return 0;                                    // a member that fails a format check: before any device work
    const double vt1 = vnow();
    const bool on_gpu = miller_on_gpu(N);
    std::vector<G1XYZZ> gout; Fq12 product = one12(); int bad = 0;
    {
        ZKC_LOCK(ctx);
        if (hipSetDevice(ctx->device) != hipSuccess) return vfail(-ZKC_ERR_HIP, "zkc_verify_batch: hipSetDevice failed");     // never a positive code: 1 means "all valid"
        Trim trim{ctx};
        const int rc = fold_pass(ctx, batch.pts, batch.rho, (uint32_t)N, batch.Bs.data(), on_gpu, gout, &product, &bad, nullptr);
        if (rc) return vfail(-rc, std::string("zkc_verify_batch: ") + zkc_last_error(ctx));
    }
    const double vt2 = vnow();
    if (!on_gpu) product = host_miller_product(batch.Bs, gout, N, true, &bad);
    if (bad) return 0;
    const int verdict = tail_ok(*V, product, batch.rsum, batch.xsum.data(), c_sum(gout, N)) ? 1 : 0;
    if (vtrace) fprintf(stderr, "zkc_verify_batch N=%d: parse %.2f ms, device %.2f ms, host tail %.2f ms\n", N, vt1 - vt0, vt2 - vt1, vnow() - vt2);
    return verdict;
}

// ---- zkc_verify_batch_each: the batch check above with a verdict per proof (include/zkcensus_verify_each.h; DESIGN.md "A verdict per proof").  The first pass IS
// zkc_verify_batch's -- the same steps above, same kernels, same buffers, one root check -- except that a proof that fails a format check is recorded and replaced by a
// neutral member instead of ending the call.  Only a batch whose root check fails goes further: the tops of the rounds it downloaded are the
// upper levels of a product tree whose every node is the Miller value of a dyadic range of proofs, so the same check runs on any node, and the bad members are found by
// descending from the root.  All checks share the call's one weight vector. ----
namespace {
// fn(i) for i < n on at most 16 host threads
template <class Fn> void each_parallel(size_t n, Fn fn) {
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>({16, std::thread::hardware_concurrency(), n}));
    std::atomic<size_t> next{0};
    auto run = [&] { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i); };
    std::vector<std::thread> th; for (unsigned t = 1; t < nt; t++) th.emplace_back(run);
    run(); for (auto& x : th) x.join();
}
struct EachNode { uint32_t level, t; };
// one tree of the descent: the tree over the rounds (nodes on the host) or the tree of one round (nodes on the device).  Level 0 is its bottom; node t of level k has the
// children 2t and 2t + 1 of level k - 1, the second only where it exists.
struct EachTree {
    std::function<uint32_t(uint32_t)> width;                                           // nodes of a level
    std::function<void(EachNode, uint32_t&, uint32_t&)> range;                         // the proofs [lo, hi) under a node
    std::function<int(const std::vector<EachNode>&, std::vector<Fq12>&)> products;     // nlines products per node, node after node
    std::function<G1XYZZ(EachNode)> csum;
};
}  // namespace

extern "C" int zkc_verify_batch_each(zkc_ctx* ctx, const uint8_t* vk, int nPublic, const uint8_t* pubs, const uint8_t* proofs, int N, const uint8_t* seed32, int32_t* verdict) {
    verify_error().clear();
    if (!ctx || !vk || !pubs || !proofs || !verdict || nPublic < 0 || nPublic > 4096 || N <= 0) return vfail(-ZKC_ERR_BAD_ARG, "zkc_verify_batch_each: bad argument");
    int code = 0;
    const std::shared_ptr<const VkReady> V = vk_ready(vk, nPublic, &code);
    if (!V) return code;
    ZKC_LOCK(ctx);
    uint64_t* st = ctx->each_stats; st[0] = st[1] = st[2] = st[3] = 0;
    Batch batch(pubs, proofs, N, nPublic, seed32, verdict);
    batch.sum(true, false);
    const bool on_gpu = miller_on_gpu(N);
    if (!on_gpu) {                                                       // the membership tests of the host path, per proof
        std::vector<char> out(N, 0);
        each_parallel((size_t)N, [&](size_t i) { out[i] = !g2_in_subgroup(batch.Bs[i]); });
        bool any = false; for (int i = 0; i < N; i++) if (out[i]) { batch.neutral(i, ZKC_PROOF_MALFORMED); any = true; }
        if (any) batch.sum(false, false);
    }
    std::vector<G1XYZZ> gout; std::vector<Fq12> tops; Fq12 root = one12(); int gpu_bad = 0;
    if (hipSetDevice(ctx->device) != hipSuccess) return vfail(-ZKC_ERR_HIP, "zkc_verify_batch_each: hipSetDevice failed");
    Trim trim{ctx};
    auto device_pass = [&] { return fold_pass(ctx, batch.pts, batch.rho, (uint32_t)N, batch.Bs.data(), on_gpu, gout, &root, &gpu_bad, &tops); };
    auto dev_error = [&](int rc) { return vfail(-rc, std::string("zkc_verify_batch_each: ") + zkc_last_error(ctx)); };
    int rc = device_pass();
    if (rc) return dev_error(rc);
    if (on_gpu && gpu_bad) {                                             // some B_i is outside G2: which ones, and the pass again without them
        std::vector<int32_t> flag(N);
        if ((rc = miller_membership_each(ctx, (uint32_t)N, flag.data()))) return dev_error(rc);
        for (int i = 0; i < N; i++) if (flag[i]) batch.neutral(i, ZKC_PROOF_MALFORMED);
        batch.sum(false, false);
        if ((rc = device_pass())) return dev_error(rc);
        if (gpu_bad) return vfail(-ZKC_ERR_GENERIC, "zkc_verify_batch_each: the membership kernels disagree");
    }
    if (!on_gpu) root = host_miller_product(batch.Bs, gout, N, false, nullptr);      // membership was tested above
    auto result = [&] { for (int i = 0; i < N; i++) if (verdict[i] != ZKC_PROOF_VALID) return 0; return 1; };
    if (tail_ok(*V, root, batch.rsum, batch.xsum.data(), c_sum(gout, N))) return result();

    // ---- the batch holds a bad member ----
    std::vector<uint32_t> singles;                                       // proofs to verify singly, once the descent is over
    auto add_singles = [&](uint32_t lo, uint32_t hi) { for (uint32_t i = lo; i < hi; i++) if (verdict[i] == ZKC_PROOF_VALID) singles.push_back(i); };
    auto run_singles = [&] {
        each_parallel(singles.size(), [&](size_t k) { const size_t i = singles[k];
            verdict[i] = zkc_verify_bin(vk, nPublic, pubs + 32 * i * (size_t)nPublic, proofs + 256 * i) == 1 ? ZKC_PROOF_VALID : ZKC_PROOF_INVALID; });
        st[1] = singles.size();
        return result();
    };
    if (!on_gpu) { add_singles(0, (uint32_t)N); return run_singles(); }

    const uint32_t nlines = verify_n_lines(), CHUNK = verify_chunk(), nch = ((uint32_t)N + CHUNK - 1) / CHUNK;
    const uint64_t budget = std::max<uint64_t>(16, (uint64_t)N / 4);
    // prefix sums in Fr: PR[i] = sum of rho over the live members below i, PX[i][j] the same of rho x_j
    std::vector<Fr> PR((size_t)N + 1, Fr::zero()), PX(((size_t)N + 1) * nPublic, Fr::zero());
    for (int i = 0; i < N; i++) {
        PR[i + 1] = PR[i]; std::copy_n(PX.begin() + (size_t)i * nPublic, nPublic, PX.begin() + ((size_t)i + 1) * nPublic);
        batch.add(i, PX.data() + ((size_t)i + 1) * nPublic, PR[i + 1]);
    }
    std::vector<G1XYZZ> hC;                                              // the G1 sum trees of all rounds
    if ((rc = miller_sum_trees(ctx, (const G1XYZZ*)ctx->vws[zkc_ctx::VWS_FOLD_TMP] + N, (uint32_t)N, hC))) return dev_error(rc);
    const size_t per = TreeShape(std::min((uint32_t)N, CHUNK)).nodes;
    auto round_n = [&](uint32_t c) { return std::min(CHUNK, (uint32_t)N - c * CHUNK); };

    // range checks of a list of nodes of one tree: pass[i]
    auto check_nodes = [&](const EachTree& T, const std::vector<EachNode>& nodes, std::vector<char>& pass) -> int {
        std::vector<Fq12> prod;
        if (const int e = T.products(nodes, prod)) return e;
        pass.assign(nodes.size(), 0);
        each_parallel(nodes.size(), [&](size_t i) {
            uint32_t lo, hi; T.range(nodes[i], lo, hi);
            std::vector<Fr> xs(nPublic);
            for (int j = 0; j < nPublic; j++) xs[j] = PX[(size_t)hi * nPublic + j] - PX[(size_t)lo * nPublic + j];
            pass[i] = tail_ok(*V, miller_walk(prod.data() + i * nlines), PR[hi] - PR[lo], xs.data(), T.csum(nodes[i]));
        });
        st[0] += nodes.size();
        return ZKC_OK;
    };
    // from a node known to be bad down to the bottom of its tree: test the left child; if it passes the right one is bad without a test, otherwise the right one is tested
    // too.  Bad ranges of at most two proofs go to the singles, and so does everything still undecided once the call's range checks reach the budget.
    auto descend = [&](const EachTree& T, EachNode top, std::vector<EachNode>& bottoms) -> int {
        std::vector<EachNode> frontier{top};
        while (!frontier.empty()) {
            std::vector<EachNode> work, next;
            for (EachNode x : frontier)
                for (;;) {
                    uint32_t lo, hi; T.range(x, lo, hi);
                    if (hi - lo <= 2) { add_singles(lo, hi); break; }
                    if (x.level == 0) { bottoms.push_back(x); break; }
                    if (2 * x.t + 1 >= T.width(x.level - 1)) { x = {x.level - 1, 2 * x.t}; continue; }      // an only child: the same product
                    work.push_back(x); break;
                }
            auto give_up = [&](EachNode x) { uint32_t lo, hi; T.range(x, lo, hi); add_singles(lo, hi); st[3] = 1; };
            std::vector<EachNode> lefts, rights; std::vector<char> pass;
            for (size_t i = 0; i < work.size(); i++) {
                if (st[0] + lefts.size() < budget) lefts.push_back({work[i].level - 1, 2 * work[i].t}); else give_up(work[i]);
            }
            if (const int e = check_nodes(T, lefts, pass)) return e;
            for (size_t i = 0; i < lefts.size(); i++) {
                const EachNode right{lefts[i].level, lefts[i].t + 1};
                if (pass[i]) { next.push_back(right); continue; }
                next.push_back(lefts[i]);
                if (st[0] + rights.size() < budget) rights.push_back(right); else give_up(right);
            }
            if (const int e = check_nodes(T, rights, pass)) return e;
            for (size_t i = 0; i < rights.size(); i++) if (!pass[i]) next.push_back(rights[i]);
            frontier.swap(next);
        }
        return ZKC_OK;
    };

    // the tree over the rounds: level 0 holds the tops the first pass downloaded, the levels above their products (host)
    std::vector<std::vector<Fq12>> up_prod{tops}; std::vector<std::vector<G1XYZZ>> up_sum(1);
    for (uint32_t c = 0; c < nch; c++) up_sum[0].push_back(hC[per * c + TreeShape(round_n(c)).nodes - 1]);
    while (up_sum.back().size() > 1) {
        const std::vector<Fq12>& a = up_prod.back(); const std::vector<G1XYZZ>& b = up_sum.back();
        const size_t m = b.size(), h = (m + 1) / 2;
        std::vector<Fq12> p(h * nlines); std::vector<G1XYZZ> q(h);
        for (size_t t = 0; t < h; t++) {
            const bool two = 2 * t + 1 < m;
            q[t] = two ? xyzz_add(b[2 * t], b[2 * t + 1]) : b[2 * t];
            for (uint32_t s = 0; s < nlines; s++) p[t * nlines + s] = two ? a[2 * t * nlines + s] * a[(2 * t + 1) * nlines + s] : a[2 * t * nlines + s];
        }
        up_prod.push_back(std::move(p)); up_sum.push_back(std::move(q));
    }
    EachTree rounds;
    rounds.width = [&](uint32_t level) { return (uint32_t)up_sum[level].size(); };
    rounds.range = [&](EachNode x, uint32_t& lo, uint32_t& hi) { lo = (uint32_t)std::min<uint64_t>((uint64_t)N, ((uint64_t)x.t << x.level) * CHUNK); hi = (uint32_t)std::min<uint64_t>((uint64_t)N, (((uint64_t)x.t + 1) << x.level) * CHUNK); };
    rounds.products = [&](const std::vector<EachNode>& nodes, std::vector<Fq12>& out) {
        out.resize(nodes.size() * nlines);
        for (size_t i = 0; i < nodes.size(); i++) std::copy_n(up_prod[nodes[i].level].begin() + (size_t)nodes[i].t * nlines, nlines, out.begin() + i * nlines);
        return ZKC_OK;
    };
    rounds.csum = [&](EachNode x) { return up_sum[x.level][x.t]; };
    std::vector<EachNode> bad_rounds;
    if ((rc = descend(rounds, {(uint32_t)up_sum.size() - 1, 0}, bad_rounds))) return dev_error(rc);

    // each bad round: its tree again with every level kept, and the descent inside it
    for (const EachNode& br : bad_rounds) {
        const uint32_t c = br.t, base = c * CHUNK; const TreeShape sh(round_n(c));
        if (st[0] >= budget) { add_singles(base, base + sh.n); st[3] = 1; continue; }
        if ((rc = miller_round_levels(ctx, (const G1XYZZ*)ctx->vws[zkc_ctx::VWS_FOLD_OUT], (uint32_t)N, c))) return dev_error(rc);
        st[2]++;
        EachTree in;
        in.width = [&](uint32_t level) { return sh.m[level]; };
        in.range = [&](EachNode x, uint32_t& lo, uint32_t& hi) { lo = base + (uint32_t)std::min<uint64_t>(sh.n, (uint64_t)x.t << (x.level + 1)); hi = base + (uint32_t)std::min<uint64_t>(sh.n, ((uint64_t)x.t + 1) << (x.level + 1)); };
        in.products = [&](const std::vector<EachNode>& nodes, std::vector<Fq12>& out) {
            out.resize(nodes.size() * nlines);
            static_assert(sizeof(EachNode) == 2 * sizeof(uint32_t), "EachNode is (level, index)");
            return nodes.empty() ? (int)ZKC_OK : miller_nodes_fetch(ctx, sh.n, (const uint32_t (*)[2])nodes.data(), nodes.size(), out.data());
        };
        in.csum = [&](EachNode x) { return hC[per * c + sh.off[x.level] + x.t]; };
        std::vector<EachNode> pairs_left;                               // none: a pair is a range of two and goes to the singles
        if ((rc = descend(in, {(uint32_t)sh.m.size() - 1, 0}, pairs_left))) return dev_error(rc);
    }
    const int res = run_singles();
    if (sw::on<sw::ZKC_VERIFY_TRACE>()) {
        size_t ws = 0; for (size_t b : ctx->vws_sz) ws += b;
        fprintf(stderr, "zkc_verify_batch_each N=%d: %llu range checks, %llu singles, %llu rounds rebuilt, budget %s, work space %.1f MB\n", N, (unsigned long long)st[0],
                (unsigned long long)st[1], (unsigned long long)st[2], st[3] ? "hit" : "not hit", ws / 1048576.0);
    }
    return res;
}
extern "C" int zkc_verify_each_stats(zkc_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return ZKC_ERR_BAD_ARG;
    ZKC_LOCK(ctx);
    for (int i = 0; i < 4; i++) out[i] = ctx->each_stats[i];
    return ZKC_OK;
}

// ---- test hook (include/zkcensus.h): the device side of the two batch verifiers by value.  N pairs (P_i, Q_i) and weights w_i of the caller's go through fold_pass as the
// verifiers' members do -- under the context's lock, in their work-space slots, in their order: the Q_i up with their membership tests and first lines, w_i P_i as N
// singleton groups and no others, prod_i f_{Q_i}(-w_i P_i) -- then the flag per point (miller_membership_each), and, for the nodes asked for, a round's tree with every level
// kept (miller_round_levels, miller_nodes_fetch), each node walked and raised as the descent does it.  Membership is reported, not enforced. ----
extern "C" int zkc_debug_pairing_dev(zkc_ctx* ctx, const uint8_t* g1, const uint8_t* g2, const uint8_t* weights, int N, uint8_t product_out[384], uint8_t* folded_out,
                                     int32_t* member_out, int* bad_out, const uint32_t* nodes, size_t count, uint8_t* node_out) {
    if (!ctx) return ZKC_ERR_BAD_ARG;
    ZKC_LOCK(ctx);
    if (!g1 || !g2 || !product_out || !bad_out || N <= 0 || (count && node_out && !nodes)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_debug_pairing_dev: bad argument");
    if (!node_out) count = 0;
    std::vector<G1Affine> pts(N); std::vector<G2Affine> Qs(N); std::vector<uint32_t> rho(8 * (size_t)N, 0);
    for (int i = 0; i < N; i++) {
        if (!rd_g1_std(pts[i], g1 + 64 * (size_t)i) || !rd_g2_std(Qs[i], g2 + 128 * (size_t)i) || !g1_on_curve(pts[i]) || !g2_on_curve(Qs[i]))
            return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_debug_pairing_dev: pair " + std::to_string(i) + " is no pair of curve points");
        if (weights) memcpy(rho.data() + 8 * (size_t)i, weights + 32 * (size_t)i, 32); else rho[8 * (size_t)i] = 1;
    }
    const uint32_t nlines = verify_n_lines(), CHUNK = verify_chunk(), nch = ((uint32_t)N + CHUNK - 1) / CHUNK;
    auto round_n = [&](uint32_t c) { return std::min(CHUNK, (uint32_t)N - c * CHUNK); };
    for (size_t i = 0; i < count; i++) {
        const uint32_t c = nodes[3 * i], lev = nodes[3 * i + 1], t = nodes[3 * i + 2];
        if (c >= nch) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_debug_pairing_dev: no such round");
        const TreeShape sh(round_n(c));
        if (lev >= sh.m.size() || t >= sh.m[lev]) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_debug_pairing_dev: no such node");
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return zkc_fail(ctx, ZKC_ERR_HIP, "zkc_debug_pairing_dev: hipSetDevice failed");
    std::vector<G1XYZZ> gout; Fq12 product = one12(); int bad = 0;
    Trim trim{ctx};
    const int rc = fold_pass(ctx, pts, rho, (uint32_t)N, Qs.data(), true, gout, &product, &bad, nullptr, [&]() -> int {
        int e;
        if (member_out && (e = miller_membership_each(ctx, (uint32_t)N, member_out))) return e;
        // the nodes, round by round: that round's tree with every level kept, the nodes' nlines products, the walk and the final exponentiation of a range check
        std::vector<char> done(count, 0);
        for (size_t i0 = 0; i0 < count; i0++) {
            if (done[i0]) continue;
            const uint32_t c = nodes[3 * i0];
            std::vector<std::array<uint32_t, 2>> want; std::vector<size_t> at;
            for (size_t i = i0; i < count; i++) if (nodes[3 * i] == c) { want.push_back({nodes[3 * i + 1], nodes[3 * i + 2]}); at.push_back(i); done[i] = 1; }
            std::vector<Fq12> prod(want.size() * nlines);
            if ((e = miller_round_levels(ctx, (const G1XYZZ*)ctx->vws[zkc_ctx::VWS_FOLD_OUT], (uint32_t)N, c)) ||
                (e = miller_nodes_fetch(ctx, round_n(c), (const uint32_t (*)[2])want.data(), want.size(), prod.data()))) return e;
            each_parallel(want.size(), [&](size_t k) { fq12_to_std(final_exp(miller_walk(prod.data() + k * nlines)), node_out + 384 * at[k]); });
        }
        return ZKC_OK;
    });
    if (rc) return rc;
    fq12_to_std(final_exp(product), product_out);
    *bad_out = bad;
    if (folded_out)
        for (int i = 0; i < N; i++) {
            const G1Affine a = xyzz_to_affine_gcd(gout[i]); uint32_t t[8];
            fp_to_std<FqParams>(t, a.x); memcpy(folded_out + 64 * (size_t)i, t, 32); fp_to_std<FqParams>(t, a.y); memcpy(folded_out + 64 * (size_t)i + 32, t, 32);
        }
    return ZKC_OK;
}
