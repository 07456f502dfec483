// zkc_smt_check.hip -- f1: census proofs checked in batches (arbo CheckProof, internal/helpers.go; the other half of zkc_smt_build / zkc_tree_gen_proof).  A node that receives
// votes with census proofs, or a prover that filters voters before a pass, climbs each proof from its leaf to a root: depth + 1 Poseidons per proof, all proofs independent.
//
// - Host, pass 1 (threads): per proof the field checks (key, value, root, every sibling below r), the circuit's last-slot rule, and the depth (1 + the last non-zero sibling).
//   A proof that fails a check gets its verdict here and never reaches the device.
// - The rest are counting-sorted by depth, so the lanes of a wave climb the same number of levels, and cut into chunks of bounded size.  Each chunk is compacted into one
//   pinned buffer -- keys, values, roots, an offsets array (CSR) and only the first `depth` siblings of each proof: ~21 x 32 B per proof of a 2^20 census instead of the
//   (nLevels + 1) x 32 B of the zero-padded layout -- uploaded and climbed by zkc_smt_check (zkc_witness.hip, one lane per proof).  Two buffers are used in turn: the host
//   compacts chunk k + 1 while the device copies and climbs chunk k.
// - Batches of at most 64 proofs go to zkc_smt_check_wave instead: one wave per proof, every Poseidon dealt over the lanes.
// - Verdicts come back in the sorted order and are written to the caller's order.
//
// zkc_smt_check_absence (exclusion proofs, circomlib SMTVerifier with fnc = 1) runs the same pipeline: per proof the old key and an is_old0 flag ride along, the host also
// refuses a present key (old key == key) and an old key off the key's path, the proofs are sorted by (depth, is_old0) so the lanes of a wave mostly agree on the leaf hash,
// and zkc_smt_check_absent / zkc_smt_check_absent_wave climb them.
#include "zkc_census_host.h"
#include "zkc_kernels.h"
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

using namespace zkc;

namespace {
constexpr size_t CHUNK_BYTES = (size_t)128 << 20;      // one upload buffer (two are pinned)
constexpr size_t CHUNK_PROOFS = (size_t)1 << 17;         // 2 048 waves: every lane of the chip once at the kernel's 2 waves per SIMD
constexpr size_t WAVE_MAX_DEFAULT = 64;                // batches up to this size take the wave-per-proof form; ZKC_SMT_WAVE_MAX overrides (0: never; A/B)
constexpr int32_t PENDING = -1;

// a and b differ in one of their first d bits (LSB first: the path bits)
inline bool prefix_differs(const uint8_t* a, const uint8_t* b, int d) {
    for (int i = 0; i < d / 8; i++) if (a[i] != b[i]) return true;
    return (d & 7) && ((a[d / 8] ^ b[d / 8]) & ((1u << (d & 7)) - 1));
}

// fn(lo, hi) over [0, n) on up to 16 host threads (at least 2 048 items each)
template <class F>
void parallel_for(size_t n, F fn) {
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t T = std::max<size_t>(1, std::min<size_t>({16, hw, n / 2048}));
    if (T == 1) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; t++) th.emplace_back(fn, n * t / T, n * (t + 1) / T);
    fn((size_t)0, n / T);
    for (auto& x : th) x.join();
}

// the layout of one chunk of c proofs holding S siblings in all: [keys c][old keys c][values c][is_old0 c][roots c, or 1 shared][off c + 1][siblings S], 32-byte words
// (is_old0, off: 4 bytes), each part 256-B aligned; the old keys and is_old0 are there for exclusion proofs only
struct Layout {
    size_t keys, okeys, vals, old0, roots, off, sib, total;
    Layout(size_t c, size_t S, bool per, bool absent) {
        const size_t ca = absent ? c : 0;
        keys = 0; okeys = align256(32 * c); vals = okeys + align256(32 * ca); old0 = vals + align256(32 * c); roots = old0 + align256(4 * ca);
        off = roots + align256(32 * (per ? c : 1)); sib = off + align256(4 * (c + 1)); total = sib + 32 * S;
    }
};

// one call's proofs: membership (old_keys, old0 null; values = the leaves' values) or exclusion (values = the old values)
struct Batch {
    int nLevels; size_t n; bool per;
    const uint8_t *keys, *old_keys, *values, *siblings, *roots;
    const int32_t* old0;
    bool absent() const { return old_keys != nullptr; }
};

struct Events {                                        // timing events of one call, destroyed with it
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
}  // namespace

// the pipeline both kinds share (see the top of the file): host checks, sort, chunked compaction and upload, climbs; fills status[0 .. n), n > 0
static int check_batch(zkc_ctx* ctx, const Batch& B, int32_t* status) {
    const clk::time_point t0 = clk::now();
    const int nLevels = B.nLevels; const size_t n = B.n; const bool per = B.per, absent = B.absent();
    const uint8_t *K = B.keys, *OK = B.old_keys, *V = B.values, *SB = B.siblings, *R = B.roots;
    const size_t stride = 32 * ((size_t)nLevels + 1);
    // pass 1: field checks, the last-slot rule, (exclusion) present keys and old keys off the path, depths
    std::vector<uint8_t> depth(n, 0);
    parallel_for(n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const uint8_t* s = SB + stride * i;
            int d = nLevels; while (d > 0 && is_zero(s + 32 * (d - 1))) d--;
            bool ok = below_r(K + 32 * i) && below_r(V + 32 * i) && (!absent || below_r(OK + 32 * i)) && below_r(R + (per ? 32 * i : 0)) && below_r(s + 32 * (size_t)nLevels);
            for (int l = 0; l < d && ok; l++) ok = below_r(s + 32 * l);
            int32_t st = !ok ? ZKC_SMT_NOT_BELOW_R : !is_zero(s + 32 * (size_t)nLevels) ? ZKC_SMT_LAST_SIBLING : PENDING;
            if (absent && st == PENDING && !B.old0[i])
                st = memcmp(OK + 32 * i, K + 32 * i, 32) == 0 ? ZKC_SMT_KEY_PRESENT : prefix_differs(OK + 32 * i, K + 32 * i, d) ? ZKC_SMT_OFF_PATH : PENDING;
            status[i] = st;
            depth[i] = (uint8_t)d;
        }
    });
    // the proofs that go to the device, counting-sorted by depth (exclusion: by depth, then is_old0 set first)
    const int nb = absent ? 2 * (nLevels + 1) : nLevels + 1;
    auto bucket = [&](size_t i) { return absent ? 2 * depth[i] + (B.old0[i] ? 0 : 1) : depth[i]; };
    std::vector<uint32_t> cnt(nb + 1, 0);
    for (size_t i = 0; i < n; i++) if (status[i] == PENDING) cnt[bucket(i) + 1]++;
    for (int b = 0; b < nb; b++) cnt[b + 1] += cnt[b];
    const size_t m = cnt[nb];
    std::vector<uint32_t> perm(m);
    for (size_t i = 0; i < n; i++) if (status[i] == PENDING) perm[cnt[bucket(i)]++] = (uint32_t)i;
    // chunks: [bound[k], bound[k + 1]) of perm
    std::vector<size_t> bound{0}; size_t need = 0;
    for (size_t a = 0; a < m;) {
        size_t b = a, S = 0;
        while (b < m && b - a < CHUNK_PROOFS && (b == a || Layout(b + 1 - a, S + depth[perm[b]], per, absent).total <= CHUNK_BYTES)) S += depth[perm[b++]];
        need = std::max(need, Layout(b - a, S, per, absent).total);
        bound.push_back(b); a = b;
    }
    double host_ms = ms_since(t0);
    if (m == 0) { ctx->chk_ms[0] = host_ms; return ZKC_OK; }
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->chk_sz < need) {
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < 2; k++) {
            if (ctx->chk_h[k]) { ZKC_HIP_CHECK(ctx, hipHostFree(ctx->chk_h[k])); ctx->chk_h[k] = nullptr; }
            if (ctx->chk_d[k]) { ZKC_HIP_CHECK(ctx, hipFree(ctx->chk_d[k])); ctx->chk_d[k] = nullptr; }
        }
        ctx->chk_sz = 0;
        const size_t sz = std::max(need, (size_t)1 << 20);
        for (int k = 0; k < 2; k++) {
            ZKC_HIP_CHECK(ctx, hipHostMalloc(&ctx->chk_h[k], sz));
            ZKC_HIP_CHECK(ctx, hipMalloc(&ctx->chk_d[k], sz));
            if (!ctx->chk_ev[k]) ZKC_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->chk_ev[k], hipEventDisableTiming));
        }
        ctx->chk_sz = sz;
    }
    int rc;
    if ((rc = zkc_ensure(ctx, (void**)&ctx->d_status, &ctx->status_n, m * sizeof(int32_t)))) return rc;
    const size_t wave_max = (size_t)sw::value<sw::ZKC_SMT_WAVE_MAX>(WAVE_MAX_DEFAULT);
    const bool wave = m <= wave_max;
    const size_t nchunks = bound.size() - 1;
    Events tev; tev.ev.resize(3 * nchunks, nullptr);
    for (hipEvent_t& e : tev.ev) ZKC_HIP_CHECK(ctx, hipEventCreate(&e));
    for (size_t k = 0; k < nchunks; k++) {
        const int b = (int)(k & 1);
        if (k >= 2) ZKC_HIP_CHECK(ctx, zkc_wait_event(ctx->chk_ev[b]));      // the upload of chunk k - 2 has left this buffer
        const clk::time_point t1 = clk::now();
        const size_t a = bound[k], c = bound[k + 1] - a;
        uint8_t* h = (uint8_t*)ctx->chk_h[b];
        // offsets first (one pass), then every proof's words in parallel
        size_t S = 0;
        { Layout L0(c, 0, per, absent); uint32_t* off = (uint32_t*)(h + L0.off);
          for (size_t t = 0; t < c; t++) { off[t] = (uint32_t)S; S += depth[perm[a + t]]; }
          off[c] = (uint32_t)S; }
        const Layout L(c, S, per, absent);
        const uint32_t* off = (const uint32_t*)(h + L.off);
        if (!per) memcpy(h + L.roots, R, 32);
        parallel_for(c, [&](size_t lo, size_t hi) {
            for (size_t t = lo; t < hi; t++) {
                const size_t i = perm[a + t];
                memcpy(h + L.keys + 32 * t, K + 32 * i, 32); memcpy(h + L.vals + 32 * t, V + 32 * i, 32);
                if (absent) { memcpy(h + L.okeys + 32 * t, OK + 32 * i, 32); ((uint32_t*)(h + L.old0))[t] = (uint32_t)B.old0[i]; }
                if (per) memcpy(h + L.roots + 32 * t, R + 32 * i, 32);
                memcpy(h + L.sib + 32 * (size_t)off[t], SB + stride * i, 32 * (size_t)(off[t + 1] - off[t]));
            }
        });
        host_ms += ms_since(t1);
        uint8_t* d = (uint8_t*)ctx->chk_d[b];
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k], ctx->stream));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d, h, L.total, hipMemcpyHostToDevice, ctx->stream));
        ZKC_HIP_CHECK(ctx, hipEventRecord(ctx->chk_ev[b], ctx->stream));
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k + 1], ctx->stream));
        auto P = [&](size_t o) { return (const uint32_t*)(d + o); };
        const dim3 grid((unsigned)(wave ? c : (c + 63) / 64));
        if (absent)
            hipLaunchKernelGGL(wave ? zkc_smt_check_absent_wave : zkc_smt_check_absent, grid, dim3(64), 0, ctx->stream, ctx->ptab, P(L.keys), P(L.okeys), P(L.vals),
                               P(L.old0), P(L.roots), (uint32_t)per, P(L.off), P(L.sib), (uint32_t)c, ctx->d_status + a);
        else
            hipLaunchKernelGGL(wave ? zkc_smt_check_wave : zkc_smt_check, grid, dim3(64), 0, ctx->stream, ctx->ptab, P(L.keys), P(L.vals), P(L.roots), (uint32_t)per, P(L.off),
                               P(L.sib), (uint32_t)c, ctx->d_status + a);
        ZKC_HIP_CHECK(ctx, hipGetLastError());
        ZKC_HIP_CHECK(ctx, hipEventRecord(tev.ev[3 * k + 2], ctx->stream));
    }
    std::vector<int32_t> verdict(m);
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(verdict.data(), ctx->d_status, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t j = 0; j < m; j++) status[perm[j]] = verdict[j] ? ZKC_SMT_ROOT_MISMATCH : ZKC_SMT_VALID;
    double up = 0, kern = 0;
    for (size_t k = 0; k < nchunks; k++) {
        float x = 0, y = 0;
        ZKC_HIP_CHECK(ctx, hipEventElapsedTime(&x, tev.ev[3 * k], tev.ev[3 * k + 1]));
        ZKC_HIP_CHECK(ctx, hipEventElapsedTime(&y, tev.ev[3 * k + 1], tev.ev[3 * k + 2]));
        up += x; kern += y;
    }
    ctx->chk_ms[0] = host_ms; ctx->chk_ms[1] = up; ctx->chk_ms[2] = kern;
    return ZKC_OK;
}

extern "C" int zkc_smt_check_stats(zkc_ctx* ctx, double ms[3]) {
    if (!ctx || !ms) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_stats: bad argument");
    ZKC_LOCK(ctx);
    for (int k = 0; k < 3; k++) ms[k] = ctx->chk_ms[k];
    return ZKC_OK;
}

extern "C" int zkc_smt_check_proofs(zkc_ctx* ctx, int nLevels, size_t n, const void* keys, const void* values, const void* siblings, const void* roots,
                                    int per_proof_roots, int32_t* status) {
    if (!ctx || nLevels < 1 || nLevels > 253 || (n && (!keys || !values || !siblings || !roots || !status)))
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_proofs: bad argument");
    if (n >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_proofs: more than 2^32 - 1 proofs in one call");
    ZKC_LOCK(ctx);
    ctx->chk_ms[0] = ctx->chk_ms[1] = ctx->chk_ms[2] = 0;
    if (n == 0) return ZKC_OK;
    const Batch B{nLevels, n, per_proof_roots != 0, (const uint8_t*)keys, nullptr, (const uint8_t*)values, (const uint8_t*)siblings, (const uint8_t*)roots, nullptr};
    return check_batch(ctx, B, status);
}

extern "C" int zkc_smt_check_absence(zkc_ctx* ctx, int nLevels, size_t n, const void* keys, const void* old_keys, const void* old_values, const int32_t* is_old0,
                                     const void* siblings, const void* roots, int per_proof_roots, int32_t* status) {
    if (!ctx || nLevels < 1 || nLevels > 253 || (n && (!keys || !old_keys || !old_values || !is_old0 || !siblings || !roots || !status)))
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_absence: bad argument");
    if (n >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_absence: more than 2^32 - 1 proofs in one call");
    for (size_t i = 0; i < n; i++)
        if (is_old0[i] != 0 && is_old0[i] != 1) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_check_absence: an is_old0 entry is not 0 or 1");
    ZKC_LOCK(ctx);
    ctx->chk_ms[0] = ctx->chk_ms[1] = ctx->chk_ms[2] = 0;
    if (n == 0) return ZKC_OK;
    const Batch B{nLevels, n, per_proof_roots != 0, (const uint8_t*)keys, (const uint8_t*)old_keys, (const uint8_t*)old_values, (const uint8_t*)siblings,
                  (const uint8_t*)roots, is_old0};
    return check_batch(ctx, B, status);
}
