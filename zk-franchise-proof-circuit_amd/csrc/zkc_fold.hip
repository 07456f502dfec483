// zkc_fold.hip -- the folding tables of a census key (product code): the kernels that compare a witness with the voter-independent template and with the key's top-of-tree
// table, the constants a folded proof gets back in its blinding (fold_prepare, fb4_prepare, top_prepare / top_seed) and the cached device lists of the wires and rows that
// stay in a folded pass (fold_vmap, nofold_vmap, abc_template / abc_rows).  zkc_prove.hip loads the key and lays out the passes through these.
#include "zkc_prover.h"
#include "zkc_host_util.h"
#include "zkc_kernels.h"
#include "zkc_fixedbase_dev.h"
#include "zkc_ecntt.h"
#include <ctime>
#include <cstdio>
#include <algorithm>

using namespace zkc;

// ---- fold check: for every proof and every foldable group, does the witness equal the template there? ----
// group g of a tree block = level g's non-control wires (g < n-1) ; group n-1 = the n2bOld block
extern "C" __global__ void __launch_bounds__(64)
zkc_fold_check(WitnessLayout L, const uint32_t* __restrict__ wtns, const uint32_t* __restrict__ tmpl, uint32_t* __restrict__ flags, int B, int stride) {
    const int n = L.n, g = blockIdx.x, tree = blockIdx.y, b = blockIdx.z;
    const int blk = tree == 0 ? L.off_census : L.off_sikver;
    int start, end;
    if (g < n - 1) {
        const int nctrl = (g == n - 3) + (g > 0 && g < n - 2) + 1;
        start = blk + L.lvl_off(g) + nctrl; end = blk + (g + 1 < n - 1 ? L.lvl_off(g + 1) : L.lvl_off(n - 1));
    } else { start = blk + L.off_n2bold; end = start + 253 + 127 + 133; }
    const uint4* w = reinterpret_cast<const uint4*>(wtns + (size_t)b * L.nWires * 8) + 2 * (size_t)start;
    const uint4* t = reinterpret_cast<const uint4*>(tmpl) + 2 * (size_t)start;
    uint32_t diff = 0;
    for (int i = threadIdx.x; i < 2 * (end - start); i += 64) { uint4 x = w[i], y = t[i]; diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w); }
    // [abc fold] wire 0 (the constant 1) counts with the census tree's old-key block: a witness that carries anything else there is a foreign one and unfolds its pass, so a
    // row over wire 0 and folded levels alone is the template's row (zkc_abc_rows.h)
    if (g == n - 1 && tree == 0 && threadIdx.x < 2) {
        const uint4 x = reinterpret_cast<const uint4*>(wtns + (size_t)b * L.nWires * 8)[threadIdx.x], y = reinterpret_cast<const uint4*>(tmpl)[threadIdx.x];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    const unsigned long long any = __ballot(diff != 0);
    if (threadIdx.x == 0) flags[(size_t)b * stride + (size_t)tree * n + g] = any ? 1u : 0u;      // per proof: [2][n] flags, then the two words of zkc_top_check
}

// ---- [top fold] for every proof and tree: which slot of the key's top-of-tree table do the groups 0 .. K-1 of this witness land on, and does the slot hold these very
// wires?  The slot index is a hash of a few words of those groups -- an index only: "hit" is said after EVERY wire of the groups has been compared with the slot's copy (one
// workgroup, an OR over its threads).  out = flags + 2 n of the proof's flag row: out[tree] = slot | hit << 31.  A slot is written once and its valid flag last
// (top_seed), so a slot seen valid is complete and stays what it is. ----
extern "C" __global__ void __launch_bounds__(256)
zkc_top_check(TopCheckArgs a, const uint32_t* __restrict__ wtns, uint32_t* __restrict__ flags, int stride, int off) {
    __shared__ uint32_t s_valid;
    const int tree = blockIdx.x, b = blockIdx.y;
    const uint32_t* w = wtns + (size_t)b * a.nWires * 8;
    uint32_t h = 2166136261u;
    for (int i = 0; i < top::HASH_PER_GROUP * a.K; i++) h = (h ^ w[8 * (size_t)a.hw[tree][i]]) * 16777619u;
    h ^= h >> 15;
    const uint32_t slot = h % a.nslots;
    if (threadIdx.x == 0) s_valid = __atomic_load_n(a.valid + (size_t)tree * a.nslots + slot, __ATOMIC_RELAXED);      // one read for the workgroup: a slot may be published meanwhile
    __syncthreads();
    int differs = 1;
    if (s_valid) {
        const uint4* c = reinterpret_cast<const uint4*>(a.copy[tree] + (size_t)slot * a.spanw[tree] * 8);
        uint32_t diff = 0;
        for (int g = 0; g < a.K; g++) {
            const uint4* x = reinterpret_cast<const uint4*>(w) + 2 * (size_t)a.gs[tree][g];
            const uint4* y = c + 2 * (size_t)(a.gs[tree][g] - a.span0[tree]);
            const int cnt = 2 * (int)(a.ge[tree][g] - a.gs[tree][g]);
            for (int i = threadIdx.x; i < cnt; i += 256) { const uint4 p = x[i], q = y[i]; diff |= (p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z) | (p.w ^ q.w); }
        }
        differs = __syncthreads_or(diff != 0);
    }
    if (threadIdx.x == 0) flags[(size_t)b * stride + off + tree] = slot | (differs ? 0u : 0x80000000u);
}

// ---- [r3] the folding depths of a voter straight from its inputs: 1 + the index of its last non-zero sibling, per tree.  That is where SMTLevIns puts the leaf, and every level
// from there down carries the voter-independent trace.  A call of one or two voters reads these BEFORE its witness kernel has run, so that everything behind the witness can be
// enqueued while it runs; zkc_fold_check still compares the finished witness with the template, and prove_batch_finish refuses the call if the two disagree for an accepted voter. ----
extern "C" __global__ void __launch_bounds__(64)
zkc_input_depths(const uint32_t* __restrict__ inputs, int nInputs, int n, uint32_t* __restrict__ out) {
    const int b = blockIdx.x, tree = blockIdx.y;
    const uint32_t* sib = inputs + ((size_t)b * nInputs + 12 + (size_t)tree * n) * 8;
    int d = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const uint4* q = reinterpret_cast<const uint4*>(sib + 8 * (size_t)i); const uint4 x = q[0], y = q[1];
        if (x.x | x.y | x.z | x.w | y.x | y.y | y.z | y.w) d = i + 1;
    }
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(d, m, 64); d = o > d ? o : d; }
    if (threadIdx.x == 0) out[2 * b + tree] = (uint32_t)d;
}

// ---- constant folding tables: per-level sums of template_value * base for every section, then suffix sums ----
template <class X> static void suffix_sums(std::vector<X>& suf, const X* g, int n) {   // suf[D] = sum_{k >= D} g[k], k < n-1 ; suf[n-1] = inf
    suf.assign(n, X::inf());
    for (int D = n - 2; D >= 0; D--) suf[D] = xyzz_add(suf[D + 1], g[D]);
}
template <class PT> static int fold_upload(zkc_ctx* ctx, PT** d, const std::vector<PT>& b, const std::vector<PT>* suf) {
    std::vector<PT> t; t.push_back(b[0]); t.insert(t.end(), suf[0].begin(), suf[0].end()); t.insert(t.end(), suf[1].begin(), suf[1].end());
    ZKC_HIP_CHECK(ctx, hipMalloc((void**)d, t.size() * sizeof(PT)));
    ZKC_HIP_CHECK(ctx, hipMemcpy(*d, t.data(), t.size() * sizeof(PT), hipMemcpyHostToDevice));
    return ZKC_OK;
}
// per-group sums of scalar * base for the four sections of a key: g?[g] = the sum over wires[gstart[g] .. gstart[g + 1]) of the section's list -- A, B (B1 and B2), C, the
// last with pt_shift = nPub + 1.  Sections may name one list, which then goes to the device once; an empty list sums to infinity without a launch.  pt_mod, st: as
// fold_group_sums_g1 takes them.  Synchronous; the device copies of the lists are freed on every way out
struct GroupList { std::vector<uint32_t> wires, gstart; };
static int group_sums(zkc_zkey* zk, const uint32_t* d_scalars, const GroupList* const list[3], uint32_t ng, uint32_t pt_mod, hipStream_t st, G1XYZZ* gA, G1XYZZ* gB1, G1XYZZ* gC, G2XYZZ* gB2) {
    zkc_ctx* ctx = zk->ctx; const hipStream_t up = st ? st : ctx->stream; DevBuf d_w[3], d_g[3]; int rc, at = 0;      // at: the section whose upload this one reads
    for (int sec = 0; sec < 3; sec++) {            // A, B (B1 and B2), C
        const GroupList& l = *list[sec]; const uint32_t nw = (uint32_t)l.wires.size(); G1XYZZ* g1 = sec == 0 ? gA : sec == 1 ? gB1 : gC;
        if (!nw) { std::fill(g1, g1 + ng, G1XYZZ::inf()); if (sec == 1) std::fill(gB2, gB2 + ng, G2XYZZ::inf()); continue; }
        if (sec == 0 || list[sec] != list[at]) {
            at = sec;
            if ((rc = d_w[at].alloc(ctx, l.wires.size() * 4)) || (rc = d_g[at].alloc(ctx, l.gstart.size() * 4))) return rc;
            ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_w[at].p, l.wires.data(), l.wires.size() * 4, hipMemcpyHostToDevice, up));
            ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d_g[at].p, l.gstart.data(), l.gstart.size() * 4, hipMemcpyHostToDevice, up));
            ZKC_HIP_CHECK(ctx, hipStreamSynchronize(up));
        }
        const G1Affine* tbl = zk->d_g1 + (sec == 0 ? zk->offA : sec == 1 ? zk->offB1 : zk->offC);
        if ((rc = fold_group_sums_g1(ctx, tbl, d_scalars, d_w[at].as<uint32_t>(), nw, sec == 2 ? (int32_t)zk->nPub + 1 : 0, d_g[at].as<uint32_t>(), ng, g1, pt_mod, st))) return rc;
        if (sec == 1 && (rc = fold_group_sums_g2(ctx, zk->d_g2, d_scalars, d_w[at].as<uint32_t>(), nw, 0, d_g[at].as<uint32_t>(), ng, gB2, pt_mod, st))) return rc;
    }
    return ZKC_OK;
}
int zkc::fold_prepare(zkc_zkey* zk) {
    if (zk->fold.ready) return ZKC_OK;
    zkc_ctx* ctx = zk->ctx; const WitnessLayout L = WitnessLayout::make(zk->nLevels); const int n = L.n;
    uint32_t* tmpl = zkc_get_template(ctx, zk->nLevels); if (!tmpl) return ZKC_ERR_HIP;
    GroupList l; std::vector<uint32_t>&wires = l.wires, &gstart = l.gstart;
    for (int tree = 0; tree < 2; tree++) for (auto& rg : abc::fold_group_ranges(L, tree)) { gstart.push_back((uint32_t)wires.size()); for (int w = rg.first; w < rg.second; w++) wires.push_back((uint32_t)w); }
    gstart.push_back((uint32_t)wires.size());
    const uint32_t ng = 2 * n;
    std::vector<G1XYZZ> gA(ng), gB1(ng), gC(ng); std::vector<G2XYZZ> gB2(ng);
    int rc; const GroupList* const every[3] = {&l, &l, &l};
    if ((rc = group_sums(zk, tmpl, every, ng, 0, nullptr, gA.data(), gB1.data(), gC.data(), gB2.data()))) return rc;
    auto& f = zk->fold;
    for (int t = 0; t < 2; t++) {
        suffix_sums(f.sufA[t], gA.data() + t * n, n); suffix_sums(f.sufB1[t], gB1.data() + t * n, n);
        suffix_sums(f.sufC[t], gC.data() + t * n, n); suffix_sums(f.sufB2[t], gB2.data() + t * n, n);
    }
    f.baseA = {xyzz_add(gA[n - 1], gA[2 * n - 1])}; f.baseB1 = {xyzz_add(gB1[n - 1], gB1[2 * n - 1])};
    f.baseC = {xyzz_add(gC[n - 1], gC[2 * n - 1])}; f.baseB2 = {xyzz_add(gB2[n - 1], gB2[2 * n - 1])};
    // device tables for the blinding kernel: [base | suf[0][0..n) | suf[1][0..n)]
    if ((rc = fold_upload(ctx, &f.d_foldA, f.baseA, f.sufA)) || (rc = fold_upload(ctx, &f.d_foldB1, f.baseB1, f.sufB1)) || (rc = fold_upload(ctx, &f.d_foldC, f.baseC, f.sufC)) ||
        (rc = fold_upload(ctx, &f.d_foldB2, f.baseB2, f.sufB2))) return rc;
    f.ready = true;
    return ZKC_OK;
}
// 4-bit fixed-base tables of everything the blinding of a small pass multiplies by r or s (zkc_finalize.hip): delta1, alpha1, beta1, and -- with folding -- alpha1 and beta1
// plus the base constants of A and B1 and the per-depth suffix constants of both trees.  960 points per base: 80 MB at nLevels = 160, built on the device in about a millisecond.
int zkc::fb4_prepare(zkc_zkey* zk) {
    if (!sw::on<sw::ZKC_BLIND_TREE>() || zk->d_fb4) return ZKC_OK;      // = 0 at key load: this key's small passes take the general blinding kernels (A/B, tests)
    zkc_ctx* ctx = zk->ctx;
    std::vector<G1XYZZ> bases = {G1XYZZ::from_affine(zk->delta1), G1XYZZ::from_affine(zk->alpha1), G1XYZZ::from_affine(zk->beta1)};
    const auto& f = zk->fold;
    if (f.ready) {
        bases.push_back(xyzz_add_affine(f.baseA[0], zk->alpha1)); bases.push_back(xyzz_add_affine(f.baseB1[0], zk->beta1));
        for (int t = 0; t < 2; t++) bases.insert(bases.end(), f.sufA[t].begin(), f.sufA[t].end());
        for (int t = 0; t < 2; t++) bases.insert(bases.end(), f.sufB1[t].begin(), f.sufB1[t].end());
    }
    G1XYZZ* d_bases = nullptr; int rc;
    if ((rc = dmalloc(ctx, &d_bases, bases.size()))) return rc;
    if ((rc = dmalloc(ctx, &zk->d_fb4, bases.size() * FB4_WIN * FB4_ROW)) || (rc = dmalloc(ctx, &zk->d_fb4g2, (size_t)FB4_WIN * FB4_ROW + 2))) { (void)hipFree(d_bases); return rc; }
    hipError_t e = hipMemcpyAsync(d_bases, bases.data(), bases.size() * sizeof(G1XYZZ), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) { rc = fb4_build(ctx, ctx->stream, d_bases, (int)bases.size(), zk->d_fb4, G2XYZZ::from_affine(zk->delta2), G2XYZZ::from_affine(zk->beta2),
                                             f.ready ? xyzz_add_affine(f.baseB2[0], zk->beta2) : G2XYZZ::from_affine(zk->beta2), zk->d_fb4g2); if (!rc) e = hipStreamSynchronize(ctx->stream); }
    (void)hipFree(d_bases);
    if (rc || e != hipSuccess) {
        (void)hipFree(zk->d_fb4); (void)hipFree(zk->d_fb4g2); zk->d_fb4 = nullptr; zk->d_fb4g2 = nullptr;
        return rc ? rc : zkc_fail(ctx, ZKC_ERR_HIP, std::string("fb4_prepare: ") + hipGetErrorString(e));
    }
    zk->fb4_bases = (int)bases.size();
    return ZKC_OK;
}
// a cached device list (fold_vmap, nofold_vmap, abc_rows): the words of v and one spare in an allocation of their own, copied on st and waited for.  *d is written on
// success only: the allocation is freed when the copy or the wait fails
static int list_upload(zkc_ctx* ctx, const std::vector<uint32_t>& v, hipStream_t st, uint32_t** d) {
    uint32_t* p = nullptr;
    ZKC_HIP_CHECK(ctx, hipMalloc((void**)&p, v.size() * 4 + 4));
    hipError_t e = hipMemcpyAsync(p, v.data(), v.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(p); return zkc_fail(ctx, ZKC_ERR_HIP, std::string("list_upload: ") + hipGetErrorString(e)); }
    *d = p;
    return ZKC_OK;
}
// device lists of the wires that stay in the MSMs of each section when levels >= Dc (census) / >= Ds (sik) and the n2bOld
// blocks are folded into constants; wires whose base is the point at infinity are dropped per section
// [top fold] ... and, where Tc / Ts = the key's K instead of 0, the groups below K of that tree are left out too: they come back as the sum of a slot of the key's
// top-of-tree table (zkc_top_fold.h builds the lists; cached per 4-tuple)
int zkc::fold_vmap(zkc_zkey* zk, int Tc, int Dc, int Ts, int Ds, zkc_zkey::Fold::VMap* out) {
    auto it = zk->fold.vmaps.find({Tc, Dc, Ts, Ds});
    if (it != zk->fold.vmaps.end()) { *out = it->second; return ZKC_OK; }
    zkc_ctx* ctx = zk->ctx; const WitnessLayout L = WitnessLayout::make(zk->nLevels);
    const top::Ranges rg[2] = {abc::fold_group_ranges(L, 0), abc::fold_group_ranges(L, 1)};
    const top::Lists l = top::section_lists((size_t)L.nWires, zk->nPub, rg, L.n, zk->fold.infA.data(), zk->fold.infB.data(), zk->fold.infC.data(), Tc, Dc, Ts, Ds);
    zkc_zkey::Fold::VMap m; m.offA = l.offA; m.nA = l.nA; m.offB = l.offB; m.nB = l.nB; m.offC = l.offC; m.nC = l.nC;
    if (int rc = list_upload(ctx, l.v, ctx->stream2, &m.d)) return rc;      // (the context's second stream: the first may hold a call's witness kernels)
    zk->fold.vmaps[{Tc, Dc, Ts, Ds}] = m; *out = m;
    return ZKC_OK;
}

// [top fold] the key's top-of-tree table, made empty at key load: K = $ZKC_TOP_FOLD levels (default 8; at most n - 2, a proof folds its top only when its depth exceeds K),
// 8 x 2^K slots per tree -- eight times the subtrees of one root, so that the voters of an election (one census root, one sik root) rarely share a slot.  Per slot a copy of the
// wire span [first wire of group 0, last of group K-1] as it stands in a witness (~115 KB at K = 8) and the four section sums.
int zkc::top_prepare(zkc_zkey* zk) {
    auto& tp = zk->fold.top; zkc_ctx* ctx = zk->ctx;
    if (tp.K || !zk->fold.ready) return ZKC_OK;
    const WitnessLayout L = WitnessLayout::make(zk->nLevels); const int n = L.n;
    const int K = std::min((int)sw::value<sw::ZKC_TOP_FOLD>(8), std::min(top::MAX_K, n - 2));
    if (K <= 0) return ZKC_OK;
    const top::Ranges rg[2] = {abc::fold_group_ranges(L, 0), abc::fold_group_ranges(L, 1)};
    for (int t = 0; t < 2; t++) for (int g = 0; g < K; g++) if (rg[t][g].second <= rg[t][g].first || (g && rg[t][g].first < rg[t][g - 1].second)) return ZKC_OK;      // (not the layout this relies on: off)
    // direct-mapped by a hash: with S slots for the 2^K subtrees of one root, 1 - (1 - e^(-2^K / S)) S / 2^K of them find their slot taken and never fold (21 % at S = 2 x 2^K,
    // 6 % at 8 x 2^K, the default up to K = 10: 2048 slots, 0.24 GB per tree at K = 8); at most 8192 slots, which is 2 x 2^K at K = 12 and keeps a slot index in 16 bits
    const uint32_t nslots = (uint32_t)sw::value<sw::ZKC_TEST_TOP_SLOTS>(std::max(2ll << K, std::min(8ll << K, 8192ll)));
    static_assert(2 * 8192 <= top::NO_SLOT && (2ll << top::MAX_K) <= 8192 && sw::rows[sw::ZKC_TEST_TOP_SLOTS].hi * 2 <= top::NO_SLOT && sw::rows[sw::ZKC_TOP_FOLD].hi == top::MAX_K, "zkc_switches.h: top fold");
    TopCheckArgs& a = tp.args; a.K = K; a.nslots = nslots; a.nWires = zk->nVars;
    for (int t = 0; t < 2; t++) {
        a.span0[t] = (uint32_t)rg[t][0].first; a.spanw[t] = (uint32_t)(rg[t][K - 1].second - rg[t][0].first);
        { const uint32_t padded = (a.spanw[t] + 3) & ~3u; if (a.span0[t] + padded <= zk->nVars) a.spanw[t] = padded; }      // whole 128-byte lines per slot: two slots share no cache line
        for (int g = 0; g < K; g++) { a.gs[t][g] = (uint32_t)rg[t][g].first; a.ge[t][g] = (uint32_t)rg[t][g].second; }
        const std::vector<uint32_t> hw = top::hash_wires(rg[t], K);
        for (size_t i = 0; i < hw.size(); i++) a.hw[t][i] = hw[i];
        for (int g = 0; g < K; g++) {
            tp.gA[t].push_back((uint32_t)tp.wA[t].size()); top::slot_wires(rg[t], g, zk->fold.infA.data(), zk->nVars, 0, tp.wA[t]);
            tp.gB[t].push_back((uint32_t)tp.wB[t].size()); top::slot_wires(rg[t], g, zk->fold.infB.data(), zk->nVars, 0, tp.wB[t]);
            tp.gC[t].push_back((uint32_t)tp.wC[t].size()); top::slot_wires(rg[t], g, zk->fold.infC.data(), zk->nVars, zk->nPub + 1, tp.wC[t]);
        }
        tp.gA[t].push_back((uint32_t)tp.wA[t].size()); tp.gB[t].push_back((uint32_t)tp.wB[t].size()); tp.gC[t].push_back((uint32_t)tp.wC[t].size());
    }
    int rc;
    for (int t = 0; t < 2; t++) if ((rc = dmalloc(ctx, &tp.d_copy[t], (size_t)nslots * a.spanw[t] * 8))) return rc;
    if ((rc = dmalloc(ctx, &tp.d_valid, 2 * (size_t)nslots)) || (rc = dmalloc(ctx, &tp.d_A, 2 * (size_t)nslots)) || (rc = dmalloc(ctx, &tp.d_B1, 2 * (size_t)nslots)) ||
        (rc = dmalloc(ctx, &tp.d_C, 2 * (size_t)nslots)) || (rc = dmalloc(ctx, &tp.d_B2, 2 * (size_t)nslots))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(tp.d_valid, 0, 2 * (size_t)nslots * 4, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    a.copy[0] = tp.d_copy[0]; a.copy[1] = tp.d_copy[1]; a.valid = tp.d_valid;
    tp.valid.assign(2 * (size_t)nslots, 0); tp.nslots = nslots;
    tp.K = K;
    return ZKC_OK;
}
// [top fold] writes empty slots from witnesses of a pass (w0: the pass' first witness): seed s takes groups 0 .. K-1 of tree s.tree of witness s.q into slot s.slot.  The sums
// come from the routines fold_prepare uses, every seed of the pass in one launch per section and one group per (seed, level), added up here; then the sums and the copy of
// the wires go to the device and, behind them on the same stream, the valid flags.  A slot is written once: nothing a kernel in flight may read is overwritten (a slot not
// yet valid is read by nobody).  Synchronous, under the context lock the caller (prove_batch_begin) holds: a one-time cost per subtree and key, like abc_template.
int zkc::top_seed(zkc_zkey* zk, const uint32_t* w0, const std::vector<plan::TopSeed>& seeds) {
    using plan::TopSeed;
    auto& tp = zk->fold.top; zkc_ctx* ctx = zk->ctx; const int K = tp.K; const uint32_t nv = zk->nVars, ns = (uint32_t)seeds.size(), ng = ns * (uint32_t)K;
    const hipStream_t st = ctx->stream2;
    timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
    std::vector<G1XYZZ> sum1[3]; std::vector<G2XYZZ> sum2(ns, G2XYZZ::inf());
    GroupList l[3];
    for (int sec = 0; sec < 3; sec++) {            // A, B (B1 and B2), C
        const std::vector<uint32_t>* W = sec == 0 ? tp.wA : sec == 1 ? tp.wB : tp.wC; const std::vector<uint32_t>* G = sec == 0 ? tp.gA : sec == 1 ? tp.gB : tp.gC;
        std::vector<uint32_t>&wires = l[sec].wires, &gstart = l[sec].gstart;
        for (const TopSeed& s : seeds) for (int g = 0; g < K; g++) {
            gstart.push_back((uint32_t)wires.size());
            for (uint32_t i = G[s.tree][g]; i < G[s.tree][g + 1]; i++) wires.push_back((uint32_t)s.q * nv + W[s.tree][i]);
        }
        gstart.push_back((uint32_t)wires.size());
        sum1[sec].assign(ns, G1XYZZ::inf());
    }
    std::vector<G1XYZZ> g1[3] = {std::vector<G1XYZZ>(ng), std::vector<G1XYZZ>(ng), std::vector<G1XYZZ>(ng)}; std::vector<G2XYZZ> g2(ng);
    const GroupList* const lists[3] = {&l[0], &l[1], &l[2]};
    if (int rc = group_sums(zk, w0, lists, ng, nv, st, g1[0].data(), g1[1].data(), g1[2].data(), g2.data())) return rc;
    for (int sec = 0; sec < 3; sec++) {
        if (l[sec].wires.empty()) continue;
        for (uint32_t s = 0; s < ns; s++) for (int g = 0; g < K; g++) {
            sum1[sec][s] = xyzz_add(sum1[sec][s], g1[sec][(size_t)s * K + g]);
            if (sec == 1) sum2[s] = xyzz_add(sum2[s], g2[(size_t)s * K + g]);
        }
    }
    for (uint32_t s = 0; s < ns; s++) {
        const TopSeed& sd = seeds[s]; const size_t idx = (size_t)sd.tree * tp.nslots + sd.slot, span = (size_t)tp.args.spanw[sd.tree] * 8;
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_A + idx, &sum1[0][s], sizeof(G1XYZZ), hipMemcpyHostToDevice, st));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_B1 + idx, &sum1[1][s], sizeof(G1XYZZ), hipMemcpyHostToDevice, st));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_C + idx, &sum1[2][s], sizeof(G1XYZZ), hipMemcpyHostToDevice, st));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_B2 + idx, &sum2[s], sizeof(G2XYZZ), hipMemcpyHostToDevice, st));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_copy[sd.tree] + (size_t)sd.slot * span, w0 + ((size_t)sd.q * nv + tp.args.span0[sd.tree]) * 8, span * 4, hipMemcpyDeviceToDevice, st));
    }
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(st));
    static const uint32_t one = 1;
    for (const TopSeed& sd : seeds) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(tp.d_valid + (size_t)sd.tree * tp.nslots + sd.slot, &one, 4, hipMemcpyHostToDevice, st));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (const TopSeed& sd : seeds) tp.valid[(size_t)sd.tree * tp.nslots + sd.slot] = 1;
    tp.seeded += ns;
    timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1);
    const double ms = (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-6; tp.seed_ms += ms;
    if (sw::on<sw::ZKC_TRACE_HOST>()) fprintf(stderr, "[zkc host] top fold: %u slots seeded in %.2f ms (%llu slots, %.1f ms so far)\n", ns, ms, (unsigned long long)tp.seeded, tp.seed_ms);
    return ZKC_OK;
}

// [r4] the same three lists with NOTHING folded: every wire whose base is not the point at infinity.  A third of the census circuit's wires have a zero B polynomial (27 263 of
// 82 754: B1 and B2 bases at infinity) and real R1CS are like that in general; an unfolded pass (a foreign circuit, a foreign witness, ZKC_NO_FOLD) used to carry them through
// digit extraction, bucketing and the gathers only to skip them inside the accumulation, where a skipped entry still costs its wave an addition's time.  out->d == nullptr:
// the key has no such wires, the pass indexes the sections directly.
int zkc::nofold_vmap(zkc_zkey* zk, zkc_zkey::Fold::VMap* out) {
    auto it = zk->fold.vmaps.find({-1, -1, -1, -1});
    if (it != zk->fold.vmaps.end()) { *out = it->second; return ZKC_OK; }
    zkc_ctx* ctx = zk->ctx; const uint32_t nv = zk->nVars, np = zk->nPub;
    std::vector<uint32_t> v; zkc_zkey::Fold::VMap m;
    m.offA = 0; for (uint32_t w = 0; w < nv; w++) if (!zk->fold.infA[w]) v.push_back(w); m.nA = (uint32_t)v.size();
    m.offB = (uint32_t)v.size(); for (uint32_t w = 0; w < nv; w++) if (!zk->fold.infB[w]) v.push_back(w); m.nB = (uint32_t)v.size() - m.offB;
    m.offC = (uint32_t)v.size(); for (uint32_t w = np + 1; w < nv; w++) if (!zk->fold.infC[w]) v.push_back(w); m.nC = (uint32_t)v.size() - m.offC;
    if ((size_t)m.nA + m.nB + m.nC + (size_t)nv / 50 < 3 * (size_t)nv - np - 1) {          // worth an indirection only when at least ~2 % of a section's entries drop out
        if (int rc = list_upload(ctx, v, ctx->stream, &m.d)) return rc;
    }
    zk->fold.vmaps[{-1, -1, -1, -1}] = m; *out = m;
    return ZKC_OK;
}

// [abc fold] the template's abc, once per key at its first folded call: buildABC's own kernels (matvec_launch, the form every pass takes) over the template witness, so a row
// copied from here holds the very bits the pass would have computed for it.  Ends with ctx->stream synchronised: the lanes' streams may read the block afterwards
int zkc::abc_template(zkc_zkey* zk, const uint32_t* tmpl) {
    if (zk->fold.d_abc_tmpl) return ZKC_OK;
    zkc_ctx* ctx = zk->ctx; const uint32_t n = zk->n; Fr *d_abc = nullptr, *d_wm = nullptr; int rc;
    if ((rc = dmalloc(ctx, &d_abc, 3 * (size_t)n))) return rc;
    if ((rc = dmalloc(ctx, &d_wm, 3 * (size_t)n))) { (void)hipFree(d_abc); return rc; }
    matvec_launch(zk, d_abc, d_wm, tmpl, 1, ctx->stream);
    hipError_t e = hipGetLastError(); if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_wm);
    if (e != hipSuccess) { (void)hipFree(d_abc); return zkc_fail(ctx, ZKC_ERR_HIP, std::string("abc_template: ") + hipGetErrorString(e)); }
    zk->fold.d_abc_tmpl = d_abc;
    return ZKC_OK;
}
// [abc fold] the voter rows of a pass whose proofs fold at depths up to (Dc, Ds), cached per pair like the wire lists above
int zkc::abc_rows(zkc_zkey* zk, int Dc, int Ds, zkc_zkey::Fold::AbcRows* out) {
    auto& f = zk->fold;
    auto it = f.abc_rows.find({Dc, Ds});
    if (it != f.abc_rows.end()) { *out = it->second; return ZKC_OK; }
    zkc_ctx* ctx = zk->ctx;
    const abc::VoterRows v = abc::voter_rows(f.abc_cls, f.abc_perm.data(), zk->nlong, zk->n, f.abc_rowptr.data(), f.abc_col.data(), zk->nVars, Dc, Ds);
    zkc_zkey::Fold::AbcRows m; m.nrows = (uint32_t)v.rows.size(); m.nlong = v.nlong; m.offC = m.nrows; m.nC = (uint32_t)v.crows.size(); m.offW = m.offC + m.nC; m.nW = (uint32_t)v.wires.size();
    std::vector<uint32_t> all(v.rows); all.insert(all.end(), v.crows.begin(), v.crows.end()); all.insert(all.end(), v.wires.begin(), v.wires.end());
    if (int rc = list_upload(ctx, all, ctx->stream, &m.d)) return rc;
    // [c rows] a key with the wide H table: the list an H job takes over these C rows when the pass leaves out C's transform pair
    if (zk->h_rows == 2 * zk->n) { if (int rc = list_upload(ctx, plan::h_vmap(zk->n, v.crows.data(), m.nC), ctx->stream, &m.d_hv)) { (void)hipFree(m.d); return rc; } }
    if (sw::on<sw::ZKC_TRACE_HOST>()) fprintf(stderr, "[zkc host] abc rows at depths (%d, %d): %u of %zu A/B rows listed (%u long), %u C rows, %u wires\n", Dc, Ds, m.nrows, f.abc_cls.size(), m.nlong, m.nC, m.nW);
    f.abc_rows[{Dc, Ds}] = m; *out = m;
    return ZKC_OK;
}
// [c rows] what a pass that leaves out the transform pair of C needs of its key, once per key at the first such pass (DESIGN.md "Constant folding"):
//   c_hat = pair(C_T)   the template's C through the very kernels a pass runs (ntt_pair_run), kept in Montgomery form: joinABC's third operand for every proof
//   -H'                 H'_j = sum_i M_ij H_i with M = F diag(g^i / n) F~ the matrix of the pair, so that sum_i pair(dC)_i H_i = sum_j dC_j H'_j.  M's factors are symmetric:
//                       H' = F~ diag F H over the key's H points.  With E = ecntt (inverse transform, natural order, 1 / n included): (F H)_k = n E(H)_(-k) and F~ S = n E(S), so
//                       -H' = E(S), S_k = (-n g^k) E(H)_(-k mod n): two point transforms and one product per point in between (g1_scale_each), then window 0 of the second
//                       half of the H table, pre-shifted for the H windows like the first half.
// Synchronous on ctx->stream under the context lock the caller holds.  Passes in flight on the lanes read the first half of the H table only.
int zkc::c_rows_prepare(zkc_zkey* zk) {
    auto& f = zk->fold; zkc_ctx* ctx = zk->ctx;
    if (f.c_rows_ready) return ZKC_OK;
    const uint32_t n = zk->n, logn = zk->logn; int rc;
    if (!f.d_abc_tmpl || zk->h_rows != 2 * n || logn < 12 || logn > 27) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "c_rows_prepare: the key has no template abc or no wide H table");
    timespec ts0; clock_gettime(CLOCK_MONOTONIC, &ts0);
    DevBuf chat, t, s, xy, sc, wi;
    if ((rc = chat.alloc(ctx, (size_t)n * sizeof(Fr)))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(chat.p, f.d_abc_tmpl + 2 * (size_t)n, (size_t)n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = ntt_pair_run(ctx, ctx->stream, chat.as<Fr>(), zk->d_tw_inv29, zk->d_tw_fwd29, zk->d_coset_br, (int)logn, 1))) return rc;
    // scalar of point p = -k mod n is -n g^k; entry k of the product takes point and scalar (n - k) mod n
    std::vector<uint32_t> h_sc(8 * (size_t)n), h_wi(n);
    { const Fr g = fr_root_of_unity((int)logn + 1); Fr c = Fr::zero() - fp_from_u32<FrParams>(n);
      for (uint32_t k = 0; k < n; k++) { const uint32_t p = (n - k) & (n - 1); fp_to_std<FrParams>(h_sc.data() + 8 * (size_t)p, c); h_wi[k] = p; c = c * g; } }
    G1Affine* const H0 = zk->d_g1 + zk->offH;
    if ((rc = t.alloc(ctx, (size_t)n * sizeof(G1Affine))) || (rc = s.alloc(ctx, (size_t)n * sizeof(G1Affine))) || (rc = xy.alloc(ctx, (size_t)n * sizeof(G1XYZZ))) ||
        (rc = sc.alloc(ctx, h_sc.size() * 4)) || (rc = wi.alloc(ctx, h_wi.size() * 4))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(sc.p, h_sc.data(), h_sc.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(wi.p, h_wi.data(), h_wi.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ecntt<Fq>(ctx, H0, logn, zk->d_tw_inv, logn, t.p, true, nullptr))) return rc;                              // E(H); synchronises
    if ((rc = g1_scale_each(ctx, t.as<G1Affine>(), sc.as<uint32_t>(), wi.as<uint32_t>(), n, xy.as<G1XYZZ>()))) return rc;
    if ((rc = fixed_affine<Fq>(ctx, xy.as<G1XYZZ>(), n, s.p, true))) return rc;                                          // S; synchronises
    if ((rc = ecntt<Fq>(ctx, s.p, logn, zk->d_tw_inv, logn, H0 + n, true, nullptr))) return rc;                          // -H' into window 0 of the second half
    if ((rc = msm_precompute_g1(ctx, n, H0 + n, zk->c_h, 2 * (size_t)n))) return rc;
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    f.d_c_hat = (Fr*)chat.release(); f.c_rows_ready = true;
    if (sw::on<sw::ZKC_TRACE_HOST>()) { timespec ts1; clock_gettime(CLOCK_MONOTONIC, &ts1);
        fprintf(stderr, "[zkc host] c rows: transformed template C and -H' (%u points, %d windows) in %.1f ms\n", n, msm_nw(zk->c_h), (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-6); }
    return ZKC_OK;
}
// everything above that lives as long as the key (zkc_zkey_free; d_fb4 / d_fb4g2 are in the key's own list there)
void zkc::fold_free(zkc_zkey* zk) {
    if (zk->fold.d_c_hat) (void)hipFree(zk->fold.d_c_hat);
    for (auto& kv : zk->fold.vmaps) if (kv.second.d) (void)hipFree(kv.second.d);
    for (auto& kv : zk->fold.abc_rows) { if (kv.second.d) (void)hipFree(kv.second.d); if (kv.second.d_hv) (void)hipFree(kv.second.d_hv); }
    if (zk->fold.d_abc_tmpl) (void)hipFree(zk->fold.d_abc_tmpl);
    { auto& tp = zk->fold.top; for (void* q : {(void*)tp.d_copy[0], (void*)tp.d_copy[1], (void*)tp.d_valid, (void*)tp.d_A, (void*)tp.d_B1, (void*)tp.d_C, (void*)tp.d_B2}) if (q) (void)hipFree(q); }
    for (void* q : {(void*)zk->fold.d_foldA, (void*)zk->fold.d_foldB1, (void*)zk->fold.d_foldC, (void*)zk->fold.d_foldB2}) if (q) (void)hipFree(q);
}
