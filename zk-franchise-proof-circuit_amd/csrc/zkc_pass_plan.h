// zkc_pass_plan.h -- the host decisions of a batch call and of each of its pipeline passes (product code): how a call splits into passes, how far a proof folds, which slot
// of the top-of-tree table it takes or seeds, the windows, tables and job counts of a pass, and on which stream each stage goes.  Every one of them is arithmetic on a few
// integers and a row of flags.  Plain C++17, no HIP, and nothing here touches a stream or reads the environment: prove_batch_begin / prove_batch_finish (zkc_prove.hip)
// call these functions and keep no copy of the logic, tests/host/pass_plan_host.cc builds them with g++ under ASan/UBSan.  Device pointers are opaque here.
#pragma once
#include "zkc_top_fold.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace zkc {
// [r3] the G2 section of a pass of one or two proofs: 8-bit windows -> 32 additions per scalar into 128 buckets.  A lone proof's B2 MSM is ~5 000 scalars and its latency is the
// bucket REDUCTION (2048 buckets: ~30 of the ~55 G2 additions in a row); with 128 buckets one wave reduces the job.  Costs a second pre-shifted G2 table (0.6 GB at nLevels 160).
constexpr int MSM_C_G2_LONE = 8;
constexpr int msm_nw(int c) { return (254 + c) / c; }          // 17 -> 15 windows (255 bits), 12 -> 22 windows (264 bits)
constexpr int msm_half(int c) { return 1 << (c - 1); }         // buckets per job

namespace plan {

// ---- the call: passes of equal size (1024 -> 10 x 94 + 84, not 10 x 96 + 64): the last pass' fixed-latency tail is not spent on a stub ----
struct CallSplit { int npasses, per_pass; };
inline CallSplit call_split(int B, int max_inflight) {
    const int npasses = (B + max_inflight - 1) / max_inflight;
    return {npasses, (B + npasses - 1) / npasses};
}

// ---- one tree's row of fold flags (zkc_fold_check: f[g] = group g of the witness differs from the template) -> the proof's depth in that tree: every group from D on is the
// template's.  FOREIGN: the old-key block (group n-1) differs -- not one of our witnesses, its pass is not folded ----
constexpr int FOREIGN = -1;
inline int row_depth(const uint32_t* f, int n) {
    if (f[n - 1]) return FOREIGN;
    int D = 0; for (int g = 0; g < n - 1; g++) if (f[g]) D = g + 1;
    return D;
}
// a call laid out from its inputs' depths before its witnesses existed: the fold check of the finished witnesses has to agree -- every accepted voter (status[q] == ok; a
// rejected voter's proof is discarded whatever it is) neither foreign nor deeper than the depth it was laid out with.  flags: per voter `stride` words, [2][n] flags first;
// early_depth: (census, sik) per voter.  Returns the first voter that disagrees, or -1
inline int early_disagrees(const uint32_t* status, uint32_t ok, const uint32_t* flags, size_t stride, int n, const uint8_t* early_depth, int voters) {
    for (int q = 0; q < voters; q++) {
        if (status[q] != ok) continue;
        for (int t = 0; t < 2; t++) { const int D = row_depth(flags + (size_t)q * stride + (size_t)t * n, n); if (D == FOREIGN || D > (int)early_depth[2 * q + t]) return q; }
    }
    return -1;
}

// ---- [top fold] a proof whose groups 0 .. K-1 of a tree are the very wires a slot of the key's table holds (zkc_top_check: hit) and whose depth in that tree exceeds K leaves
// them out of its MSMs; the blinding kernel adds the slot's sums (FinalizeArgs::tc / ts).  Not in a pass laid out early (no flags yet), not in a pass of one or two proofs
// (the tree form of the blinding has no fixed-base rows for these sums).  A proof that misses is proved as before, and if its slot is empty its witness fills it (top_seed):
// one seed per (tree, slot), however many proofs of the pass miss on it.
// dc / ds: the depths; words: the first proof's two zkc_top_check words (slot | hit << 31 per tree), `stride` words from proof to proof; K = 0: the key (or this pass) folds no
// top; valid: the host mirror of the table's valid flags, [2][nslots].  tc / ts [nb]: index into the table's [2][nslots] sums, or top::NO_SLOT ----
struct TopSeed { int q, tree; uint32_t slot; };
inline void top_fold(const uint8_t* dc, const uint8_t* ds, const uint32_t* words, size_t stride, int K, uint32_t nslots, const uint8_t* valid, bool early, int nb,
                     uint16_t* tc, uint16_t* ts, std::vector<TopSeed>& seeds) {
    for (int q = 0; q < nb; q++) tc[q] = ts[q] = top::NO_SLOT;
    seeds.clear();
    if (K <= 0 || early || nb <= 2) return;
    for (int q = 0; q < nb; q++) for (int t = 0; t < 2; t++) {
        if ((int)(t == 0 ? dc : ds)[q] <= K) continue;
        const uint32_t word = words[(size_t)q * stride + t], slot = word & 0x7fffffffu; const size_t idx = (size_t)t * nslots + slot;
        if (slot >= nslots) continue;
        if (word >> 31) { (t == 0 ? tc : ts)[q] = (uint16_t)idx; continue; }
        bool listed = valid[idx] != 0; for (const TopSeed& s : seeds) listed = listed || (s.tree == t && s.slot == slot);
        if (!listed) seeds.push_back({q, t, slot});
    }
}

// ---- the shape of a pass ----
struct KeyShape {                                    // what a pass reads of its key
    int c_sec, c_h, c_deep;                          // window bits: witness sections, H, the second section tables (0: not built)
    uint32_t nv, np, n;                              // wires, public signals, domain size
    uint32_t offA, offB1, offC, offA_deep, offB1_deep, offC_deep;      // the sections' tables inside the G1 point array
    bool lone_table, fb4;                            // the key has the 8-bit-window G2 table / the 4-bit fixed-base tables of the small-pass blinding
};
struct LaneCaps { size_t w1_entries, w1_buckets; int w1_jobs; size_t w2_entries; };      // the lane's G1 and G2 work space (MsmWork::max_*)
// the values of the switches a pass reads (zkc_switches.h; numbers: 0 = not given)
struct Switches {
    uint32_t vw_big = 0, vw_small = 0, vw_g2 = 0; size_t deep_wires = 16000;                         // ZKC_VW_BIG, ZKC_VW_SMALL, ZKC_VW_G2, ZKC_DEEP_WIRES
    bool matvec_inline = false, g2_acc_hold = false, g2_acc_early = false, reduce_stream = false;   // ZKC_MATVEC_INLINE, ZKC_G2_ACC_HOLD, ZKC_G2_ACC_EARLY, ZKC_REDUCE_STREAM
    bool serial_streams = false;                                                                    // ZKC_SERIAL_STREAMS, as the key was loaded
    int lane_streams = 0;                                                                           // ZKC_LANE_STREAMS, as the key was loaded (lane_roles)
};
struct PassShape {
    uint32_t vws, vwb, vw_g2;                        // buckets per reduction wave: witness sections, H, the G2 jobs
    bool deep; int cw;                               // the sections take the key's second tables; window bits of this pass' witness sections
    uint32_t oA, oB1, oC;                            // their tables
    int c2;                                          // window bits of the G2 jobs
    bool tree; int per;                              // the pass carries its blinding's two variable-base products as MSM jobs: 5 results per proof instead of 3
};
// lists: per proof the sizes of its wire lists (any struct with nA, nB, nC: zkc_zkey::Fold::VMap), or nullptr: the jobs run over whole sections
template <class Lists> inline PassShape pass_shape(const KeyShape& k, int nb, const Lists* lists, const LaneCaps& cap, const Switches& s) {
    const uint32_t nv = k.nv, nc = nv - k.np - 1;
    PassShape p;
    // buckets per wave of the bucket reduction ("virtual window"): a lane walks vw / 64 buckets with two full additions each, then the 64 lanes pay ~17 more for the scan and
    // the tree -- fixed cost per wave, so a full pass wants large windows (fewer additions in all), a small one small windows (fewer in a row).  [r4] re-measured on the
    // round-4 pipeline, one box, (H, sections): (1024, 256) 3195 / 3205 / 3212 / 3214 proofs/s -- round 1's optimum, the default until now -- (2048, 512) 3235 / 3238,
    // (4096, 1024) 3229, (4096, 2048) 3248 / 3261 / 3264 / 3268 (+1.8 %), (8192, 1024) 3100.  Passes of fewer than 32 proofs keep the smaller windows (latency).
    p.vws = nb <= 4 ? 64u : s.vw_small ? s.vw_small : nb < 32 ? 256u : 2048u; p.vwb = nb <= 4 ? 256u : s.vw_big ? s.vw_big : nb < 32 ? 1024u : 4096u;
    // the G2 section of one or two proofs takes the 8-bit-window table: 128 buckets per job, reduced by one wave (vw = 128), if the G2 work space holds 32 entries per scalar
    size_t lone_entries = 0; for (int q = 0; q < nb; q++) lone_entries += (size_t)msm_nw(MSM_C_G2_LONE) * (lists ? lists[q].nB : nv);
    // [r4] deep pass: the voters of this pass keep, on average, more than ZKC_DEEP_WIRES (16 000) wires per section in their MSMs (leaves far down the trees, or witnesses that
    // do not fold): the sections take the key's second tables (c_deep bits: msm_c_for).  Per section of W full-width scalars: 22 W + 2048 x 4.2 additions at 12 bits,
    // 17 W + 16384 x 4.2 at 15: break-even at W = 12 k by that count, at 14 k measured (profiles/r04_deep_pass_threshold.json: voters 30 levels down; +1.4 % at 40 levels,
    // +16 % at 160); a census of 2^13 .. 2^20 voters keeps 6-9 k and stays at 12 bits (-3 % if forced over the second tables).
    size_t live_wires = 0; for (int q = 0; q < nb; q++) live_wires += lists ? (size_t)lists[q].nA + lists[q].nB + lists[q].nC : 2 * (size_t)nv + nc;
    p.deep = k.c_deep != 0 && nb > 2 && live_wires >= 3 * s.deep_wires * (size_t)nb;
    p.cw = p.deep ? k.c_deep : k.c_sec;
    p.oA = p.deep ? k.offA_deep : k.offA; p.oB1 = p.deep ? k.offB1_deep : k.offB1; p.oC = p.deep ? k.offC_deep : k.offC;
    p.c2 = (nb <= 2 && k.lone_table && lone_entries <= cap.w2_entries) ? MSM_C_G2_LONE : p.cw;
    p.vw_g2 = p.c2 == MSM_C_G2_LONE ? 128u : (s.vw_g2 && nb >= 32) ? s.vw_g2 : p.vws;      // ZKC_VW_G2: A/B, the G2 jobs' window apart from the G1 sections'
    // [r3] a pass of one or two proofs carries its blinding's two variable-base products as two more MSM jobs each -- sum (s w_i) A_i and sum (r w_i) B1_i over the
    // wires that stay in the proof's MSMs -- so that the blinding kernel is left with fixed-base products only (zkc_finalize.hip)
    // (the lanes' work space is sized for max(4, passes of this key) proofs of 3 + 1 jobs each: two proofs of 5 + 1 fit unless ZKC_INFLIGHT made the passes smaller than that)
    size_t tree_entries = 0; for (int q = 0; q < nb; q++) tree_entries += (size_t)msm_nw(k.c_h) * k.n + (size_t)msm_nw(k.c_sec) * (lists ? 2 * (size_t)lists[q].nA + 2 * (size_t)lists[q].nB + lists[q].nC : 4 * (size_t)nv + nc);
    p.tree = k.fb4 && nb <= 2 && 6 * nb <= cap.w1_jobs && tree_entries <= cap.w1_entries && (size_t)nb * (5 * msm_half(k.c_sec) + msm_half(k.c_h)) <= cap.w1_buckets;
    p.per = p.tree ? 5 : 3;
    return p;
}

// ---- one MSM section of one proof: what becomes the MsmJob fields.  A proof with lists takes its scalars and points through them; one without runs over the whole
// sections, C's scalars starting at wire np + 1 (so no shift) ----
struct SectionView { const uint32_t* scalars; const uint32_t* vmap; uint32_t count, tbl_off, tbl_count; int32_t pt_shift; };
struct ProofViews { SectionView A, B1, C; };
// w: the proof's witness; vm: its lists (any struct with d, offA, nA, offB, nB, offC, nC) or nullptr
template <class Lists> inline ProofViews proof_views(const KeyShape& k, const PassShape& p, const uint32_t* w, const Lists* vm) {
    const uint32_t nv = k.nv, np = k.np, nc = nv - np - 1;
    if (vm) return {{w, vm->d + vm->offA, vm->nA, p.oA, nv, 0}, {w, vm->d + vm->offB, vm->nB, p.oB1, nv, 0}, {w, vm->d + vm->offC, vm->nC, p.oC, nc, (int32_t)np + 1}};
    return {{w, nullptr, nv, p.oA, nv, 0}, {w, nullptr, nv, p.oB1, nv, 0}, {w + 8ull * (np + 1), nullptr, nc, p.oC, nc, 0}};
}

// ---- [c rows] the transform pair of C left out of a folded pass (DESIGN.md "Constant folding", ZKC_C_ROWS) ----
// C on the domain is the key's template except on the constraints the pass lists (zkc_abc_rows.h: VoterRows::crows), and the pair is linear: the pass joins A'B' with the
// template's transformed C, kept per key, and the listed differences enter the H job as k more (scalar, base) pairs against the second half of the H table (-H').  That
// trades a third of the pass' transform work for k nw_H additions per proof, so it pays while k nw_H <= beta n log2 n.  Everything else keeps the pair of three vectors:
// a pass that is not folded or whose buildABC is not (the prefetched one of a one-lane call, ZKC_ABC_FOLD=0), a pass laid out early, the tree-shaped pass of one or two
// proofs, a key without the wide H table, a lane whose work space does not hold the further entries or the second half of the H scalars.
// The answer reads the pass' depths (through k) and its lane, never the state of the top-of-tree table: section_entries is counted over the lists that fold no top.
struct CRowsIn {
    int mode;                        // ZKC_C_ROWS as the key was loaded: 0 never, 2 wherever legal, else the rule
    uint32_t beta_milli;             // beta in thousandths
    bool wide_table;                 // the key's H table has 2 n rows per window
    bool abc_folded, early;          // buildABC of this pass runs over the voter rows only; the pass was laid out before its witnesses existed
    uint32_t k;                      // constraints whose C the pass forms
    int logn;
    size_t section_entries;          // (scalar, window) entries of the pass' A, B1 and C jobs, at most: over the lists that fold no top, at the key's 12-bit windows
    size_t cap_p_words;              // words of the lane's H-scalar buffer
};
inline bool c_rows_rule(uint32_t k, int nw_h, uint32_t n, int logn, uint32_t beta_milli) { return (uint64_t)k * (uint64_t)nw_h * 1000u <= (uint64_t)beta_milli * n * (uint64_t)logn; }
// what costs nothing to ask: a pass that fails this never takes the path, and its caller need not count section_entries for it
inline bool c_rows_candidate(const KeyShape& key, const PassShape& p, int nb, const CRowsIn& in) {
    if (in.mode == 0 || !in.wide_table || !in.abc_folded || in.early || p.tree || nb <= 2) return false;
    return in.mode == 2 || c_rows_rule(in.k, msm_nw(key.c_h), key.n, in.logn, in.beta_milli);
}
inline bool c_rows(const KeyShape& key, const PassShape& p, int nb, const LaneCaps& cap, const CRowsIn& in) {
    if (!c_rows_candidate(key, p, nb, in)) return false;
    const int nw_h = msm_nw(key.c_h);
    if (in.section_entries + (size_t)nb * nw_h * ((size_t)key.n + in.k) > cap.w1_entries) return false;
    if ((size_t)nb * 16 * key.n > in.cap_p_words) return false;
    return true;
}
// the H job's list on that path: the identity over [0, n), then n + j for the listed constraints j (ascending): scalar and table row of entry i are both h_vmap[i]
inline std::vector<uint32_t> h_vmap(uint32_t n, const uint32_t* crows, uint32_t k) {
    std::vector<uint32_t> v((size_t)n + k);
    for (uint32_t i = 0; i < n; i++) v[i] = i;
    for (uint32_t i = 0; i < k; i++) v[(size_t)n + i] = n + crows[i];
    return v;
}

// ---- on which stream, and behind what, the stages of a pass go ----
struct StreamOrder {
    bool mv_prefetch;          // buildABC of the next pass is issued on the blinding stream beside this pass' accumulation (a call that stays on one lane)
    bool mv_done;              // ... so this pass' buildABC has been run already
    bool g2_acc_with_sort;     // the G2 accumulation is held until the G1 stream leaves its transforms
    bool red_split;            // the G1 bucket reduction runs on the lane's reduction stream
    bool blind_on_st;          // blinding and copy go on the G1 stream itself instead of the blinding stream
};
// one_lane: every pass of the call runs on one lane; pass: index of this pass in its call; lane0 >= 0: the caller named the lane (the proving service)
inline StreamOrder stream_order(int nb, bool one_lane, int pass, int npasses, int lane0, bool tree, const Switches& s) {
    StreamOrder o;
    // [r2] buildABC is gather-bound and needs only the witness: the one of pass p+1 is issued on the blinding stream as soon as the accumulation
    // of pass p starts (VALU-bound, 15 ms) and is through long before the G1 stream gets there; only the first pass runs it in line
    o.mv_prefetch = !s.matvec_inline && one_lane;
    o.mv_done = o.mv_prefetch && pass > 0;
    // [r2] its bucketing starts with the pass, but its accumulation (VALU-bound, 3.3 ms alone) is held until the G1 stream leaves the NTT: it then
    // runs beside the G1 bucketing and segment kernels, which wait on memory and LDS atomics, instead of beside the NTT, which is VALU-bound too
    // [r4] ... which was right for round 2's pipeline and is not for this one: with the larger reduction windows the G2 side's tail is longer (one wave walks a job's 2048
    // buckets: ~64 G2 additions in a row), and holding its accumulation back makes the blinding -- and with it the result slot the pass after next needs -- wait for it.
    // Alternating on one box: 3160 / 3143 / 3160 / 3150 / 3151 proofs/s held back, 3205 / 3198 / 3206 / 3169 / 3206 started with the pass: +1.4 %.  ZKC_G2_ACC_HOLD=1: the old order.
    // (Two pipeline lanes, -4 % in round 2, are +1.4 % now too -- 3202 / 3206 / 3197 / 3202 / 3201 -- but not on top of this (3107 / 3115 with both) and for twice the work space.)
    // Passes of fewer than 32 proofs keep the hold: a lone proof's G2 kernels (1024 waves of 400 registers) slowed buildABC and the first transform kernel threefold when they were
    // not held (round 3), and the twelve-proof passes of a 2^20-domain key run 140 proofs/s held against 136 early (their bucketing phase is 9 ms long: room for the G2 accumulation).
    // [r5] ... and with the passes of a call rotating over four lanes the hold is right again for full passes: the G2 accumulation of lane k then lands beside lane k's own
    // bucketing instead of beside another lane's transforms (alternating on one box: 3380 / 3386 proofs/s held, 3363 / 3363 started with the pass: +0.6 %)
    // ... which is what a rotating call gets without an event now that its G2 MSM is enqueued on the lane's st behind the transforms (lane_roles): there the flag is read only
    // under ZKC_LANE_STREAMS=2 / 3, where the G2 side has its own stream again
    o.g2_acc_with_sort = s.g2_acc_hold || ((nb < 32 || !one_lane) && !s.g2_acc_early);
    // (measured, alternating on one box: 3102 / 3089 / 3083 proofs/s with the reduction on its own stream, 3074 / 3087 / 3097 without -- nothing: the pass is bound by the
    // sum of its kernels' VALU work, and where the reduction's waves run does not change that sum.  Off unless ZKC_REDUCE_STREAM=1.)
    o.red_split = s.reduce_stream && !s.serial_streams && nb >= 32;
    // a call that is one small pass: its blinding and its copy go on the G1 stream itself -- nothing follows that they could overlap with, and a hop to the blinding stream is
    // ~25 us of a 3.2 ms proof
    // [r5] ... and so does every one-pass call that stays on its lane (the proving service): its blinding can only start when both MSM sides are through and nothing of the
    // call follows it, so a stream of its own buys nothing and costs a hardware queue (a service of four lanes keeps 8 streams busy instead of 12)
    o.blind_on_st = (tree || lane0 >= 0) && npasses == 1;
    return o;
}

// ---- which of a lane's roles share a stream in this pass ----
// A lane has up to four streams (zkc_lane): st, st2, fin, red.  Each role of a pass names the one that carries it; two roles with the same answer need no event between them,
// and prove_batch_begin enqueues none.
enum LaneStream { ON_ST = 0, ON_ST2 = 1, ON_FIN = 2, ON_RED = 3 };
struct LaneRoles {
    int g1;                    // buildABC, transforms, G1 MSM: always ON_ST
    int g2;                    // G2 MSM (and piB of a small pass)
    int blind;                 // blinding and the copy of the proofs
    int red;                   // G1 bucket reduction
    int streams;               // how many streams of the lane the pass touches
};
// lanes: how many lanes the passes of this call rotate over (1: the call stays on one lane -- a key with one lane, a call of one pass, a lane named by the caller).
// The second and third stream of a lane overlap a pass with ITSELF: the G2 side beside the G1 side, the blinding beside the next pass.  That was the single-lane pipeline of
// rounds 2-4 and it still is the plan of a call that stays on one lane, whatever the switch says.  A call whose passes rotate over several lanes finds the same overlap BETWEEN
// lanes -- a lane works ~20 ms of the ~75 ms between two of its passes -- and every further stream is a further share of the process' hardware queues, every hop between two
// streams of a lane a barrier packet that another lane's stream may have to queue behind (zkc_api.hip, "Hardware queues").  So such a call runs every stage of a pass on the
// lane's st, in the order they are enqueued today: transforms, G2 MSM, G1 MSM, blinding, copy.  ZKC_LANE_STREAMS: 1 that plan, 2 the G2 side on st2 again, 3 the plan of
// rounds 2-5 (st, st2, fin) for a host that gives the process a hardware queue per stream.  Measured on four queues: DESIGN.md section 3, "Lanes, hardware queues".
// The reduction stream (ZKC_REDUCE_STREAM=1, stream_order) is an A/B switch of its own and stays one under every plan.
inline LaneRoles lane_roles(int nb, bool one_lane, int pass, int npasses, int lane0, bool tree, int lanes, const Switches& s) {
    const StreamOrder o = stream_order(nb, one_lane, pass, npasses, lane0, tree, s);
    const bool rotates = !one_lane && lanes > 1;
    const int want = !rotates ? 3 : (s.lane_streams >= 1 && s.lane_streams <= 3) ? s.lane_streams : 1;
    LaneRoles r;
    r.g1 = ON_ST;
    r.g2 = want >= 2 ? ON_ST2 : ON_ST;
    r.blind = (o.blind_on_st || want <= 2) ? ON_ST : ON_FIN;
    r.red = o.red_split ? ON_RED : ON_ST;
    r.streams = 1 + (r.g2 != ON_ST) + (r.blind != ON_ST) + (r.red != ON_ST);
    return r;
}

}}  // namespace zkc::plan
