// zkc_top_fold.h -- the wire lists behind the folding of a census tree's TOP levels (product code): which wires stay in a proof's MSMs, which are summed into a slot of the
// key's top-of-tree table, which wires the slot index is hashed from.  Plain C++17, no HIP: zkc_fold.hip builds a key's lists through it, tests/host/top_fold_host.cc
// builds it with g++ under ASan/UBSan.
//
// Nothing of the circuit is used beyond the group ranges of zkc_abc_rows.h (fold_group_ranges: group g < n-1 of a tree = the non-control wires of level g, group n-1 = the
// old-key block).  Per proof and tree, with D = the proof's depth (every group g >= D holds template values, zkc_fold_check) and T = 0 or K:
//   groups [T, D)        stay in the proof's MSMs                         (section_lists)
//   groups [D, n-1), n-1 are behind the key's suffix sums and base        (fold_prepare)
//   groups [0, T)        are behind ONE slot of the key's table: the sums of exactly these wires as they stood in the witness that seeded the slot.  zkc_top_check has
//                        compared every one of them with the slot's copy before a proof is laid out with T = K.   (slot_wires)
// A section drops the wires whose base is the point at infinity, and C starts at wire nPub + 1.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace zkc { namespace top {

constexpr int MAX_K = 12;                        // ZKC_TOP_FOLD is clamped to this (zkc_switches.h)
constexpr int HASH_PER_GROUP = 3;                // wires per group whose low word goes into the slot index
constexpr uint16_t NO_SLOT = 0xffff;             // FinalizeArgs::tc / ts: this proof adds no slot sum for that tree
using Ranges = std::vector<std::pair<int, int>>;

struct Lists { std::vector<uint32_t> v; uint32_t offA = 0, nA = 0, offB = 0, nB = 0, offC = 0, nC = 0; };      // three ascending lists in one vector

// the wires that stay in the MSMs of a proof of depths (Dc, Ds) whose groups below (Tc, Ts) come from slots
inline Lists section_lists(size_t nWires, uint32_t nPub, const Ranges rg[2], int n, const uint8_t* infA, const uint8_t* infB, const uint8_t* infC,
                           int Tc, int Dc, int Ts, int Ds) {
    std::vector<uint8_t> folded(nWires, 0);
    auto mark = [&](const std::pair<int, int>& r) { for (int w = r.first; w < r.second && (size_t)w < nWires; w++) folded[(size_t)w] = 1; };
    for (int tree = 0; tree < 2; tree++) {
        const int D = tree == 0 ? Dc : Ds, T = tree == 0 ? Tc : Ts;
        for (int g = 0; g < T && g < n - 1; g++) mark(rg[tree][(size_t)g]);
        for (int g = D; g < n - 1; g++) mark(rg[tree][(size_t)g]);
        mark(rg[tree][(size_t)n - 1]);
    }
    Lists m;
    m.offA = 0; for (size_t w = 0; w < nWires; w++) if (!folded[w] && !infA[w]) m.v.push_back((uint32_t)w); m.nA = (uint32_t)m.v.size();
    m.offB = (uint32_t)m.v.size(); for (size_t w = 0; w < nWires; w++) if (!folded[w] && !infB[w]) m.v.push_back((uint32_t)w); m.nB = (uint32_t)m.v.size() - m.offB;
    m.offC = (uint32_t)m.v.size(); for (size_t w = (size_t)nPub + 1; w < nWires; w++) if (!folded[w] && !infC[w]) m.v.push_back((uint32_t)w); m.nC = (uint32_t)m.v.size() - m.offC;
    return m;
}

// the wires of group g of a tree that one section sums into a slot (first: the section's first wire, 0 or nPub + 1)
inline void slot_wires(const Ranges& rg, int g, const uint8_t* inf, size_t nWires, uint32_t first, std::vector<uint32_t>& out) {
    for (int w = rg[(size_t)g].first; w < rg[(size_t)g].second && (size_t)w < nWires; w++) if ((uint32_t)w >= first && !inf[(size_t)w]) out.push_back((uint32_t)w);
}

// the wires the slot index is hashed from: first, middle and last wire of every group below K.  An index only -- a proof folds its top after the full comparison alone
inline std::vector<uint32_t> hash_wires(const Ranges& rg, int K) {
    std::vector<uint32_t> h;
    for (int g = 0; g < K; g++) {
        const int a = rg[(size_t)g].first, b = rg[(size_t)g].second;
        h.push_back((uint32_t)a); h.push_back((uint32_t)(a + (b - a) / 2)); h.push_back((uint32_t)(b - 1));
    }
    return h;
}

}}  // namespace zkc::top
