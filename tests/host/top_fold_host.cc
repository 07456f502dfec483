// top_fold_host.cc -- the wire lists of the top-of-tree folding (csrc/zkc_top_fold.h) as a stand-alone host program, built by tests/test_top_fold_cpu.py with g++ under
// AddressSanitizer + UBSan.
//   top_fold_host IN OUT
// IN  (u32 little endian): n, off_census, off_sikver, off_n2bold, lvl_off[0 .. n), nWires, nPub, then per wire three words: its A, B, C base is the point at infinity,
//     then nK and the nK values of K.  The layout numbers stand in for WitnessLayout (zkc_device.h), which needs HIP.
// For every K and every (Tc, Dc, Ts, Ds) with D in 0 .. n-1 and T = 0, or T = K where D > K, the program checks that per section
//     the wires of section_lists  +  the wires slot_wires sums into a slot (tree by tree, where T = K)  +  the wires behind the suffix sums and the base (groups >= D, old-key block)
// hold every wire of the section whose base is not at infinity exactly once (C: from wire nPub + 1), and nothing else.
// OUT (u32): per K and tuple, in loop order: nA, nB, nC.
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_abc_rows.h"
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_top_fold.h"
#include <cstdio>
#include <cstdlib>

using namespace zkc;

struct Layout {
    int n = 0, off_census = 0, off_sikver = 0, off_n2bold = 0; std::vector<int> lvl;
    int lvl_off(int i) const { return lvl.at((size_t)i); }
};
static int fail(const char* what) { printf("top fold: FAILED %s\n", what); return 1; }

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage");
    std::vector<uint32_t> in;
    { FILE* f = fopen(argv[1], "rb"); if (!f) return fail("open input"); uint32_t x; while (fread(&x, 4, 1, f) == 1) in.push_back(x); fclose(f); }
    size_t at = 0; bool short_input = false;
    auto next = [&]() -> uint32_t { if (at >= in.size()) { short_input = true; return 0; } return in[at++]; };
    Layout L; L.n = (int)next(); L.off_census = (int)next(); L.off_sikver = (int)next(); L.off_n2bold = (int)next();
    if (L.n < 3 || L.n > 254) return fail("n");
    for (int i = 0; i < L.n; i++) L.lvl.push_back((int)next());
    const uint32_t nWires = next(), nPub = next();
    if (short_input || 3 * (size_t)nWires > in.size() - at || nPub + 1 > nWires) return fail("input too short");
    std::vector<uint8_t> inf[3]; for (auto& v : inf) v.resize(nWires);
    for (uint32_t w = 0; w < nWires; w++) for (int s = 0; s < 3; s++) inf[s][w] = next() != 0;
    const int n = L.n;
    const top::Ranges rg[2] = {abc::fold_group_ranges(L, 0), abc::fold_group_ranges(L, 1)};
    for (int t = 0; t < 2; t++) { if ((int)rg[t].size() != n) return fail("groups per tree"); for (auto& g : rg[t]) if (g.first < 1 || g.second < g.first || (uint32_t)g.second > nWires) return fail("group range"); }

    std::vector<uint32_t> out; size_t tuples = 0;
    const uint32_t nK = next();
    for (uint32_t k = 0; k < nK; k++) {
        const int K = (int)next(); if (short_input || K < 1 || K > top::MAX_K || K > n - 2) return fail("K");
        const std::vector<uint32_t> hw[2] = {top::hash_wires(rg[0], K), top::hash_wires(rg[1], K)};
        for (int t = 0; t < 2; t++) {
            if (hw[t].size() != (size_t)K * top::HASH_PER_GROUP) return fail("hash wires");
            for (size_t i = 0; i < hw[t].size(); i++) { const auto& g = rg[t][i / top::HASH_PER_GROUP]; if ((int)hw[t][i] < g.first || (int)hw[t][i] >= g.second) return fail("hash wire outside its group"); }
        }
        for (int Tc = 0; Tc <= K; Tc += K) for (int Dc = 0; Dc < n; Dc++) for (int Ts = 0; Ts <= K; Ts += K) for (int Ds = 0; Ds < n; Ds++) {
            if ((Tc && Dc <= K) || (Ts && Ds <= K)) continue;
            const top::Lists l = top::section_lists(nWires, nPub, rg, n, inf[0].data(), inf[1].data(), inf[2].data(), Tc, Dc, Ts, Ds);
            if (l.offA != 0 || l.offB != l.nA || l.offC != l.nA + l.nB || l.v.size() != (size_t)l.nA + l.nB + l.nC) return fail("list offsets");
            for (int s = 0; s < 3; s++) {
                const uint32_t first = s == 2 ? nPub + 1 : 0, off = s == 0 ? l.offA : s == 1 ? l.offB : l.offC, cnt = s == 0 ? l.nA : s == 1 ? l.nB : l.nC;
                std::vector<uint32_t> seen(nWires, 0);
                for (uint32_t i = 0; i < cnt; i++) { const uint32_t w = l.v[off + i]; if (w >= nWires || (i && w <= l.v[off + i - 1])) return fail("list not ascending"); seen[w]++; }
                for (int t = 0; t < 2; t++) {
                    const int T = t == 0 ? Tc : Ts, D = t == 0 ? Dc : Ds;
                    std::vector<uint32_t> sw;
                    for (int g = 0; g < T; g++) top::slot_wires(rg[t], g, inf[s].data(), nWires, first, sw);
                    for (uint32_t w : sw) seen[w]++;
                    for (int g = D; g < n; g++) for (int w = rg[t][(size_t)g].first; w < rg[t][(size_t)g].second; w++) if ((uint32_t)w >= first && !inf[s][(size_t)w]) seen[(size_t)w]++;      // behind suf[D] and the base
                }
                for (uint32_t w = 0; w < nWires; w++) if (seen[w] != (uint32_t)(w >= first && !inf[s][w])) return fail("a wire is not counted exactly once");
            }
            out.push_back(l.nA); out.push_back(l.nB); out.push_back(l.nC); tuples++;
        }
    }
    if (short_input) return fail("input too short");
    { FILE* f = fopen(argv[2], "wb"); if (!f) return fail("open output"); const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size(); if (fclose(f) != 0 || !ok) return fail("write output"); }
    printf("top fold: %zu tuples partition every section\ntop fold: ok\n", tuples);
    return 0;
}
