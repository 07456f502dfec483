// abc_rows_host.cc -- the row classes of a census key's A / B matrices and the voter-row lists of buildABC (csrc/zkc_abc_rows.h over csrc/zkc_jds.h) as a stand-alone host
// program, built by tests/test_abc_rows_cpu.py with g++ under AddressSanitizer + UBSan.
//   abc_rows_host IN OUT
// IN  (u32 little endian): n, off_census, off_sikver, off_n2bold, lvl_off[0 .. n), nWires, nCons, long_over, nCoeffs, nCoeffs x (matrix, constraint, wire) in the key's
//     order, nPairs, nPairs x (Dc, Ds).  The layout numbers stand in for WitnessLayout (zkc_device.h), which needs HIP.
// OUT (u32): rows never constant, rows constant at depths (0, 0), then per pair: nrows, nlong, nC, nW, the listed rows as INPUT rows (perm[position]) in list order, the C
//     constraints, the wires.  The rows are put into compressed-row form and jagged-diagonal order the way zkc_zkey_load does it.
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_abc_rows.h"
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_jds.h"
#include <cstdio>
#include <cstdlib>

using namespace zkc;

struct Layout {
    int n = 0, off_census = 0, off_sikver = 0, off_n2bold = 0; std::vector<int> lvl;
    int lvl_off(int i) const { return lvl.at((size_t)i); }
};
static int fail(const char* what) { printf("abc rows: FAILED %s\n", what); return 1; }

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage");
    std::vector<uint32_t> in;
    { FILE* f = fopen(argv[1], "rb"); if (!f) return fail("open input"); uint32_t x; while (fread(&x, 4, 1, f) == 1) in.push_back(x); fclose(f); }
    size_t at = 0; bool short_input = false;
    auto next = [&]() -> uint32_t { if (at >= in.size()) { short_input = true; return 0; } return in[at++]; };
    Layout L; L.n = (int)next(); L.off_census = (int)next(); L.off_sikver = (int)next(); L.off_n2bold = (int)next();
    if (L.n < 3 || L.n > 254) return fail("n");
    for (int i = 0; i < L.n; i++) L.lvl.push_back((int)next());
    const uint32_t nWires = next(), nCons = next(), long_over = next(), nCoeffs = next();
    if (short_input || (size_t)nCoeffs * 3 > in.size() - at) return fail("input too short");
    const size_t nrows = 2 * (size_t)nCons; const uint32_t* co = in.data() + at; at += 3 * (size_t)nCoeffs;
    std::vector<uint32_t> rowptr(nrows + 1, 0), col(nCoeffs);
    for (uint32_t i = 0; i < nCoeffs; i++) { if (co[3 * i] > 1 || co[3 * i + 1] >= nCons || co[3 * i + 2] >= nWires) return fail("coefficient out of range"); rowptr[(size_t)co[3 * i] * nCons + co[3 * i + 1] + 1]++; }
    for (size_t r = 0; r < nrows; r++) rowptr[r + 1] += rowptr[r];
    { std::vector<uint32_t> fill(rowptr.begin(), rowptr.end() - 1); for (uint32_t i = 0; i < nCoeffs; i++) col[fill[(size_t)co[3 * i] * nCons + co[3 * i + 1]]++] = co[3 * i + 2]; }
    const JdsLayout J = jds_layout(nrows, [&](uint32_t r) { return rowptr[r + 1] - rowptr[r]; }, long_over);

    const std::vector<std::pair<int, int>> rg[2] = {abc::fold_group_ranges(L, 0), abc::fold_group_ranges(L, 1)};
    for (int t = 0; t < 2; t++) { if ((int)rg[t].size() != L.n) return fail("groups per tree"); for (auto& g : rg[t]) if (g.first < 1 || g.second < g.first || (uint32_t)g.second > nWires) return fail("group range"); }
    const std::vector<abc::RowClass> cls = abc::classify_rows(nrows, rowptr.data(), col.data(), abc::wire_groups(nWires, rg), L.n);
    if (cls.size() != nrows) return fail("classes");
    const abc::RowCounts cnt = abc::row_counts(cls);
    if (cnt.never + cnt.constant_at_0 != nrows) return fail("never + constant at 0 != rows");
    std::vector<uint32_t> out = {(uint32_t)cnt.never, (uint32_t)cnt.constant_at_0};

    const uint32_t npairs = next();
    for (uint32_t p = 0; p < npairs; p++) {
        const int Dc = (int)next(), Ds = (int)next(); if (short_input) return fail("pairs");
        const abc::VoterRows v = abc::voter_rows(cls, J.perm.data(), J.nlong, nCons, rowptr.data(), col.data(), nWires, Dc, Ds);
        // what the kernels rely on: ascending positions inside the key's rows, the long rows in front and counted, C and wire lists ascending and in range
        if (v.nlong > v.rows.size()) return fail("nlong");
        for (size_t i = 0; i < v.rows.size(); i++) {
            if (v.rows[i] >= nrows || (i && v.rows[i] <= v.rows[i - 1])) return fail("positions not ascending");
            if ((i < v.nlong) != (v.rows[i] < J.nlong)) return fail("long rows not in front");
            if (i && J.rowlen[v.rows[i]] > J.rowlen[v.rows[i - 1]]) return fail("lengths increase");
        }
        for (size_t i = 0; i < v.crows.size(); i++) if (v.crows[i] >= nCons || (i && v.crows[i] <= v.crows[i - 1])) return fail("C rows");
        for (size_t i = 0; i < v.wires.size(); i++) if (v.wires[i] >= nWires || (i && v.wires[i] <= v.wires[i - 1])) return fail("wires");
        if (v.rows.size() < cnt.never) return fail("a never-constant row is missing");
        out.push_back((uint32_t)v.rows.size()); out.push_back(v.nlong); out.push_back((uint32_t)v.crows.size()); out.push_back((uint32_t)v.wires.size());
        for (uint32_t s : v.rows) out.push_back(J.perm[s]);
        out.insert(out.end(), v.crows.begin(), v.crows.end()); out.insert(out.end(), v.wires.begin(), v.wires.end());
        printf("abc rows (%d, %d): %zu of %zu rows listed, %u long, %zu C rows, %zu wires\n", Dc, Ds, v.rows.size(), nrows, v.nlong, v.crows.size(), v.wires.size());
    }
    { FILE* f = fopen(argv[2], "wb"); if (!f) return fail("open output"); const bool ok = fwrite(out.data(), 4, out.size(), f) == out.size(); if (fclose(f) != 0 || !ok) return fail("write output"); }
    printf("abc rows: never constant %zu, constant at depth 0 %zu of %zu\nabc rows: ok\n", cnt.never, cnt.constant_at_0, nrows);
    return 0;
}
