// zkc_abc_rows.h -- which rows of a census key's A and B matrices a voter can change, and the lists buildABC runs over when the rest is copied from the template (product code).
// Plain C++17, no HIP: zkc_prove.hip (key load) and zkc_fold.hip (abc_rows) build a key's lists through it, tests/host/abc_rows_host.cc builds it with g++ under ASan/UBSan.
//
// The ONLY thing a row's constancy rests on is what zkc_fold_check (zkc_fold.hip) verifies, per proof: the witness equals the template on the wires of group (tree, g), for
// g < n-1 the non-control wires of level g, for g = n-1 the old-key block; wire 0 is compared with the old-key block of the census tree.  A pass is folded when no proof's
// old-key flag is set, and a proof's depth per tree is 1 + its highest level group that differs: every level group g >= depth then holds template values.  Hence
//   a row is constant for the depths (Dc, Ds) of a folded pass  <=>  every wire of the row is wire 0 or lies in a level group g of the census tree with g >= Dc or of
//                                                                    the sik tree with g >= Ds.
// A row that touches an old-key block is recorded (RowClass::old_key) and stays with the voter rows at every depth: the block's flag is the pass-wide condition, not a
// depth, and at depths (n-1, n-1) -- no level folded -- the voter rows are then exactly the rows that hold a wire other than wire 0.  Nothing else about the circuit is used:
// a wire outside the groups (inputs, control wires of a level, the hashes outside the trees) makes its rows voter rows for good.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace zkc { namespace abc {

constexpr uint8_t NO_LEVEL = 255;          // RowClass::min_c / min_s of a row without a wire in that tree's level groups (depths are at most 253)

// [start, end) wire ranges of one tree's groups 0 .. n-1, as zkc_fold_check walks them.  Layout: WitnessLayout (zkc_device.h) or anything with its n, off_census, off_sikver,
// off_n2bold and lvl_off(i)
template <class Layout>
std::vector<std::pair<int, int>> fold_group_ranges(const Layout& L, int tree) {
    std::vector<std::pair<int, int>> r; const int n = L.n, blk = tree == 0 ? L.off_census : L.off_sikver;
    for (int g = 0; g < n - 1; g++) {
        const int nctrl = (g == n - 3) + (g > 0 && g < n - 2) + 1;
        r.push_back({blk + L.lvl_off(g) + nctrl, blk + (g + 1 < n - 1 ? L.lvl_off(g + 1) : L.lvl_off(n - 1))});
    }
    r.push_back({blk + L.off_n2bold, blk + L.off_n2bold + 253 + 127 + 133});
    return r;
}

// per wire: WIRE_VOTER, WIRE_ONE (wire 0), or tree << 8 | group
constexpr uint16_t WIRE_VOTER = 0xffff, WIRE_ONE = 0xfffe;
inline std::vector<uint16_t> wire_groups(size_t nWires, const std::vector<std::pair<int, int>> ranges[2]) {
    std::vector<uint16_t> w(nWires, WIRE_VOTER);
    if (nWires) w[0] = WIRE_ONE;
    for (int tree = 0; tree < 2; tree++)
        for (size_t g = 0; g < ranges[tree].size(); g++)
            for (int i = std::max(ranges[tree][g].first, 1); i < ranges[tree][g].second && (size_t)i < nWires; i++) w[i] = (uint16_t)(tree << 8 | (int)g);
    return w;
}

struct RowClass {
    uint8_t voter;            // holds a wire outside the foldable groups that is not wire 0: never constant
    uint8_t old_key;          // holds a wire of an old-key block
    uint8_t min_c, min_s;     // smallest level group among its census / sik wires (NO_LEVEL: none)
};
// rows in compressed-row form: the wires of row r are col[rowptr[r] .. rowptr[r + 1]); n = groups per tree (the old-key block is group n - 1)
inline std::vector<RowClass> classify_rows(size_t nrows, const uint32_t* rowptr, const uint32_t* col, const std::vector<uint16_t>& wg, int n) {
    std::vector<RowClass> cls(nrows);
    for (size_t r = 0; r < nrows; r++) {
        RowClass c{0, 0, NO_LEVEL, NO_LEVEL};
        for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) {
            const uint16_t g = col[k] < wg.size() ? wg[col[k]] : WIRE_VOTER;
            if (g == WIRE_ONE) continue;
            if (g == WIRE_VOTER) { c.voter = 1; continue; }
            const int lvl = g & 0xff;
            if (lvl == n - 1) { c.old_key = 1; continue; }
            uint8_t& m = (g >> 8) ? c.min_s : c.min_c;
            if (lvl < m) m = (uint8_t)lvl;
        }
        cls[r] = c;
    }
    return cls;
}
inline bool row_constant(const RowClass& c, int Dc, int Ds) { return !c.voter && !c.old_key && (int)c.min_c >= Dc && (int)c.min_s >= Ds; }

// What buildABC computes in a folded pass of depths (Dc, Ds); everything else is the template's.
struct VoterRows {
    std::vector<uint32_t> rows;      // A / B rows as POSITIONS in the jagged-diagonal order (perm[position] = row), ascending: the long rows (positions < nlong of the key) first
    uint32_t nlong = 0;              // how many of them are long rows
    std::vector<uint32_t> crows;     // constraints i whose C_i = A_i B_i has to be formed: A row i or B row n_cons + i is listed (ascending)
    std::vector<uint32_t> wires;     // the wires the listed rows read (ascending)
};
// perm: sorted position -> row (zkc_jds.h), key_nlong: its long rows; rows [0, n_cons) are A, [n_cons, 2 n_cons) are B
inline VoterRows voter_rows(const std::vector<RowClass>& cls, const uint32_t* perm, uint32_t key_nlong, uint32_t n_cons, const uint32_t* rowptr, const uint32_t* col,
                            size_t nWires, int Dc, int Ds) {
    VoterRows v; const size_t nrows = cls.size();
    std::vector<uint8_t> cmark(n_cons, 0), wmark(nWires, 0);
    for (size_t s = 0; s < nrows; s++) {
        const uint32_t r = perm[s];
        if (row_constant(cls[r], Dc, Ds)) continue;
        v.rows.push_back((uint32_t)s); if (s < key_nlong) v.nlong++;
        cmark[r < n_cons ? r : r - n_cons] = 1;
        for (uint32_t k = rowptr[r]; k < rowptr[r + 1]; k++) if (col[k] < nWires) wmark[col[k]] = 1;
    }
    for (uint32_t i = 0; i < n_cons; i++) if (cmark[i]) v.crows.push_back(i);
    for (size_t w = 0; w < nWires; w++) if (wmark[w]) v.wires.push_back((uint32_t)w);
    return v;
}
struct RowCounts { size_t never = 0, constant_at_0 = 0; };      // rows no depth makes constant / rows constant when every level folds (Dc = Ds = 0)
inline RowCounts row_counts(const std::vector<RowClass>& cls) {
    RowCounts c; for (const RowClass& r : cls) { c.never += (r.voter || r.old_key); c.constant_at_0 += row_constant(r, 0, 0); } return c;
}

}}  // namespace zkc::abc
