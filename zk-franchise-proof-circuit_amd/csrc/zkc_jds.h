// zkc_jds.h -- the one builder of the jagged-diagonal (JDS) sparse-row layout that zkc_matvec_jds (zkc_ntt.hip; rows = (matrix, constraint) of a key's section 4) and
// zkc_r1cs_check_rows (zkc_r1cs.hip; rows = A | B | C of a constraint, merged) read through the same mv_term (zkc_kernels.h).  Plain C++17, no HIP, a template on the value
// type: tests/host/jds_host.cc builds it with g++ under ASan/UBSan over a 32-byte stand-in for Fr.
//
// Rows are sorted by decreasing length (stable: rows of equal length keep their input order); slot jdptr[k] + s holds term k of sorted row s, so the loads of neighbouring
// lanes are contiguous and their work is (nearly) equal.  The first `nlong` sorted rows have more terms than the caller's threshold: the kernels give those a wave each.
// A value equal to the caller's +1 or -1 is marked in the two top bits of its column word, and the kernels add or subtract the wire instead of multiplying; the wire index
// itself must therefore be below 2^30 (the callers refuse larger files).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace zkc {

constexpr uint32_t MV_UNIT = 0x80000000u, MV_NEG = 0x40000000u, MV_COL = 0x3fffffffu;

struct JdsLayout {
    std::vector<uint32_t> perm;        // sorted position -> input row
    std::vector<uint32_t> rowlen;      // terms of the row at each sorted position: non-increasing
    std::vector<uint32_t> jdptr;       // maxlen + 1 entries: jdptr[k] = first slot of the k-th terms, jdptr[maxlen] = nterms
    uint32_t nlong = 0;                // rows with more than `long_over` terms (the first nlong sorted positions)
    uint64_t nterms = 0;
};

// len_of(input row) -> its number of terms
template <class LenOf>
JdsLayout jds_layout(size_t nrows, LenOf len_of, uint32_t long_over) {
    JdsLayout L;
    std::vector<uint32_t> len(nrows);
    for (size_t r = 0; r < nrows; r++) { len[r] = (uint32_t)len_of((uint32_t)r); L.nterms += len[r]; }
    L.perm.resize(nrows); L.rowlen.resize(nrows);
    for (size_t r = 0; r < nrows; r++) L.perm[r] = (uint32_t)r;
    std::stable_sort(L.perm.begin(), L.perm.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
    for (size_t s = 0; s < nrows; s++) L.rowlen[s] = len[L.perm[s]];
    const uint32_t maxlen = nrows ? L.rowlen[0] : 0;
    while (L.nlong < nrows && L.rowlen[L.nlong] > long_over) L.nlong++;
    L.jdptr.assign((size_t)maxlen + 1, 0);
    size_t live = nrows;                                        // rows that have a k-th term
    for (uint32_t k = 0; k < maxlen; k++) { while (live > 0 && L.rowlen[live - 1] <= k) live--; L.jdptr[k + 1] = L.jdptr[k] + (uint32_t)live; }
    return L;
}

// term(input row, k) -> (wire, value) of the k-th term of that row; col and val have room for L.nterms entries.  Returns the number of unit (+1 / -1) coefficients.
template <class V, class Term>
uint64_t jds_fill(const JdsLayout& L, Term term, const V& plus_one, const V& minus_one, uint32_t* col, V* val) {
    uint64_t nunit = 0;
    for (size_t s = 0; s < L.perm.size(); s++)
        for (uint32_t k = 0; k < L.rowlen[s]; k++) {
            const size_t dst = (size_t)L.jdptr[k] + s;
            const std::pair<uint32_t, V> t = term(L.perm[s], k);
            uint32_t wire = t.first; const V& v = t.second;
            if (v == plus_one) { wire |= MV_UNIT; nunit++; } else if (v == minus_one) { wire |= MV_UNIT | MV_NEG; nunit++; }
            col[dst] = wire; val[dst] = v;
        }
    return nunit;
}

}  // namespace zkc
