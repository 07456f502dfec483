// jds_host.cc -- the jagged-diagonal sparse-row builder (csrc/zkc_jds.h) as a stand-alone host program over a 32-byte stand-in for Fr, built by
// tests/test_jds_cpu.py with g++ under AddressSanitizer + UBSan.  For every case: perm is a permutation, the sorted lengths do not increase, equal lengths keep their
// input order, jdptr[0] = 0 and jdptr[maxlen] = the number of terms, slot jdptr[k] + s read back gives every input row term for term with exactly the marked column
// words, nlong counts the rows longer than the threshold, and the unit count is right.
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_jds.h"
#include <cstdio>
#include <cstring>
#include <string>

using namespace zkc;

struct V32 {
    uint32_t v[8];
    bool operator==(const V32& o) const { return memcmp(v, o.v, 32) == 0; }
};
struct Term { uint32_t wire; V32 val; };
typedef std::vector<std::vector<Term>> Rows;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }
static V32 some_value() { V32 x; for (int i = 0; i < 8; i++) x.v[i] = rnd(); return x; }
static V32 PLUS, MINUS;

static Term some_term() { return Term{rnd() & MV_COL, some_value()}; }
static std::vector<Term> row_of(size_t n) { std::vector<Term> r(n); for (Term& t : r) t = some_term(); return r; }

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("%s: FAILED %s (line %d)\n", name.c_str(), #cond, __LINE__); g_bad++; return; } } while (0)

static void run_case(const std::string& name, const Rows& rows, uint32_t T) {
    const size_t n = rows.size();
    const JdsLayout L = jds_layout(n, [&](uint32_t r) { return rows[r].size(); }, T);
    uint64_t nterms = 0, want_long = 0, want_unit = 0; size_t maxlen = 0;
    for (const auto& r : rows) {
        nterms += r.size(); want_long += r.size() > T; maxlen = std::max(maxlen, r.size());
        for (const Term& t : r) want_unit += (t.val == PLUS) || (t.val == MINUS);
    }
    CHECK(L.perm.size() == n && L.rowlen.size() == n && L.nterms == nterms);
    std::vector<char> seen(n, 0);
    for (size_t s = 0; s < n; s++) { CHECK(L.perm[s] < n && !seen[L.perm[s]]); seen[L.perm[s]] = 1; CHECK(L.rowlen[s] == rows[L.perm[s]].size()); }
    for (size_t s = 1; s < n; s++) {
        CHECK(L.rowlen[s - 1] >= L.rowlen[s]);
        if (L.rowlen[s - 1] == L.rowlen[s]) CHECK(L.perm[s - 1] < L.perm[s]);        // stable
    }
    CHECK(L.jdptr.size() == maxlen + 1 && L.jdptr[0] == 0 && L.jdptr[maxlen] == nterms);
    CHECK(L.nlong == want_long);
    for (size_t s = 0; s < n; s++) CHECK((s < L.nlong) == (L.rowlen[s] > T));
    // exactly nterms slots, each guarded on both sides: a slot outside [0, nterms) is the sanitizer's to report
    std::vector<uint32_t> col(nterms, 0xffffffffu); std::vector<V32> val(nterms);
    std::vector<char> hit(nterms, 0);
    const uint64_t nunit = jds_fill(L, [&](uint32_t r, uint32_t k) { return std::pair<uint32_t, V32>(rows[r][k].wire, rows[r][k].val); }, PLUS, MINUS, col.data(), val.data());
    CHECK(nunit == want_unit);
    for (size_t s = 0; s < n; s++) {
        const auto& r = rows[L.perm[s]];
        for (size_t k = 0; k < r.size(); k++) {
            CHECK(L.jdptr[k] + s < L.jdptr[k + 1]);
            const size_t slot = (size_t)L.jdptr[k] + s;
            CHECK(!hit[slot]); hit[slot] = 1;
            const uint32_t want = r[k].wire | (r[k].val == PLUS ? MV_UNIT : r[k].val == MINUS ? (MV_UNIT | MV_NEG) : 0u);
            CHECK(col[slot] == want && (col[slot] & MV_COL) == r[k].wire && val[slot] == r[k].val);
        }
    }
    for (uint64_t i = 0; i < nterms; i++) CHECK(hit[i]);
    printf("%s: ok (%zu rows, %llu terms, %u long, %llu units)\n", name.c_str(), n, (unsigned long long)nterms, L.nlong, (unsigned long long)nunit);
}

int main() {
    static_assert(sizeof(V32) == 32, "stand-in for Fr");
    static_assert(MV_UNIT == 0x80000000u && MV_NEG == 0x40000000u && MV_COL == 0x3fffffffu && (MV_UNIT | MV_NEG | MV_COL) == 0xffffffffu, "mark bits");
    PLUS = some_value(); MINUS = some_value();
    for (uint32_t T : {16u, 48u}) {
        const std::string t = " (T = " + std::to_string(T) + ")";
        run_case("no rows" + t, Rows{}, T);
        run_case("rows all empty" + t, Rows(7), T);
        run_case("a single row" + t, Rows{row_of(3)}, T);
        run_case("a single empty row" + t, Rows{row_of(0)}, T);
        run_case("a single long row" + t, Rows{row_of(T + 1)}, T);
        {   // the nlong boundary, in an order that the sort has to change, between short and empty rows
            Rows r{row_of(2), row_of(T), row_of(0), row_of(T + 1), row_of(T - 1), row_of(1), row_of(T + 1), row_of(T)};
            run_case("lengths T - 1, T, T + 1" + t, r, T);
        }
        {   // many rows of equal length keep their input order
            Rows r; for (int i = 0; i < 300; i++) r.push_back(row_of(3));
            run_case("300 rows of 3 terms" + t, r, T);
            for (int i = 0; i < 300; i += 7) r[i] = row_of(5);
            run_case("rows of 3 and 5 terms interleaved" + t, r, T);
        }
        {   // one row of 521 terms (the census circuit's longest merged row) among short ones
            Rows r; for (int i = 0; i < 130; i++) r.push_back(row_of(rnd() % 5));
            r[77] = row_of(521);
            run_case("one row of 521 terms among short ones" + t, r, T);
        }
        {   // the +1 and -1 markers, and values that differ from them in one bit
            Rows r; for (int i = 0; i < 40; i++) r.push_back(row_of(1 + rnd() % (T + 4)));
            uint64_t k = 0;
            for (auto& row : r) for (Term& x : row) {
                switch (k++ % 6) {
                    case 0: x.val = PLUS; break;
                    case 1: x.val = MINUS; break;
                    case 2: x.val = PLUS; x.val.v[rnd() % 8] ^= 1u << (rnd() % 32); break;
                    case 3: x.val = MINUS; x.val.v[rnd() % 8] ^= 1u << (rnd() % 32); break;
                    default: break;
                }
            }
            r[0][0].wire = MV_COL; r[0][0].val = MINUS;                        // the largest wire index beside both marks
            run_case("unit markers and their one-bit neighbours" + t, r, T);
        }
    }
    if (g_bad) { printf("jds builder: %d case(s) FAILED\n", g_bad); return 1; }
    printf("jds builder: ok\n");
    return 0;
}
