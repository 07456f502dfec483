// c_rows_plan_host.cc -- the decision whether a pass leaves out the transform pair of C, and the H job's list on that path (csrc/zkc_pass_plan.h: c_rows_rule, c_rows_candidate,
// c_rows, h_vmap), as a stand-alone host program, built by tests/test_c_rows_plan_cpu.py with g++ under AddressSanitizer + UBSan.  One case per line on standard input, a word and
// then integers; one line of integers per case on standard output.  The expected values are stated by the test, not here.
//   rule k nw_h n logn beta_milli                                                        -> 0 / 1
//   take c_h n nb tree mode beta_milli wide abc_folded early k logn section_entries cap_p_words w1_entries      -> taken (0 / 1), candidate before the lane's caps are asked (0 / 1)
//   vmap n k crows[k]                                                                     -> the n + k entries
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_pass_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace zkc;

int main() {
    std::string line; size_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line); std::string what; if (!(in >> what)) continue;
        bool short_line = false;
        auto next = [&]() -> long long { long long v = 0; if (!(in >> v)) short_line = true; return v; };
        std::ostringstream out;
        if (what == "rule") {
            const uint32_t k = (uint32_t)next(); const int nw = (int)next(); const uint32_t n = (uint32_t)next(); const int logn = (int)next(); const uint32_t beta = (uint32_t)next();
            if (!short_line) out << (plan::c_rows_rule(k, nw, n, logn, beta) ? 1 : 0);
        } else if (what == "take") {
            plan::KeyShape key{}; key.c_h = (int)next(); key.n = (uint32_t)next();
            const int nb = (int)next(); plan::PassShape p{}; p.tree = next() != 0;
            plan::CRowsIn ci{}; ci.mode = (int)next(); ci.beta_milli = (uint32_t)next(); ci.wide_table = next() != 0; ci.abc_folded = next() != 0; ci.early = next() != 0;
            ci.k = (uint32_t)next(); ci.logn = (int)next(); ci.section_entries = (size_t)next(); ci.cap_p_words = (size_t)next();
            plan::LaneCaps cap{}; cap.w1_entries = (size_t)next();
            if (!short_line) out << (plan::c_rows(key, p, nb, cap, ci) ? 1 : 0) << ' ' << (plan::c_rows_candidate(key, p, nb, ci) ? 1 : 0);
        } else if (what == "vmap") {
            const uint32_t n = (uint32_t)next(), k = (uint32_t)next(); std::vector<uint32_t> crows; for (uint32_t i = 0; i < k; i++) crows.push_back((uint32_t)next());
            if (!short_line) { const std::vector<uint32_t> v = plan::h_vmap(n, crows.data(), k); for (size_t i = 0; i < v.size(); i++) out << (i ? " " : "") << v[i]; }
        } else { printf("FAILED: unknown case %s\n", what.c_str()); return 1; }
        if (short_line) { printf("FAILED: short line: %s\n", line.c_str()); return 1; }
        printf("%s\n", out.str().c_str()); cases++;
    }
    printf("c rows plan: %zu cases\nc rows plan: ok\n", cases);
    return 0;
}
