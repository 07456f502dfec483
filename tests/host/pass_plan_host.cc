// pass_plan_host.cc -- the host decisions of a batch call and its passes (csrc/zkc_pass_plan.h) as a stand-alone host program, built by tests/test_pass_plan_cpu.py with g++
// under AddressSanitizer + UBSan.  Reads one case per line from standard input -- a word that names the function, then its arguments as integers in the order given below --
// and prints the function's results as one line of integers.  The expected values are stated by the test, not here.
//   split B max_inflight                                   -> npasses per_pass
//   depth n f[n]                                           -> D (-1: foreign)
//   early n stride voters ok status[voters] early_depth[2 voters] flags[voters stride]       -> first voter that disagrees, or -1
//   top K nslots early nb dc[nb] ds[nb] words[2 nb] valid[2 nslots]                          -> tc[nb] ts[nb] nseeds (q tree slot)[nseeds]
//   shape c_sec c_h c_deep nv np n lone_table fb4 w1_entries w1_buckets w1_jobs w2_entries vw_big vw_small vw_g2 deep_wires nb listed (nA nB nC)[nb if listed]
//                                                          -> vws vwb vw_g2 deep cw oA oB1 oC c2 tree per      (tables: A 1000, B1 2000, C 3000; second tables 4000, 5000, 6000)
//   views nv np listed offA nA offB nB offC nC              -> per section A, B1, C: scalars - w (words), vmap - d (-1: none), count, tbl_off, tbl_count, pt_shift
//   order nb one_lane pass npasses lane0 tree matvec_inline g2_acc_hold g2_acc_early reduce_stream serial_streams
//                                                          -> mv_prefetch mv_done g2_acc_with_sort red_split blind_on_st
#include "../../zk-franchise-proof-circuit_amd/csrc/zkc_pass_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace zkc;

struct Sizes { const uint32_t* d; uint32_t offA, nA, offB, nB, offC, nC; };

int main() {
    std::string line; size_t cases = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line); std::string what; if (!(in >> what)) continue;
        bool short_line = false;
        auto next = [&]() -> long long { long long v = 0; if (!(in >> v)) short_line = true; return v; };
        auto many = [&](size_t cnt) { std::vector<long long> v(cnt); for (auto& x : v) x = next(); return v; };
        std::ostringstream out;
        if (what == "split") {
            const int B = (int)next(), mi = (int)next();
            const plan::CallSplit s = plan::call_split(B, mi); out << s.npasses << ' ' << s.per_pass;
        } else if (what == "depth") {
            const int n = (int)next(); std::vector<uint32_t> f; for (long long x : many((size_t)n)) f.push_back((uint32_t)x);
            if (!short_line) out << plan::row_depth(f.data(), n);
        } else if (what == "early") {
            const int n = (int)next(); const size_t stride = (size_t)next(); const int voters = (int)next(); const uint32_t ok = (uint32_t)next();
            std::vector<uint32_t> status, flags; std::vector<uint8_t> ed;
            for (long long x : many((size_t)voters)) status.push_back((uint32_t)x);
            for (long long x : many(2 * (size_t)voters)) ed.push_back((uint8_t)x);
            for (long long x : many((size_t)voters * stride)) flags.push_back((uint32_t)x);
            if (!short_line) out << plan::early_disagrees(status.data(), ok, flags.data(), stride, n, ed.data(), voters);
        } else if (what == "top") {
            const int K = (int)next(); const uint32_t nslots = (uint32_t)next(); const bool early = next() != 0; const int nb = (int)next();
            std::vector<uint8_t> dc, ds, valid; std::vector<uint32_t> words;
            for (long long x : many((size_t)nb)) dc.push_back((uint8_t)x);
            for (long long x : many((size_t)nb)) ds.push_back((uint8_t)x);
            for (long long x : many(2 * (size_t)nb)) words.push_back((uint32_t)x);
            for (long long x : many(2 * (size_t)nslots)) valid.push_back((uint8_t)x);
            std::vector<uint16_t> tc((size_t)nb, 7), ts((size_t)nb, 7); std::vector<plan::TopSeed> seeds(1, plan::TopSeed{99, 99, 99});      // (stale content: the function owns all three)
            if (!short_line) {
                plan::top_fold(dc.data(), ds.data(), words.data(), 2, K, nslots, valid.data(), early, nb, tc.data(), ts.data(), seeds);
                for (uint16_t x : tc) out << x << ' ';
                for (uint16_t x : ts) out << x << ' ';
                out << seeds.size(); for (const plan::TopSeed& s : seeds) out << ' ' << s.q << ' ' << s.tree << ' ' << s.slot;
            }
        } else if (what == "shape") {
            plan::KeyShape k{}; k.c_sec = (int)next(); k.c_h = (int)next(); k.c_deep = (int)next(); k.nv = (uint32_t)next(); k.np = (uint32_t)next(); k.n = (uint32_t)next();
            k.lone_table = next() != 0; k.fb4 = next() != 0; k.offA = 1000; k.offB1 = 2000; k.offC = 3000; k.offA_deep = 4000; k.offB1_deep = 5000; k.offC_deep = 6000;
            plan::LaneCaps cap{}; cap.w1_entries = (size_t)next(); cap.w1_buckets = (size_t)next(); cap.w1_jobs = (int)next(); cap.w2_entries = (size_t)next();
            plan::Switches s; s.vw_big = (uint32_t)next(); s.vw_small = (uint32_t)next(); s.vw_g2 = (uint32_t)next(); s.deep_wires = (size_t)next();
            const int nb = (int)next(); const bool listed = next() != 0;
            std::vector<Sizes> l; if (listed) for (int q = 0; q < nb; q++) { Sizes z{}; z.nA = (uint32_t)next(); z.nB = (uint32_t)next(); z.nC = (uint32_t)next(); l.push_back(z); }
            if (!short_line) {
                const plan::PassShape p = plan::pass_shape(k, nb, listed ? l.data() : (const Sizes*)nullptr, cap, s);
                out << p.vws << ' ' << p.vwb << ' ' << p.vw_g2 << ' ' << p.deep << ' ' << p.cw << ' ' << p.oA << ' ' << p.oB1 << ' ' << p.oC << ' ' << p.c2 << ' ' << p.tree << ' ' << p.per;
            }
        } else if (what == "views") {
            plan::KeyShape k{}; k.nv = (uint32_t)next(); k.np = (uint32_t)next(); const bool listed = next() != 0;
            plan::PassShape p{}; p.oA = 1000; p.oB1 = 2000; p.oC = 3000;
            std::vector<uint32_t> w(8 * ((size_t)k.np + 2)), d(4096);
            Sizes z{}; z.d = d.data(); z.offA = (uint32_t)next(); z.nA = (uint32_t)next(); z.offB = (uint32_t)next(); z.nB = (uint32_t)next(); z.offC = (uint32_t)next(); z.nC = (uint32_t)next();
            if (!short_line) {
                const plan::ProofViews v = plan::proof_views(k, p, w.data(), listed ? &z : (const Sizes*)nullptr);
                for (const plan::SectionView* s : {&v.A, &v.B1, &v.C})
                    out << (s->scalars - w.data()) << ' ' << (s->vmap ? (long long)(s->vmap - d.data()) : -1ll) << ' ' << s->count << ' ' << s->tbl_off << ' ' << s->tbl_count << ' ' << s->pt_shift << ' ';
            }
        } else if (what == "order") {
            const int nb = (int)next(); const bool one_lane = next() != 0; const int pass = (int)next(), npasses = (int)next(), lane0 = (int)next(); const bool tree = next() != 0;
            plan::Switches s; s.matvec_inline = next() != 0; s.g2_acc_hold = next() != 0; s.g2_acc_early = next() != 0; s.reduce_stream = next() != 0; s.serial_streams = next() != 0;
            const plan::StreamOrder o = plan::stream_order(nb, one_lane, pass, npasses, lane0, tree, s);
            out << o.mv_prefetch << ' ' << o.mv_done << ' ' << o.g2_acc_with_sort << ' ' << o.red_split << ' ' << o.blind_on_st;
        } else { printf("pass plan: FAILED unknown case '%s'\n", what.c_str()); return 1; }
        if (short_line) { printf("pass plan: FAILED short line '%s'\n", line.c_str()); return 1; }
        printf("%s\n", out.str().c_str()); cases++;
    }
    printf("pass plan: %zu cases\npass plan: ok\n", cases);
    return 0;
}
