// lane_streams_host.cc -- which of a lane's roles share a stream in a pass (csrc/zkc_pass_plan.h: plan::lane_roles) as a stand-alone host program, built by
// tests/test_lane_streams_cpu.py with g++ under AddressSanitizer + UBSan.  Reads one case per line from standard input, integers in the order given below, and prints the
// function's answer as one line of integers, followed by the two fields of plan::stream_order that the plan of a one-lane call is made of.  The expected values are stated by
// the test, not here.
//   roles nb one_lane pass npasses lane0 tree lanes lane_streams reduce_stream serial_streams
//                                                          -> g1 g2 blind red streams   blind_on_st red_split      (0 st, 1 st2, 2 fin, 3 red)
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
        if (what != "roles") { printf("lane streams: FAILED unknown case '%s'\n", what.c_str()); return 1; }
        const int nb = (int)next(); const bool one_lane = next() != 0; const int pass = (int)next(), npasses = (int)next(), lane0 = (int)next(); const bool tree = next() != 0;
        const int lanes = (int)next();
        plan::Switches s; s.lane_streams = (int)next(); s.reduce_stream = next() != 0; s.serial_streams = next() != 0;
        if (short_line) { printf("lane streams: FAILED short line '%s'\n", line.c_str()); return 1; }
        const plan::LaneRoles r = plan::lane_roles(nb, one_lane, pass, npasses, lane0, tree, lanes, s);
        const plan::StreamOrder o = plan::stream_order(nb, one_lane, pass, npasses, lane0, tree, s);
        printf("%d %d %d %d %d %d %d\n", r.g1, r.g2, r.blind, r.red, r.streams, (int)o.blind_on_st, (int)o.red_split); cases++;
    }
    printf("lane streams: %zu cases\nlane streams: ok\n", cases);
    return 0;
}
