// zkc_file_points.h -- the host-side check of a point read from a file, next to the device side of the same points (zkc_point_ops.h, points_check_dev in
// zkc_fixedbase_dev.h): used by the ctx = NULL paths of zkc_setup_ptau.hip and zkc_ptau_prepare.hip.  Host only, product code.
#pragma once
#include "zkc_host_util.h"
#include "zkc_pairing.h"

namespace zkc {
// a point read from a file: coordinates < q (the words are Montgomery form, so this is a test of the raw words) and on its curve; all zero is infinity and passes
template <class F> bool host_point_ok(const Affine<F>& a);
template <> inline bool host_point_ok<Fq>(const G1Affine& a) { return fp_std_lt_p<FqParams>(a.x.v) && fp_std_lt_p<FqParams>(a.y.v) && pairing::g1_on_curve(a); }
template <> inline bool host_point_ok<Fq2>(const G2Affine& a) {
    return fp_std_lt_p<FqParams>(a.x.c0.v) && fp_std_lt_p<FqParams>(a.x.c1.v) && fp_std_lt_p<FqParams>(a.y.c0.v) && fp_std_lt_p<FqParams>(a.y.c1.v) && pairing::g2_on_curve(a);
}
// the smallest index of a point of p[0 .. n) that host_point_ok refuses, 0xffffffff when there is none; on the threads of par_chunks
template <class F> uint32_t host_first_bad(const Affine<F>* p, size_t n) {
    std::atomic<uint32_t> first_bad{0xffffffffu};
    par_chunks(n, 4096, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) if (!host_point_ok<F>(p[i])) { uint32_t cur = first_bad.load(); while ((uint32_t)i < cur && !first_bad.compare_exchange_weak(cur, (uint32_t)i)) {} break; }
    });
    return first_bad.load();
}
}  // namespace zkc
