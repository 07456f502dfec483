// zkc_file_points.h -- the host-side check of a point read from a file, next to the device side of the same points (zkc_point_ops.h, zkc_ptau_check_* in zkc_kernels.h):
// used by the ctx = NULL paths of zkc_setup_ptau.hip and zkc_ptau_prepare.hip.  Host only, product code.
#pragma once
#include "zkc_pairing.h"

namespace zkc {
// a point read from a file: coordinates < q (the words are Montgomery form, so this is a test of the raw words) and on its curve; all zero is infinity and passes
template <class F> bool host_point_ok(const Affine<F>& a);
template <> inline bool host_point_ok<Fq>(const G1Affine& a) { return fp_std_lt_p<FqParams>(a.x.v) && fp_std_lt_p<FqParams>(a.y.v) && pairing::g1_on_curve(a); }
template <> inline bool host_point_ok<Fq2>(const G2Affine& a) {
    return fp_std_lt_p<FqParams>(a.x.c0.v) && fp_std_lt_p<FqParams>(a.x.c1.v) && fp_std_lt_p<FqParams>(a.y.c0.v) && fp_std_lt_p<FqParams>(a.y.c1.v) && pairing::g2_on_curve(a);
}
}  // namespace zkc
