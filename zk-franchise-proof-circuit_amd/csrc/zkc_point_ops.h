// zkc_point_ops.h -- G1 and G2 behind one interface for the kernels that work on the points of a file (zkc_phase2.hip: one scalar times many points; zkc_setup_ptau.hip:
// a sparse matrix times a vector of points; zkc_ecntt.hip: a transform over points; zkc_ptau_verify.hip: two weighted sums over consecutive points): the check of such a point, an accumulator in radix 2^29, set from / added to by an
// affine point in Montgomery words, the complete additions of two such accumulators, and the trait by which host code that is generic in the field picks the group
// (GroupOf).  The merge kernel of the MSM's bucket reduction (zkc_msm_merge29, zkc_msm.hip) is instantiated with the same two structs, for the complete addition and the
// way in and out of the accumulator (from_xyzz, add, is_inf, set_inf, leave).  The operations are device only and the header needs hipcc: a plain C++ host program (tests/host/*.cc) cannot include it.  Product code.
//
// The additions.  Unlike a prover's bases these points are an adversary's, or merely unlucky, and an addition can meet equal points, opposite points and infinity.  So:
// an all-zero point is skipped, an accumulator at infinity is set rather than added to, and f29_madd's `false` return is taken at every mixed addition -- equal: double
// the accumulator (it holds that very point), opposite: back to infinity -- in both groups (add_point).  G::add is the complete f29_pt_add / f29g2_pt_add.
// Where the GPU tests reach each case ("setup": tests/test_gpu_ptau_setup.py; "repeats": tests/test_gpu_ptau_setup_repeats.py, named by the rows of
// tests/repeat_circuits.py, whose A and B1 rows are G1 and whose B2 row of the same shape is G2):
//   infinity              G1, G2: setup and tests/test_gpu_ptau_prepare.py with tau a root of unity (all but one Lagrange point are infinity, and the monomial points
//                         repeat); repeats `pmp` (set again after P - P), `empty`, and every row but the long ones with tau a root of unity
//   add_point, equal      G1: setup, the K rows with alpha = beta.  G1, G2: repeats `pp`, `p5` (then lean additions onto what G::dbl left), `kk` (two scaled terms), and
//                         the first two terms of every segment of the long rows (zkc_ptau_acc)
//   add_point, opposite   G1: setup, the K rows with alpha = -beta.  G1, G2: repeats `pm`, `pmp`, `k-k`, `half` (zkc_ptau_acc)
//   G::add, equal         G1, G2: repeats `red_eq` at the first reduction step, `red_eq2` at the second, `red3_eq` at the third (zkc_ptau_red)
//   G::add, opposite      G1, G2: repeats `red_op` (zkc_ptau_red)
// zkc_wsum (zkc_ptau_verify.hip) reaches all three in both groups, and in G2 on twist points outside G2, in tests/test_gpu_ptau_verify.py: the sets `same` (equal), `alternating`
// (opposite, then set again from infinity) and `infinities`, and the files with tau = 1, tau = r - 1 and tau on the domain; its partial sums meet G::add's cases in zkc_ptau_red there.
// The double-and-add users of add_point (zkc_ptau_scale, the load kernel of zkc_ecntt.hip) meet no equal or opposite operand for a scalar below r, so no test takes the
// `false` return there; zkc_p2_scale_g1 walks signed digits and meets it for the scalar r - 2 alone (zkc_phase2.hip).
#pragma once
#include "zkc_f29.h"
#include "zkc_f29_g1.h"
#include "zkc_f29_g2.h"

namespace zkc {

template <int W> __device__ __forceinline__ void load_words(uint32_t* w, const uint32_t* __restrict__ p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < W / 4; k++) { const uint4 v = q[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
}
template <int W> __device__ __forceinline__ bool all_zero(const uint32_t* w) { uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < W; k++) o |= w[k]; return o == 0; }
__device__ __forceinline__ Fq fq_of(const uint32_t* w) { Fq a;
#pragma unroll
    for (int k = 0; k < 8; k++) a.v[k] = w[k]; return a; }
// the leading bit of the 256-bit k leaves as the return value; k moves up by one
__device__ __forceinline__ uint32_t shl1_out(uint32_t k[8]) {
    const uint32_t top = k[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    k[0] <<= 1;
    return top;
}

struct G1Ops {
    static constexpr int W = 16;                                 // words of an affine point
    typedef Fq F; typedef Acc29 Acc;
    struct Pt { uint32_t x[9], y[9]; };
    __device__ static __forceinline__ Fq coord(const uint32_t* w) { return fq_of(w); }
    __device__ static __forceinline__ Pt enter(const uint32_t* w, bool neg) {
        Pt p; Fq Y = fq_of(w + 8); if (neg) Y = fp_neg(Y);
        f29_enter_fq(p.x, w); f29_enter_fq(p.y, Y.v);            // below 1.2 p each: well inside what f29_madd takes
        return p;
    }
    __device__ static __forceinline__ void set(Acc& a, const Pt& p) {
#pragma unroll
        for (int k = 0; k < 9; k++) { a.X[k] = p.x[k]; a.Y[k] = p.y[k]; a.ZZ[k] = a.ZZZ[k] = F29K<FqParams>::one.l[k]; }
    }
    __device__ static __forceinline__ bool madd(Acc& a, const Pt& p, bool& same_y) { return f29_madd(a, p.x, p.y, same_y); }
    __device__ static __forceinline__ void dbl(Acc& a) { f29_acc_dbl(a); }
    __device__ static __forceinline__ XYZZ<Fq> leave(const Acc& a) { return f29_pt_to_xyzz(a); }
    // the complete operations' own form (loose, zkc_f29_g1.h)
    __device__ static __forceinline__ Acc from_xyzz(const XYZZ<Fq>& p) { return f29_pt_from_xyzz(p); }
    __device__ static __forceinline__ void add(Acc& r, const Acc& a, const Acc& b) { f29_pt_add(r, a, b); }
    __device__ static __forceinline__ void pt_dbl(Acc& r, const Acc& a) { f29_pt_dbl(r, a); }
    __device__ static __forceinline__ bool is_inf(const Acc& a) { return f29_pt_is_inf(a); }
    __device__ static __forceinline__ void set_inf(Acc& a) { f29_pt_set_inf(a); }
};
struct G2Ops {
    static constexpr int W = 32;
    typedef Fq2 F; typedef Acc29G2 Acc;
    struct Pt { F2x29 x, y; };
    __device__ static __forceinline__ Fq2 coord(const uint32_t* w) { return Fq2{fq_of(w), fq_of(w + 8)}; }
    __device__ static __forceinline__ Pt enter(const uint32_t* w, bool neg) {
        Pt p; Fq2 X = coord(w), Y = coord(w + 16); if (neg) Y = fp_neg(Y);
        f29g2_enter(p.x, X); f29g2_enter(p.y, Y);               // carried, below 3 p per component
        return p;
    }
    __device__ static __forceinline__ void set(Acc& a, const Pt& p) {
        a.X = p.x; a.Y = p.y;
#pragma unroll
        for (int k = 0; k < 9; k++) { a.ZZ.c0[k] = a.ZZZ.c0[k] = F29K<FqParams>::one.l[k]; a.ZZ.c1[k] = a.ZZZ.c1[k] = 0; }
    }
    __device__ static __forceinline__ bool madd(Acc& a, const Pt& p, bool& same_y) { return f29g2_madd_lean(a, p.x, p.y, same_y); }
    // f29g2_pt_dbl returns X, Y below 3 p and ZZ, ZZZ below 2.6 p, carried: inside what f29g2_madd takes (its D24 dominates carried values below 5.29 p), and
    // f29g2_madd's results are tame, which is what f29g2_pt_dbl takes
    __device__ static __forceinline__ void dbl(Acc& a) { Acc r; f29g2_pt_dbl(r, a); a = r; }
    __device__ static __forceinline__ XYZZ<Fq2> leave(const Acc& a) { return f29g2_pt_to_xyzz(a); }
    __device__ static __forceinline__ Acc from_xyzz(const XYZZ<Fq2>& p) { return f29g2_pt_from_xyzz(p); }
    __device__ static __forceinline__ void add(Acc& r, const Acc& a, const Acc& b) { f29g2_pt_add(r, a, b); }
    __device__ static __forceinline__ void pt_dbl(Acc& r, const Acc& a) { f29g2_pt_dbl(r, a); }
    __device__ static __forceinline__ bool is_inf(const Acc& a) { return f29g2_pt_is_inf(a); }
    __device__ static __forceinline__ void set_inf(Acc& a) { f29g2_pt_set_inf(a); }
};

// field -> group, for host code that is generic in F: the operations its kernels are instantiated with, and the words its messages need
template <class F> struct GroupOf;
template <> struct GroupOf<Fq> { typedef G1Ops Ops; static constexpr bool g2 = false; static constexpr const char *curve = "curve", *lagrange_dev = "zkc_g1_lagrange_dev"; };
template <> struct GroupOf<Fq2> { typedef G2Ops Ops; static constexpr bool g2 = true; static constexpr const char *curve = "twist", *lagrange_dev = "zkc_g2_lagrange_dev"; };

// ---- the check of a point read from a file, w = its G::W Montgomery words (all zero is infinity and is not brought here): every coordinate < q, which is a test of the
// raw words, and y^2 = x^3 + b (G1: 3; G2: the twist's 3 / (9 + u), computed on the host) ----
template <class G> __device__ __forceinline__ bool coords_below_q(const uint32_t* w) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < G::W; c += 8) ok = ok && fp_std_lt_p<FqParams>(w + c);
    return ok;
}
template <class G> __device__ __forceinline__ bool on_curve(const uint32_t* w, const typename G::F& b) {
    const typename G::F X = G::coord(w), Y = G::coord(w + G::W / 2);
    return fp_sqr(Y) == fp_sqr(X) * X + b;
}

// acc (inf: at infinity) += p, every case handled: see the head of the file
template <class G> __device__ __forceinline__ void add_point(typename G::Acc& acc, bool& inf, const typename G::Pt& p) {
    if (inf) { G::set(acc, p); inf = false; return; }
    bool same_y = false;
    if (!G::madd(acc, p, same_y)) {
        if (same_y) G::dbl(acc);                 // acc holds p itself
        else inf = true;                         // acc holds -p
    }
}

}  // namespace zkc
