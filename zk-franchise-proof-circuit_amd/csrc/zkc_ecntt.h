// zkc_ecntt.h -- host-side interface of the transform over points (zkc_ecntt.hip), for the file that builds on it (zkc_ptau_prepare.hip).  The kernels themselves are
// launched only from their own file, so zkc_kernels.h does not list them.
#pragma once
#include "zkc_internal.h"
#include "zkc_curve.h"

namespace zkc {

constexpr uint32_t ECNTT_MAX_LOGN = 28;            // the two-adicity of r - 1: Fr has no root of unity of a higher order (fr_root_of_unity)

// The inverse twiddles w^-j, j < 2^(logn - 1), of the size-2^logn domain as Montgomery-form Fr on the device: the `inv` table of the loaders' twiddle set
// (ntt_twiddle_tables without its limb forms; the forward table is freed again).  A table of a larger domain serves every smaller one by stride.  1 <= logn <=
// ECNTT_MAX_LOGN, anything else is ZKC_ERR_BAD_ARG.  Free with hipFree.
int ecntt_twiddles(zkc_ctx* ctx, uint32_t logn, Fr** d_tw);

// d_out[c] = 1/n sum_i w^(-c i) d_pts[i] for the n = 2^logn affine points at d_pts (F = Fq: G1, Fq2: G2; Montgomery words, all zero = infinity, ALREADY CHECKED:
// points_check_dev, zkc_fixedbase_dev.h), natural order on both sides, affine again (out_mont: Montgomery words).  d_tw: ecntt_twiddles of tw_logn >= logn (may be NULL when
// logn < 2).  d_out may be d_pts.  Launches on ctx->stream, has synchronised and freed its work space on return; the context's lock is held by the caller.  ms (may be NULL):
// += [0] the transform, [1] to affine.
template <class F> int ecntt(zkc_ctx* ctx, const void* d_pts, uint32_t logn, const Fr* d_tw, uint32_t tw_logn, void* d_out, bool out_mont, double* ms);
// ncoord coordinates of 32 B in standard form at d_in -> Montgomery form at d_out, on ctx->stream and not waited for (the engines' mont = 0 inputs: zkc_g1_lagrange_dev,
// zkc_g1_wsum_pair_dev and their G2 forms).  A coordinate >= q is copied as it is, for points_check_dev to find.
int coords_to_mont(zkc_ctx* ctx, const void* d_in, void* d_out, size_t ncoord);
// the device bytes one call needs beside d_pts and d_out
inline size_t ecntt_work_bytes(uint32_t logn, bool g2) { return ((size_t)1 << logn) * (g2 ? sizeof(G2XYZZ) : sizeof(G1XYZZ)) * 2; }

}  // namespace zkc
