// zkc_fixedbase_dev.h -- host-side interface of the device fixed-base batch products (zkc_fixedbase_dev.hip), for the files that build on them (zkc_setup.hip), and of
// the two steps that every file of kernels over the points of a file shares (zkc_phase2.hip, zkc_setup_ptau.hip, zkc_ecntt.hip, zkc_ptau_prepare.hip): the check of the
// points read (points_check_dev) and the way back from XYZZ sums to affine points (fixed_affine).  The kernels themselves are launched only from their own file, so
// zkc_kernels.h does not list them.
#pragma once
#include "zkc_internal.h"
#include "zkc_curve.h"

namespace zkc {

constexpr int FIXED_W = 8;                                          // window width: the host table's (zkc_fixedbase.h), which is uploaded as it is
constexpr int FIXED_NWIN = 256 / FIXED_W;                           // 32 windows
constexpr int FIXED_ROWS = FIXED_NWIN * ((1 << FIXED_W) - 1);       // 8160 table rows: T[j][d - 1] = d 2^(8 j) P, d = 1 .. 255

// The window table of one base, built on the host (FixedBase<F>, 32 x 255 affine points) and uploaded: G1 as 64-byte Montgomery points (522 240 B), G2 in the
// radix-2^29 row format of the G2 MSM (zkc_g2_table29, rows of G2ROW_WORDS words, zkc_f29_g2.h: 240 B per row, 1 958 400 B).  Global memory; both tables stay in the L2 during a launch.
// host_ms (may be NULL): milliseconds of the host build.  Free with hipFree.  The context's lock is held by the caller; `base` is finite and on its curve.
int fixed_table_g1(zkc_ctx* ctx, const G1Affine& base, G1Affine** d_table, double* host_ms);
int fixed_table_g2(zkc_ctx* ctx, const G2Affine& base, uint32_t** d_table29, double* host_ms);

// d_out[i] = k_i * P for n scalars on the device, P given by its table.  scalars_mont: the scalars are Fr elements in Montgomery form (what the setup holds) instead of
// 32-byte standard form; out_mont: coordinates are written in Montgomery form (what a .zkey stores) instead of standard form.  Scalars are below r (see zkcensus_setup.h).
// Launches on ctx->stream, synchronises and frees its work space before it returns.
int fixed_mul_g1(zkc_ctx* ctx, const G1Affine* d_table, const void* d_scalars, bool scalars_mont, uint32_t n, void* d_out, bool out_mont);
int fixed_mul_g2(zkc_ctx* ctx, const uint32_t* d_table29, const void* d_scalars, bool scalars_mont, uint32_t n, void* d_out, bool out_mont);

// The second half of a batch product on its own, for other kernels that leave XYZZ sums (zkc_phase2.hip, zkc_setup_ptau.hip, zkc_ecntt.hip): d_in (n points on the device,
// infinity = ZZ zero) -> d_out (n x 64 B affine, G2: n x 128 B; all zero = infinity; d_out may alias whatever d_in was computed from) through the batched inversion of
// zkc_fixed_affine<F>.  F = Fq or Fq2.  Launches on ctx->stream, synchronises and frees its work space before it returns; the context's lock is held by the caller.
template <class F> int fixed_affine(zkc_ctx* ctx, const XYZZ<F>* d_in, uint32_t n, void* d_out, bool out_mont);

// *bad = the smallest index of a point of d_pts (n affine points on the device, Montgomery words, F = Fq: G1, Fq2: G2) with a coordinate >= q or off its curve, 0xffffffff
// when there is none; all zero is infinity and passes (the device side of host_point_ok, zkc_file_points.h).  Launches on ctx->stream and has synchronised on return; the
// context's lock is held by the caller.
template <class F> int points_check_dev(zkc_ctx* ctx, const void* d_pts, uint32_t n, uint32_t* bad);

}  // namespace zkc
