/* zkcensus_ptau_prepare.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): a powers-of-tau file prepared for phase 2.
 *
 * ---- f6: `snarkjs powersoftau prepare phase2 pot_beacon.ptau pot_final.ptau` (circuit/circuit-compiler.sh:71), the step before `groth16 setup` (zkcensus_ptau.h),
 * and the check that a prepared file's Lagrange sections ARE the transforms of its monomial sections, which zkc_setup_from_ptau alone cannot tell (it checks that the
 * points it reads are on their curves and that a basis sums to the right point; any vector that sums to zero can be added to a block without tripping that).
 *
 * The computation.  For a block of n = 2^p points M_0 .. M_(n-1) (M_i = tau^i G; alpha or beta folded in for sections 4 and 5) the Lagrange basis is
 *     L_c = 1/n sum_(i<n) w^(-c i) M_i,   c = 0 .. n - 1, natural order on both sides, w = 5^((r - 1) >> 28) squared 28 - p times:
 * an inverse discrete Fourier transform whose elements are curve points.  A prepared file holds it for every p = 0 .. power: section 12 from section 2 (tau G1),
 * 13 from 3 (tau G2), 14 from 4 (alpha tau G1), 15 from 5 (beta tau G1), block p at point offset 2^p - 1; section 12 holds p = power + 1 as well.
 *
 * THE TOP BLOCK.  Section 2 holds 2^(power+1) - 1 points, and the block of size 2N = 2^(power+1) needs 2N: tau^(2N-1) G is not in the file.  What any preparer can
 * produce is the transform of (M_0 .. M_(2N-2), infinity), in the exponent  L'_c = L_c(tau) - w_2N^c tau^(2N-1) / 2N.  zkc_ptau_prepare writes that padded form and
 * zkc_ptau_check_prepared accepts only it: the true basis cannot be verified from the file.  Both give the same proofs -- the prover contracts the odd points of that
 * block with the evaluations of a polynomial of degree <= 2N - 2, and sum_c f(w^c) w^c picks out the coefficient of x^(2N-1), which is 0 -- but the H points of a key whose
 * domain equals the file's power differ, and so do the key's bytes.  Like the layout itself (zkcensus_ptau.h) this is implemented to the format's description and has
 * not been executed against a snarkjs-written file.
 *
 * zkc_g1_lagrange_dev / zkc_g2_lagrange_dev: the transform on its own, over device buffers: d_out[c] = L_c of the n = 2^logn points at d_points.  Points are affine,
 *                        n x 64 B (G2: n x 128 B, x.c0 x.c1 y.c0 y.c1), all zero = infinity; mont: the coordinates are in Montgomery form on both sides, as a .ptau
 *                        stores them.  logn = 0 copies the point; d_out may equal d_points.  The conventions are zkc_g1_scale_dev's: the context's lock is taken, the
 *                        work runs on zkc_ctx_stream, and the call has synchronised on return.  ZKC_ERR_BAD_ARG for a NULL pointer or logn > 28 (Fr has no larger domain); ZKC_ERR_FORMAT for a
 *                        coordinate >= q or a point off its curve (zkc_last_error names the smallest such index; d_out is not written).
 * zkc_ptau_prepare     : out_path = the input's sections as they are and in the input's order (section 7 is copied unread), then sections 12, 13, 14, 15.  ctx = NULL
 *                        runs the same transform on at most 16 host threads and writes the same bytes.  Every input point is checked (coordinates < q, on its curve;
 *                        the text names the section and the index).  ZKC_ERR_BAD_ARG for a NULL path; ZKC_ERR_FORMAT (text in err) for a file that does not parse, that
 *                        already has one of sections 12 .. 15, for a file of power 28 (section 12's last block would be a transform of size 2^29, and Fr has no
 *                        root of unity of order above 2^28: the largest power prepared or checked here is 27; zkc_setup_from_ptau still READS a power-28 file), for a bad point, for a power whose largest block does not fit the device's free memory (blocks are
 *                        processed one at a time: the device holds one monomial section, one block and its work space), and for an unwritable output; ZKC_ERR_HIP
 *                        when the device fails.  The output is written under a temporary name and renamed into place: on any failure nothing is left at out_path.
 * zkc_ptau_check_prepared: recomputes sections 12 .. 15 of a prepared file from its sections 2 .. 5 and compares bytes.  1 valid; 0 not: *section / *index (either may
 *                        be NULL) = the first difference in the order 12, 13, 14, 15 and then by point index in the section, and err says e.g. "ptau: section 14 point
 *                        37 is not the transform of section 4"; < 0 = -ZKC_ERR_* (a file that does not parse, is not prepared or has power 28, a bad monomial point).  ctx = NULL
 *                        does the same work on host threads.
 * zkc_ptau_prepare_stats: milliseconds of the calling thread's last zkc_ptau_prepare or zkc_ptau_check_prepared: ms[0] read, [1] upload and the check of the input
 *                        points, [2] the transforms in G1, [3] in G2, [4] to affine and download, [5] write (check_prepared: read the stored blocks and compare).
 *                        ctx = NULL: [1] is the check alone, [2] and [3] include the conversion to affine, [4] = 0. ---- */
#ifndef ZKCENSUS_PTAU_PREPARE_H
#define ZKCENSUS_PTAU_PREPARE_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_g1_lagrange_dev(zkc_ctx* ctx, const void* d_points, uint32_t logn, int mont, void* d_out);
int zkc_g2_lagrange_dev(zkc_ctx* ctx, const void* d_points, uint32_t logn, int mont, void* d_out);

int zkc_ptau_prepare(zkc_ctx* ctx, const char* in_path, const char* out_path, char* err, size_t errlen);
int zkc_ptau_check_prepared(zkc_ctx* ctx, const char* ptau_path, uint32_t* section, uint64_t* index, char* err, size_t errlen);
int zkc_ptau_prepare_stats(double ms[6]);

#ifdef __cplusplus
}
#endif
#endif
