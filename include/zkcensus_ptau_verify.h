/* zkcensus_ptau_verify.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): is a powers-of-tau file the powers of ONE tau?
 *
 * ---- f7: the point checks of `snarkjs powersoftau verify` (circuit/circuit-compiler.sh:67 and :73), without the contribution transcript of section 7.
 * zkc_setup_from_ptau (zkcensus_ptau.h) reads only the Lagrange sections 12 .. 15 and zkc_ptau_check_prepared (zkcensus_ptau_prepare.h) ties them to the monomial
 * sections 2 .. 5; neither asks whether sections 2 .. 5 are tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1 for one tau, one alpha and one beta.  A file whose
 * section 2 is (G, any points on the curve ..), prepared from that, passes both.  This call closes that: with N = 2^power, T = section 2 (2N - 1 points), U = section
 * 3, A = section 4, B = section 5 (N points each), beta2 = section 6 and one vector of 128-bit weights r_0 .. r_(2N-3), drawn AFTER the file is fixed, the checks are,
 * in this order (the first failure is the one reported):
 *   ZKC_PTAU_CHECK_POINT         every point has coordinates < q, is on its curve and is not infinity (tau, alpha, beta are not zero); the smallest index is named
 *   ZKC_PTAU_CHECK_G2_SUBGROUP   every point of section 3, and beta2, is in the order-r subgroup of the twist (the pairings cannot see a cofactor component)
 *   ZKC_PTAU_CHECK_GENERATORS    T_0 is the G1 generator and U_0 the G2 generator
 *   ZKC_PTAU_CHECK_TAU_G1_G2     sameRatio(G1, T_1; G2, U_1)
 *   ZKC_PTAU_CHECK_TAU_G1        R1 = sum_(i < 2N-2) r_i T_i, R2 = sum r_i T_(i+1): sameRatio(R1, R2; G2, U_1)
 *   ZKC_PTAU_CHECK_TAU_G2        S1 = sum_(i < N-1) r_i U_i, S2 = sum r_i U_(i+1): sameRatio(G1, T_1; S1, S2)
 *   ZKC_PTAU_CHECK_ALPHA_TAU_G1, ZKC_PTAU_CHECK_BETA_TAU_G1   as TAU_G1, over A and over B with N - 1 terms
 *   ZKC_PTAU_CHECK_BETA_G1_G2    sameRatio(G1, B_0; G2, beta2)
 * A sum at infinity fails its check.  The six pairings run on the host; the sums are the work: millions of 128-bit weights times points, on the GPU.  Section 7 (the
 * contribution records: proofs of knowledge, the hash chain, the beacon) is not read, and like the layout itself (zkcensus_ptau.h) the checks are implemented to the
 * ceremony's description and have not been run on a snarkjs-written file.
 *
 * zkc_g1_wsum_pair_dev / zkc_g2_wsum_pair_dev: the hot path on its own, over device buffers: out_lo = sum_(i < n-1) w_i P_i and out_hi = sum_(i < n-1) w_i P_(i+1) for
 *                        the n >= 2 affine points at d_points, laid out as zkc_g1_lagrange_dev takes them (n x 64 B, G2: n x 128 B, all zero = infinity; mont: the
 *                        coordinates are in Montgomery form), and the n - 1 weights at d_weights16, 16 B little endian each, any value.  The outputs are affine,
 *                        standard form, in HOST memory (64 B, G2: 128 B), all zero = infinity.  One lane per segment of 16 consecutive terms walks the 128 weight
 *                        bits from the top: one doubling of its accumulator per bit, then a mixed addition of each point of the segment whose weight has that bit --
 *                        the doubling chain is shared by the segment, not paid per point, and no array of n products is written.  Every exceptional addition is
 *                        handled, on the whole twist in G2.  Lock, stream and synchronisation as zkc_g1_lagrange_dev; ZKC_ERR_BAD_ARG for a NULL pointer or n < 2,
 *                        ZKC_ERR_FORMAT for a coordinate >= q or a point off its curve (zkc_last_error names the smallest such index).
 * zkc_ptau_verify      : 1 valid; 0 not: *check = ZKC_PTAU_CHECK_*, *section / *index = the point to blame where one is (POINT, G2_SUBGROUP, GENERATORS; TAU_G1_G2: 3, 1;
 *                        BETA_G1_G2: 6, 0; otherwise the section the sums ran over and 0), err names the check, e.g. "ptau: section 2 is not the powers of one tau: sameRatio(R1, R2; G2, tauG2[1])
 *                        fails"; < 0 = -ZKC_ERR_* for a file that does not parse (zkc_ptau_check_prepared's conventions; check, section, index, err may be NULL).
 *                        Prepared and unprepared files alike: sections 2 .. 6 only are read, in chunks of 2^22 terms, neighbouring chunks sharing one point, the
 *                        chunks' sums added on the host: the device holds one chunk, never a section.  ctx = NULL does the same work on at most 16 host threads and
 *                        gives the same verdict and the same sums.  seed32 follows zkc_verify_batch's rule: NULL = weights from the OS (what a verifier wants), 32
 *                        bytes = reproducible (tests).  The weights of a call take 32 B of host memory per term while they are drawn, 16 B afterwards.
 * zkc_ptau_verify_stats: milliseconds of the calling thread's last zkc_ptau_verify: ms[0] read, [1] upload and point checks, [2] G2 membership, [3] the sums in G1,
 *                        [4] in G2, [5] pairings.  ctx = NULL: [1] is the checks alone.
 *
 * Hook for the tests and the measurement tool, not a product call (the zkc_debug_* convention of zkcensus.h):
 * zkc_debug_ptau_verify: zkc_ptau_verify with the caller's weights (n_weights = 2N - 2 of 16 B; NULL is ZKC_ERR_BAD_ARG) and chunks of chunk_terms terms (0: the
 *                        default); sums_out (640 B, may be NULL) = R1 R2 | S1 S2 | the A pair | the B pair in standard form, all zero where a sum is infinity or
 *                        was not reached (a POINT or G2_SUBGROUP failure ends the sums).  Returns as zkc_ptau_verify. ---- */
#ifndef ZKCENSUS_PTAU_VERIFY_H
#define ZKCENSUS_PTAU_VERIFY_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
    ZKC_PTAU_CHECK_NONE = 0, ZKC_PTAU_CHECK_POINT = 1, ZKC_PTAU_CHECK_G2_SUBGROUP = 2, ZKC_PTAU_CHECK_GENERATORS = 3, ZKC_PTAU_CHECK_TAU_G1_G2 = 4, ZKC_PTAU_CHECK_TAU_G1 = 5,
    ZKC_PTAU_CHECK_TAU_G2 = 6, ZKC_PTAU_CHECK_ALPHA_TAU_G1 = 7, ZKC_PTAU_CHECK_BETA_TAU_G1 = 8, ZKC_PTAU_CHECK_BETA_G1_G2 = 9
};

int zkc_g1_wsum_pair_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, int mont, const void* d_weights16, uint8_t out_lo[64], uint8_t out_hi[64]);
int zkc_g2_wsum_pair_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, int mont, const void* d_weights16, uint8_t out_lo[128], uint8_t out_hi[128]);

int zkc_ptau_verify(zkc_ctx* ctx, const char* ptau_path, const uint8_t* seed32, uint32_t* check, uint32_t* section, uint64_t* index, char* err, size_t errlen);
int zkc_ptau_verify_stats(double ms[6]);

/* test hook */
int zkc_debug_ptau_verify(zkc_ctx* ctx, const char* ptau_path, const uint8_t* weights16, uint64_t n_weights, uint32_t chunk_terms, uint8_t* sums_out, uint32_t* check,
                          uint32_t* section, uint64_t* index, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
