/* zkcensus_setup.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): fixed-base batch products in G1 and G2 on the GPU, and the
 * test-only key generator built on them.
 *
 * ---- f3: Groth16 keys generated on the GPU.  A key is almost nothing but fixed-base products -- 3 nWires + domainSize + 3 multiples of the G1 generator and nWires + 3
 * of the G2 generator (zkc_setup_from_r1cs, zkcensus.h) -- and with a window table T[j][d - 1] = d 2^(w j) P a product k P is one mixed addition per non-zero w-bit
 * digit of k: no doubling, no sorting, one scalar per lane.  The conventions are zkcensus.h's: 32-byte little-endian words in standard form, affine points
 * (G1 = x||y, 64 B; G2 = x.c0||x.c1||y.c0||y.c1, 128 B; all-zero = infinity), 0 on success and a ZKC_ERR_* code otherwise with the text in zkc_last_error(ctx).
 * zkc_g1_fixed_mul_dev : d_out[i] = k_i * base for n scalars on the device (n x 32 B) into n x 64 B on the device.  The conventions of zkc_g1_mul_batch_dev: it takes
 *                        the context's lock, launches on zkc_ctx_stream and has synchronised when it returns; ZKC_ERR_BAD_ARG for a NULL pointer, n = 0 and a base
 *                        coordinate >= q -- and, here, for a base that is not on y^2 = x^3 + 3 (no subgroup check; the all-zero base is infinity and gives n
 *                        points at infinity).  A scalar 0 gives the all-zero point.  Every scalar must be BELOW r: the kernel adds with the incomplete mixed
 *                        addition, which the partial sums of a scalar below r never take to its exceptional case; for a scalar >= r the output is undefined
 *                        (nothing is read or written out of bounds).  The same contract zkc_prove_dev sets for witnesses.  The table is built on the host and
 *                        uploaded per call (tens of milliseconds): the entry point is meant for batches.
 * zkc_g2_fixed_mul_dev : the same in G2: base 128 B, checked to be on the twist y^2 = x^3 + 3 / (9 + u); d_out n x 128 B.
 * zkc_fixed_mul_window : the window width w (8): 256 / w windows of 2^w - 1 table rows.
 * zkc_setup_from_r1cs_dev: zkc_setup_from_r1cs with the points computed on ctx's GPU.  Same arguments after ctx, same .zkey and verification_key.json byte for byte
 *                        for the same .r1cs and seed, same return codes and error texts for an unreadable, malformed or truncated .r1cs or an unwritable output
 *                        (ZKC_ERR_FORMAT, text in err); ZKC_ERR_BAD_ARG for ctx = NULL before any file is touched; ZKC_ERR_HIP (text in err and in
 *                        zkc_last_error) when the device fails.  Reading the file and the scalars of the key (linear in the constraint matrix) and writing the
 *                        outputs stay on the host and are shared with zkc_setup_from_r1cs.  TEST ONLY, as that function is: the toxic waste is known (a key nobody holds the
 *                        waste of comes from zkc_setup_from_ptau, zkcensus_ptau.h).
 * zkc_setup_stats      : milliseconds of the calling thread's last zkc_setup_from_r1cs or zkc_setup_from_r1cs_dev: ms[0] read the .r1cs and compute the scalars, ms[1]
 *                        build the two window tables (host; the device path's upload included), ms[2] scalars -> points without the tables (device path: uploads,
 *                        kernels, downloads), ms[3] write the .zkey and the JSON (the pairing e(alpha, beta) included).  A call that failed leaves what it reached. ---- */
#ifndef ZKCENSUS_SETUP_H
#define ZKCENSUS_SETUP_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_g1_fixed_mul_dev(zkc_ctx* ctx, const uint8_t base_std[64], const void* d_scalars, uint32_t n, void* d_out);
int zkc_g2_fixed_mul_dev(zkc_ctx* ctx, const uint8_t base_std[128], const void* d_scalars, uint32_t n, void* d_out);
int zkc_fixed_mul_window(void);
int zkc_setup_from_r1cs_dev(zkc_ctx* ctx, const char* r1cs_path, uint64_t seed, const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen);
int zkc_setup_stats(double ms[4]);

#ifdef __cplusplus
}
#endif
#endif
