/* zkcensus_phase2.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): the phase-2 ceremony of a Groth16 key on the GPU.
 *
 * ---- f3: `snarkjs zkey contribute` and the ceremony part of `snarkjs zkey verify` (circuit/circuit-compiler.sh:112-131 runs three contributions, a beacon and a
 * verify after `groth16 setup`).  A contribution with secret d multiplies delta1 and delta2 by d and every point of sections 8 (C) and 9 (H) by 1 / d: many bases, ONE
 * scalar, the shape zkc_g1_scale_dev computes -- one lane per point, every lane of a wave on the same signed-digit addition chain.  It appends a record to section 10,
 * the ceremony log: csHash(64) nContributions(u32), then per contribution deltaAfter(G1) g1_s(G1) g1_sx(G1) g2_spx(G2) transcript(64) type(u32) paramsLen(u32) params
 * (items 0x01 len name | 0x02 iterExp | 0x03 len beaconHash).  Hashes are BLAKE2b-512; a point enters a hash as big-endian standard-form x || y (G2: c1 before c0;
 * infinity: zeros with bit 0x40 of the first byte set).  pubkey_j = U(deltaAfter) U(g1_s) U(g1_sx) U(g2_spx) transcript_j;
 * transcript_k = H(csHash, pubkey_0 .. pubkey_(k-1), U(g1_s_k), U(g1_sx_k)); the contribution hash is H(csHash, pubkey_0 .. pubkey_k).
 *
 * INTEROPERABILITY LIMIT.  The key material a contribution writes (delta1, delta2, sections 8 and 9) and the record layout are snarkjs'.  The proof of knowledge is
 * not: its G2 challenge is this library's own hash to G2 (SHA-256 try-and-increment), because snarkjs derives it from a ChaCha stream that cannot
 * be restated without its source.  snarkjs' `zkey verify` does not accept the proof of knowledge of a contribution made here, and zkc_zkey_verify_contributions does
 * not accept one made by snarkjs.  Beacon records (type 1) are parsed and carried over byte for byte, never created, and fail verification with a reason that says so.
 * A key from zkc_setup_from_r1cs* stays TEST ONLY after any number of contributions: with tau, alpha, beta known, (1 / delta) G falls out of any C point.  A key from
 * zkc_setup_from_ptau (zkcensus_ptau.h) over a public powers-of-tau file, with at least one honest contribution on top, is not.
 *
 * The conventions are zkcensus.h's: 0 on success and a ZKC_ERR_* code otherwise, the text in zkc_last_error(ctx) or in err.
 * zkc_g1_scale_dev     : d_out[i] = k * d_points[i] for n points on the device (n x 64 B affine; all zero = infinity and gives infinity) and ONE scalar k (32 B
 *                        little-endian, standard form).  mont != 0: coordinates are in Montgomery form, as a .zkey stores them, on both sides; 0: standard form on both.
 *                        d_out may equal d_points.  ZKC_ERR_BAD_ARG: a NULL pointer, n = 0, k >= r.  k = 0 gives n points at infinity.  ZKC_ERR_FORMAT: a coordinate
 *                        >= q or a point off y^2 = x^3 + 3; the text names the smallest such index and d_out is not written.  It takes the context's lock, launches
 *                        on zkc_ctx_stream and has synchronised when it returns, as zkc_g1_fixed_mul_dev does.
 * zkc_blake2b512       : BLAKE2b-512, unkeyed (RFC 7693).  Host only.
 * zkc_zkey_contributions: section 10 of a .zkey image.  Host only, nothing is loaded.  csHash (64 B, may be NULL), *n = the number of records, and the raw records,
 *                        back to back as the file holds them: *records_len in = room in records_out, out = their size (records_out NULL: the size only;
 *                        too little room: ZKC_ERR_SHORT_BUFFER).  ZKC_ERR_FORMAT with the text in err: no section 10, a count that does not fit the section, a
 *                        truncated record, paramsLen beyond the section, an unknown tag or type, bytes after the last record.
 * zkc_zkey_contribute  : one type-0 contribution with secret delta (32 B standard form; NULL: drawn with zkc_random_scalars; 0 or >= r: ZKC_ERR_BAD_ARG).  The output is
 *                        the input image with delta1 and delta2 multiplied by delta, sections 8 and 9 multiplied by 1 / delta on the GPU and one record appended to
 *                        section 10; every other byte, section order included, is unchanged.  name: NUL-terminated, cut at 64 bytes, may be NULL.  out NULL: *out_len =
 *                        the size of the output; else *out_len in = room (too little: ZKC_ERR_SHORT_BUFFER, the size written back), out = bytes written.  hash (64 B,
 *                        may be NULL) = the contribution hash.
 * zkc_zkey_verify_contributions: is `final` an honest chain of contributions on top of `init`?  1 valid, 0 invalid (err names the first failing check), < 0 =
 *                        -ZKC_ERR_*, the convention of zkc_verify_batch.  *n_new (may be NULL) = records of final beyond init's.  seed32: NULL = the weights of check
 *                        (e) come from zkc_random_scalars; given = from the generator the batch verifier seeds the same way (reproducible: for tests).  Checks, in order:
 *                        (a) both images parse; nVars, nPublic, domainSize, alpha1, beta1, beta2, gamma2 equal; sections 3-7 byte-equal; csHash equal (in this order)
 *                        (b) init's records are a byte-equal prefix of final's
 *                        (c) from delta = init's delta1, for each new record: type 0 (a beacon fails here), points on their curves and g2_spx in G2, the stored
 *                            transcript equals the recomputed one, sameRatio(g1_s, g1_sx; g2_sp, g2_spx), sameRatio(delta, deltaAfter; g2_sp, g2_spx), delta = deltaAfter
 *                            (sameRatio(a, b; c, d): e(a, d) = e(b, c), host pairing; g2_sp = the challenge of the transcript)
 *                        (d) delta = final's delta1, and sameRatio(G1, delta1; G2, delta2)
 *                        (e) with random weights rho, one set per section: e(sum rho_i C_init,i, delta2_init) = e(sum rho_i C_final,i, delta2_final), the same
 *                            for H; the four sums are zkc_msm_g1_load_dev / zkc_msm_g1_dev on ctx's GPU, which also reject points off the curve
 *                        (f) no new record and everything equal is valid.
 * zkc_phase2_stats     : milliseconds of the calling thread's last contribute: ms[0] parse and host points, [1] upload, [2] scale kernel, [3] to affine, [4] download,
 *                        [5] hashes and output image; of its last verify: ms[6] table loads (upload, conversion, window tables), [7] the four MSMs, [8] pairings.
 *
 * Hooks for the tests and the measurement tool, not product calls (the zkc_debug_* convention of zkcensus.h):
 * zkc_debug_phase2_challenge_g2: the G2 challenge of a 64-byte transcript, 128 B standard form (tests/test_phase2_cpu.py).
 * zkc_debug_phase2_host_scale: what zkc_g1_scale_dev computes, on `threads` host threads (1..256) with the variable-base multiplication of csrc/zkc_curve.h: n points
 *                        in host memory, Montgomery coordinates on both sides, taken as on the curve; *ms (may be NULL) = wall time.  The CPU side of the comparison
 *                        tools/phase2_bench.py records. ---- */
#ifndef ZKCENSUS_PHASE2_H
#define ZKCENSUS_PHASE2_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int  zkc_g1_scale_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const uint8_t k[32], int mont, void* d_out);
void zkc_blake2b512(const void* data, size_t len, uint8_t out[64]);
int  zkc_zkey_contributions(const void* zkey, size_t len, uint8_t csHash[64], uint32_t* n, void* records_out, size_t* records_len, char* err, size_t errlen);
int  zkc_zkey_contribute(zkc_ctx* ctx, const void* zkey, size_t len, const uint8_t delta[32], const char* name, void* out, size_t* out_len, uint8_t hash[64]);
int  zkc_zkey_verify_contributions(zkc_ctx* ctx, const void* init, size_t init_len, const void* final_, size_t final_len, const uint8_t* seed32, uint32_t* n_new,
                                   char* err, size_t errlen);
int  zkc_phase2_stats(double ms[9]);

/* test and measurement hooks */
int  zkc_debug_phase2_challenge_g2(const uint8_t transcript[64], uint8_t out[128]);
int  zkc_debug_phase2_host_scale(const void* points, uint32_t n, const uint8_t k[32], int threads, void* out, double* ms);

#ifdef __cplusplus
}
#endif
#endif
