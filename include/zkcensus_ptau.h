/* zkcensus_ptau.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): Groth16 keys from a powers-of-tau file.
 *
 * ---- f5: `snarkjs groth16 setup circuit.r1cs pot_final.ptau circuit_0000.zkey` and the whole of `snarkjs zkey verify circuit.r1cs pot_final.ptau proving_key.zkey`
 * (circuit/circuit-compiler.sh:99-136).  A key from zkc_setup_from_r1cs* is TEST ONLY because its tau, alpha, beta are drawn from a seed; a key made HERE holds no
 * waste anybody knows, provided the .ptau is a public ceremony's: tau, alpha and beta exist only as the points of that file, and gamma = delta = 1 until the phase-2
 * contributions (zkcensus_phase2.h) replace delta.  Such a key, with at least one honest contribution on top, is NOT test only.
 *
 * The key.  n = 2^cirPower >= nConstraints + nPublic + 1; L, La, Lb, L2 = the Lagrange bases of the size-n domain in sections 12 (tau G1), 14 (alpha tau G1),
 * 15 (beta tau G1), 13 (tau G2) of a PREPARED file (`powersoftau prepare phase2`):
 *   A_s  = sum_c A[c][s] L_c, plus L_(nConstraints + s) for s <= nPublic (snarkjs' extra rows)      B1_s = sum_c B[c][s] L_c      B2_s = sum_c B[c][s] L2_c
 *   K_s  = sum_c (A[c][s] Lb_c + B[c][s] La_c + C[c][s] L_c), the extra rows included through Lb; IC = K_0 .. K_nPublic, section 8 = the rest
 *   H_i  = point 2 i + 1 of section 12's size-2n basis
 *   alpha1 = alphaTauG1[0], beta1 = betaTauG1[0], beta2 = betaG2, gamma2 = delta2 = the G2 generator, delta1 = the G1 generator
 * which is zkc_setup_from_r1cs's key at gamma = delta = 1.  The sums are a sparse matrix times a vector of POINTS: on the GPU, a scale pass (one lane per coefficient
 * that is not +-1), an accumulation pass (one lane per 32 terms of a wire's row) and reduction passes (32 partial sums per lane); with ctx = NULL, on host threads.
 *
 * The file is not trusted: every point read is checked for coordinates < q and for being on its curve, and before anything is written:
 *   sum_c L_c = G1, sum_c L2_c = G2, sum_c La_c = alpha1, sum_c Lb_c = beta1 (the Lagrange basis is a partition of unity: a wrong block, offset or byte order fails
 *   here), and sameRatio(G1, beta1; G2, beta2).
 * That ties the key to the Lagrange sections; zkc_ptau_check_prepared (zkcensus_ptau_prepare.h) ties those to the monomial sections 2 .. 5, and zkc_ptau_verify
 * (zkcensus_ptau_verify.h) checks that the monomial sections are the powers of one tau, alpha, beta: the three together are what "not trusted" means for a downloaded file.
 * Only the ranges the circuit needs are read (the section table first, then pread at 64-bit offsets): a 2^28 file serves a 2^17 circuit.
 *
 * Section 10 of the key written opens with csHash = BLAKE2b-512 over, in this order,
 *   U(alpha1) U(beta1) U2(beta2) U2(gamma2) U(delta1) U2(delta2), then for each of IC, H, C (section 8), A, B1, B2: the count as u32 BIG endian and the points,
 * U / U2 being the uncompressed forms of zkcensus_phase2.h (big-endian standard-form x || y, G2 components c1 before c0, infinity = zeros with bit 0x40 of the first
 * byte set).  INTEROPERABILITY LIMIT, on top of zkcensus_phase2.h's: this is NOT snarkjs' csHash, which hashes H in bellman's monomial form that cannot be restated
 * here; like the proof of knowledge it keeps a transcript made here apart from one made by snarkjs, and unlike the 64 zero bytes of a seeded key it binds a transcript
 * to its circuit.  The layout of the .ptau is restated from the format's description and has not been read from a snarkjs-written file.
 *
 * zkc_setup_from_ptau  : the key of r1cs_path from ptau_path into zkey_path and (unless NULL) vkey_json_path.  ctx = NULL: the sums run on host threads and no GPU is
 *                        touched; the two paths write the same bytes.  Return codes and error conventions are zkc_setup_from_r1cs_dev's: ZKC_ERR_BAD_ARG for a NULL
 *                        path; ZKC_ERR_FORMAT (text in err) for an unreadable or malformed .r1cs or .ptau -- bad magic or version, a section table that runs past
 *                        the file, q != BN254's, a section whose length does not match `power`, an unprepared file, power below the circuit's --, for a point
 *                        with a coordinate >= q or off its curve (the text names the section and the point's index in it), for a failed sanity check, and for an
 *                        unwritable output; ZKC_ERR_HIP when the device fails.  Nothing is written unless every check has passed.
 * zkc_zkey_verify_circuit: `snarkjs zkey verify` in full: derives the initial key of (r1cs, ptau) into memory on ctx's GPU and hands it to the checks of
 *                        zkc_zkey_verify_contributions with `final`.  1 valid, 0 invalid (err names the first failing check: a key of another circuit or another
 *                        .ptau fails check (a)), < 0 = -ZKC_ERR_*.  seed32 and *n_new as there.
 * zkc_setup_ptau_stats : milliseconds of the calling thread's last zkc_setup_from_ptau (or the derivation inside zkc_zkey_verify_circuit): ms[0] read and parse the
 *                        .r1cs and the .ptau ranges, [1] transpose to rows by wire and classify the coefficients, [2] upload, [3] the scale pass (to affine included),
 *                        [4] accumulation and reduction (to affine and download included), [5] checks, hash and write.  ctx = NULL: [2] = 0, [3] and [4] the host threads'.
 *
 * Hook for the tests, not a product call (the zkc_debug_* convention of zkcensus.h):
 * zkc_debug_setup_from_waste: zkc_setup_from_r1cs with tau, alpha, beta, gamma, delta given (32 B little endian, standard form, in [1, r)) instead of drawn from a
 *                        seed.  Host only. ---- */
#ifndef ZKCENSUS_PTAU_H
#define ZKCENSUS_PTAU_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_setup_from_ptau(zkc_ctx* ctx, const char* r1cs_path, const char* ptau_path, const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen);
int zkc_zkey_verify_circuit(zkc_ctx* ctx, const char* r1cs_path, const char* ptau_path, const void* final_, size_t final_len, const uint8_t* seed32, uint32_t* n_new,
                            char* err, size_t errlen);
int zkc_setup_ptau_stats(double ms[6]);

/* test hook */
int zkc_debug_setup_from_waste(const char* r1cs_path, const uint8_t tau[32], const uint8_t alpha[32], const uint8_t beta[32], const uint8_t gamma[32],
                               const uint8_t delta[32], const char* zkey_path, const char* vkey_json_path, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
