/* zkcensus_ptau_contribute.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): the first half of the ceremony, phase 1.
 *
 * ---- f8: `snarkjs powersoftau new` and `powersoftau contribute` (circuit/circuit-compiler.sh:52-65), and the transcript part of `powersoftau verify` (:67, :73) on top
 * of the point checks of zkcensus_ptau_verify.h.  A contribution with secrets tau', alpha', beta' replaces every point of the monomial sections by a multiple of itself:
 *   section 2  T_i -> tau'^i T_i        section 3  U_i -> tau'^i U_i        section 4  A_i -> alpha' tau'^i A_i        section 5  B_i -> beta' tau'^i B_i
 *   section 6  beta2 -> beta' beta2
 * about 4.2 M products in G1 and 1 M in G2 at power 20, each under its own full-width scalar: the batch product the library lacked.
 *
 * zkc_g1_scale_each_dev / zkc_g2_scale_each_dev: that product on its own, over device buffers: d_out[i] = k_i * P_i for the n affine points at d_points (n x 64 B, G2:
 *                        n x 128 B as x.c0 x.c1 y.c0 y.c1; all zero = infinity; mont as for zkc_g1_scale_dev: the coordinates are in Montgomery form on both sides) and
 *                        the n scalars at d_scalars32, 32 B little endian, standard form, any value below r; scalar 0 gives infinity.  d_out may alias d_points.  One
 *                        lane per point: the lane recodes its scalar into 64 signed 4-bit digits, builds the table 1P .. 8P of its point in device work space (8 x 144
 *                        B per G1 lane, 8 x 288 B per G2 lane, freed before the call returns) and walks the digits from the top: four doublings and one complete
 *                        addition per digit, the same for every lane.  Lock, stream and synchronisation as zkc_g1_scale_dev; ZKC_ERR_BAD_ARG for a NULL pointer or
 *                        n = 0; ZKC_ERR_FORMAT for a coordinate >= q, a point off its curve or a scalar >= r (zkc_last_error names the smallest such index), and then
 *                        d_out is not written.
 * zkc_ptau_new         : an unprepared file of `power` (1 .. 27, what zkc_ptau_prepare takes) with sections 1 .. 7 and tau = alpha = beta = 1: every point is its
 *                        group's generator, section 7 holds the count 0.  Host only.  Written under a temporary name and renamed: a failure leaves nothing at path.
 * zkc_ptau_contribute  : dst = src with the contribution of secrets96 = tau' alpha' beta' (32 B each, little endian, standard form; NULL: drawn with
 *                        zkc_random_scalars; any of them 0 or >= r: ZKC_ERR_BAD_ARG) and one more record in section 7.  name: NUL-terminated, cut at 64 bytes, may be
 *                        NULL (as zkc_zkey_contribute treats it).  hash64 (64 B, may be NULL) receives the contribution hash.  Sections 2 .. 6 are read in chunks of
 *                        2^20 points; per chunk the points are checked (coordinates < q, on the curve, not infinity: ZKC_ERR_FORMAT names the section and the smallest
 *                        index), the scalars tau'^(first + lane) [x alpha', x beta'] are made ON THE DEVICE from an uploaded table of tau'^(2^k), and the products are
 *                        written to a temporary file that is renamed into place at the end: the device holds one chunk and its work space, never a section, and a
 *                        failure leaves nothing at dst.  The output has sections 1 .. 7 ONLY, in this order whatever the input's: the Lagrange sections 12 .. 15 of a
 *                        prepared input would be stale and are dropped (prepare again).  Section 1 and the earlier records of section 7 are carried over byte for byte.
 *                        ctx = NULL does the same work on at most 16 host threads and writes the same bytes.  The secrets and everything derived from them are
 *                        cleared before their storage is released, on the host and on the device.  Given secrets give one contribution: the scalars of the proofs of
 *                        knowledge are derived from the secrets and the records so far, so the hash is reproducible.
 * zkc_ptau_contributions: *n = the count of section 7 and, when records_out is given, its records as they lie in the file (*records_len: in, the room; out, the bytes
 *                        needed; ZKC_ERR_SHORT_BUFFER when short).  Host only, the counterpart of zkc_zkey_contributions.  ZKC_ERR_FORMAT for a count that does not fit
 *                        the section, a truncated record, an unknown tag or type, or bytes after the last record.  A file without section 7 has no contribution.
 * zkc_ptau_verify_contributions: 1 valid; 0 invalid, err names the first failing check; < 0 = -ZKC_ERR_*.  The checks, in this order:
 *                          1  both files parse and have the same power
 *                          2  prev's records are a byte-equal prefix of next's (*n_new = the number of records after them)
 *                          3  for each new record, starting from prev's tauG1 = T_1, tauG2 = U_1, alphaG1 = A_0, betaG1 = B_0, betaG2: (3.1) its points are on
 *                             their curves and not infinity, its G2 points in G2; (3.2) the stored transcript is the recomputed one; (3.3) the three proofs of knowledge
 *                             hold, sameRatio(g1_s, g1_sx; g2_sp, g2_spx); (3.4) the three chain steps hold, sameRatio(before, after; g2_sp, g2_spx) for tau, alpha,
 *                             beta; (3.5) tau and beta agree between G1 and G2
 *                          4  the last record's five points are next's T_1, U_1, A_0, B_0, beta2 (no new record: the chain's start is)
 *                          5  zkc_ptau_verify(ctx, next, seed32) holds: the file is the powers of that tau, alpha, beta (its failing check is quoted)
 *                        No new record and equal sections is valid.  prev_path = NULL: the chain starts at the generators, i.e. the check is against a zkc_ptau_new
 *                        file of next's power.  The pairings run on the host; ctx only serves check 5 and may be NULL.  seed32 as for zkc_ptau_verify.
 * zkc_ptau_contribute_stats: milliseconds of the calling thread's last zkc_ptau_contribute: ms[0] read, [1] upload, scalars and (ctx = NULL) point checks, [2] the scale
 *                        kernel in G1 (the point checks are fused into it), [3] in G2, [4] to affine and download, [5] hashes, proofs of knowledge and write.
 *
 * Section 7 as this library writes it.  nContributions(u32), then per contribution
 *     tauG1(G1 64) tauG2(G2 128) alphaG1(G1 64) betaG1(G1 64) betaG2(G2 128)      T_1, U_1, A_0, B_0, beta2 AFTER the contribution
 *     for tau, alpha, beta in this order: g1_s(G1 64) g1_sx(G1 64) g2_spx(G2 128)  g1_sx = x g1_s, g2_spx = x g2_sp for the key's secret x
 *     transcript(64) type(u32 = 0) paramsLen(u32) params: items 0x01 len name[len]
 * points affine, little-endian Montgomery coordinates, as everywhere in the file.  With U() the uncompressed big-endian encoding of zkcensus_phase2.h,
 *     pubkey_j     = U(tauG1) U(tauG2) U(alphaG1) U(betaG1) U(betaG2), then for tau, alpha, beta U(g1_s) U(g1_sx) U(g2_spx), then transcript_j      (1280 bytes)
 *     transcript_k = BLAKE2b-512("zkc-ptau" || power as u32 LE || pubkey_0 .. pubkey_(k-1) || for tau, alpha, beta U(g1_s) U(g1_sx) of record k)
 *     g2_sp of key i (0 tau, 1 alpha, 2 beta) = the hash to G2 of zkcensus_phase2.h (zkc_debug_phase2_challenge_g2) of BLAKE2b-512(transcript_k || i as one byte)
 *     contribution hash = BLAKE2b-512("zkc-ptau" || power || pubkey_0 .. pubkey_k)
 * The interoperability limit is that of phase 2: sections 2 .. 6 are what snarkjs writes for the same tau', alpha', beta'; the record and its proofs of knowledge are
 * this library's own, restated from the ceremony's description.  snarkjs' `powersoftau verify` will not accept this transcript, nor this verifier one made by snarkjs
 * (a snarkjs-written section 7 does not parse here, and zkc_ptau_contribute refuses such an input).  Beacon contributions, `export challenge`, `challenge contribute`
 * and `import response` are not implemented.
 *
 * Hooks for the tests and the measurement tool, not product calls (the zkc_debug_* convention of zkcensus.h):
 * zkc_debug_ptau_contribute: zkc_ptau_contribute with chunks of chunk_points points (0: the default) and the kernel form (0: the shipped windowed form; 1: bit-serial
 *                        double-and-add, the yardstick of tools/ptau_contribute_bench.py).
 * zkc_debug_scale_each_dev: zkc_g1_scale_each_dev (g2 = 0) / zkc_g2_scale_each_dev (g2 = 1) with the kernel form.
 * zkc_debug_scale_each_stats: milliseconds of the calling thread's last scale_each call: ms[0] the scale kernel (point checks included), ms[1] to affine.
 * zkc_debug_scale_each_work_bytes: the device work space one such call allocates beside its arguments.
 * zkc_debug_tau_scalars_dev: the scalars of a chunk of a contribution on their own: d_out[i] = mult * tau^(first + i) for i < n, 32 B little endian, standard form, by the
 *                        power table and the kernel launch a contribution uses (zkc_tau_scalars).  tau32, mult32: 32 B little endian, standard form.  ZKC_ERR_BAD_ARG for a
 *                        NULL pointer, n = 0, tau or mult outside [1, r), or first + n > 2^32: the table holds tau^(2^k) for k < 32.  The table and the work copy of the
 *                        scalars are cleared on the stream before they are released. ---- */
#ifndef ZKCENSUS_PTAU_CONTRIBUTE_H
#define ZKCENSUS_PTAU_CONTRIBUTE_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_g1_scale_each_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out);
int zkc_g2_scale_each_dev(zkc_ctx* ctx, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out);

int zkc_ptau_new(const char* path, uint32_t power, char* err, size_t errlen);
int zkc_ptau_contribute(zkc_ctx* ctx, const char* src_path, const char* dst_path, const uint8_t* secrets96, const char* name, uint8_t* hash64, char* err, size_t errlen);
int zkc_ptau_contributions(const char* path, uint32_t* n, void* records_out, size_t* records_len, char* err, size_t errlen);
int zkc_ptau_verify_contributions(zkc_ctx* ctx, const char* prev_path, const char* next_path, const uint8_t* seed32, uint32_t* n_new, char* err, size_t errlen);
int zkc_ptau_contribute_stats(double ms[6]);

/* test hooks */
int zkc_debug_ptau_contribute(zkc_ctx* ctx, const char* src_path, const char* dst_path, const uint8_t* secrets96, const char* name, uint32_t chunk_points, int form,
                              uint8_t* hash64, char* err, size_t errlen);
int zkc_debug_scale_each_dev(zkc_ctx* ctx, int g2, const void* d_points, uint32_t n, const void* d_scalars32, int mont, void* d_out, int form);
int zkc_debug_scale_each_stats(double ms[2]);
uint64_t zkc_debug_scale_each_work_bytes(int g2, uint32_t n, int form);
int zkc_debug_tau_scalars_dev(zkc_ctx* ctx, const uint8_t* tau32, const uint8_t* mult32, uint64_t first, uint32_t n, void* d_out);

#ifdef __cplusplus
}
#endif
#endif
