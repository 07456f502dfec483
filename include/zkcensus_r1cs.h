/* zkcensus_r1cs.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): witnesses checked against a constraint system on the GPU.
 *
 * ---- f5: `snarkjs wtns check <circuit.r1cs> <witness.wtns>` / snarkjs.wtns.check, for batches.  The prover turns ANY nWires x 32 bytes into 256 well-formed proof
 * bytes; a witness that violates a constraint is found out only when the proof fails to verify, and nothing says which constraint broke.  A .zkey carries the A and B
 * matrices only, so the check needs the .r1cs: zkc_r1cs_load parses an iden3 .r1cs image (host memory, any section order, unknown sections skipped) and keeps A, B and C
 * resident on ctx's device; zkc_r1cs_check holds B witnesses against all of its constraints in one pass.
 * Conventions are zkcensus.h's: 32-byte little-endian words in standard form, 0 or a ZKC_ERR_* code, text in zkc_last_error(ctx) (of the ctx the system was loaded on).
 *
 * zkc_r1cs_header_info : (nWires, nPublic = outputs + public inputs, nConstraints) from the image alone; host only, nothing is loaded, no context.  Any out pointer may be
 *                        NULL.  ZKC_ERR_FORMAT for an image whose header the reader refuses, ZKC_ERR_BAD_ARG for r1cs == NULL.
 * zkc_r1cs_load        : ZKC_ERR_BAD_ARG: ctx, r1cs or out NULL, or a system beyond the limits nWires < 2^30 and nConstraints < 2^31 (two bits of a wire word mark unit
 *                        coefficients; a verdict is a non-negative int64 read from a 32-bit device word).  ZKC_ERR_FORMAT with the reader's text: bad magic or section
 *                        table, header section shorter than 64 bytes, field size other than 32, a prime other than BN254's r, nPublic >= nWires, constraints that run
 *                        past the image, a wire index >= nWires.  A coefficient >= r means its value mod r; a wire that occurs twice in one linear combination
 *                        contributes the sum of its coefficients.  The image is not referenced after the call.  Several systems may be resident on one context, next to
 *                        proving keys.
 * zkc_r1cs_free        : releases the device memory; NULL is ignored.
 * zkc_r1cs_info        : the three header figures of a resident system (any out pointer may be NULL).
 * zkc_r1cs_check       : wtns = B contiguous witnesses of nWitness x 32 B in host memory, the layout zkc_witness writes.  first_bad (host, B entries) receives per witness
 *                          ZKC_R1CS_NOT_ONE    wire 0 is not 1;
 *                          ZKC_R1CS_WIRE_RANGE some wire is >= r;
 *                          ZKC_R1CS_SATISFIED  <A_k, w> * <B_k, w> == <C_k, w> (mod r) for every constraint k;
 *                          otherwise the LOWEST k, in the order of the file, whose equation fails.
 *                        NOT_ONE wins over WIRE_RANGE, and both are decided before any constraint is looked at.  n_bad (host, B entries, may be NULL) receives the number
 *                        of violated constraints; 0 whenever first_bad is negative.  The batch is walked in chunks of a bounded number of witnesses (device work space of at
 *                        most ~256 MB whatever B is; a single witness larger than that takes what it takes).
 * zkc_r1cs_check_dev   : the same on a device buffer (hipMalloc'ed or a torch tensor), the layout zkc_witness_dev writes and zkc_prove_batch_dev reads; the buffer is read
 *                        only.  first_bad and n_bad are still host arrays.
 *                        Both return ZKC_OK when the check ran, whatever the verdicts; ZKC_ERR_BAD_ARG (before any device work): cs, the witnesses or first_bad NULL,
 *                        B <= 0, nWitness != nWires.  Both take the context's lock, run on zkc_ctx_stream and have synchronised with it when they return.
 * zkc_r1cs_check_stats : ms of the context's last zkc_r1cs_load, zkc_r1cs_check or zkc_r1cs_check_dev: ms[0] host (load: parsing and laying the matrices out; check:
 *                        gathering the verdicts), ms[1] host-to-device copies, ms[2] kernels.  ZKC_ERR_BAD_ARG for a NULL argument. ---- */
#ifndef ZKCENSUS_R1CS_H
#define ZKCENSUS_R1CS_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
    ZKC_R1CS_SATISFIED = -1,
    ZKC_R1CS_WIRE_RANGE = -2,
    ZKC_R1CS_NOT_ONE = -3
};
typedef struct zkc_r1cs zkc_r1cs;
int  zkc_r1cs_header_info(const void* r1cs, size_t len, uint32_t* nWires, uint32_t* nPublic, uint32_t* nConstraints);
int  zkc_r1cs_load(zkc_ctx* ctx, const void* r1cs, size_t len, zkc_r1cs** out);
void zkc_r1cs_free(zkc_r1cs* cs);
int  zkc_r1cs_info(const zkc_r1cs* cs, uint32_t* nWires, uint32_t* nPublic, uint32_t* nConstraints);
int  zkc_r1cs_check(zkc_r1cs* cs, const void* wtns, uint32_t nWitness, int B, int64_t* first_bad, uint32_t* n_bad);
int  zkc_r1cs_check_dev(zkc_r1cs* cs, const void* d_wtns, uint32_t nWitness, int B, int64_t* first_bad, uint32_t* n_bad);
int  zkc_r1cs_check_stats(zkc_ctx* ctx, double ms[3]);

#ifdef __cplusplus
}
#endif
#endif
