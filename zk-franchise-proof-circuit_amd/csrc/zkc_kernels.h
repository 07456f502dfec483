// zkc_kernels.h -- the one declaration of every kernel that is launched from a file other than the one that defines it (product code).
//
// The kernels have C linkage, so the parameter list is not part of the symbol: a launch through a declaration that disagrees with the definition in another .hip file links
// and then packs the wrong bytes into the kernel arguments.  Hence the launching files AND the defining file include this header: C++ allows one function of a given name with
// C linkage, so a definition that disagrees with it fails to compile ("conflicting types").  No .hip file declares a kernel by hand (tests/test_kernel_decls_cpu.py); a kernel
// used only inside its own file is not listed.  Needs only zkc_device.h, zkc_field.h and zkc_curve.h: no host-side header reaches the kernel files through it.
#pragma once
#include "zkc_field.h"
#include "zkc_curve.h"
#include "zkc_device.h"
#include "zkc_jds.h"

namespace zkc {

// ---- device helpers the sparse-row kernels of zkc_ntt.hip and zkc_r1cs.hip share: 32-byte loads and stores of a field element, and one term of a row whose coefficients
// are stored as val R^2 with +1 / -1 marked in the two top bits of the column word (the term is then the wire's Montgomery form from wm, or its negation) ----
__device__ __forceinline__ Fr ld_fr(const Fr* p) {
    const uint4* d = reinterpret_cast<const uint4*>(p); uint4 a = d[0], b = d[1];
    Fr r; r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w; return r;
}
__device__ __forceinline__ void st_fr(Fr* p, const Fr& r) {
    uint4* d = reinterpret_cast<uint4*>(p);
    d[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]); d[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}
__device__ __forceinline__ Fr mv_term(const Fr* __restrict__ val, const Fr* __restrict__ w, const Fr* __restrict__ wm, uint32_t idx, uint32_t c) {
    if (wm && (c & MV_UNIT)) { const Fr x = ld_fr(wm + (c & MV_COL)); return (c & MV_NEG) ? fp_neg(x) : x; }
    return ld_fr(val + idx) * ld_fr(w + (c & MV_COL));
}

// ---- zkc_ntt.hip (launched from zkc_prove.hip) ----
extern "C" __global__ void zkc_wtns_mont(const Fr* wtns_std, size_t wtns_stride, Fr* wm, size_t wm_stride, uint32_t nv);
extern "C" __global__ void zkc_wtns_mont_list(const Fr* wtns_std, size_t wtns_stride, Fr* wm, size_t wm_stride, const uint32_t* list, uint32_t nlist);
extern "C" __global__ void zkc_abc_fill(const uint4* tmpl, uint4* abc, uint32_t per, uint32_t stride);
extern "C" __global__ void zkc_matvec_jds(const uint32_t* perm, const uint32_t* rowlen, const uint32_t* jdptr, const uint32_t* col, const Fr* val, const Fr* wtns_std,
                                          size_t wtns_stride, Fr* abc, int n, uint32_t nlong, const Fr* wm_all, size_t wm_stride, const uint32_t* list, uint32_t nrows);
extern "C" __global__ void zkc_pointwise_mul(Fr* abc, int n, const uint32_t* list, uint32_t count);
extern "C" __global__ void zkc_join_abc(const Fr* abc, uint32_t* p_std, int n);
extern "C" __global__ void zkc_join_abc_ct(const Fr* abc, const Fr* c_hat, uint32_t* p_std, int n);
extern "C" __global__ void zkc_c_rows_delta(const Fr* abc, const Fr* c_tmpl, uint32_t* p_std, int n, const uint32_t* list, uint32_t count);

// ---- zkc_fold.hip: a call's witnesses against the template and the top-of-tree table, depths off the inputs (launched from zkc_prove.hip) ----
struct TopCheckArgs;      // zkc_prover.h, which both files include
extern "C" __global__ void zkc_fold_check(WitnessLayout L, const uint32_t* wtns, const uint32_t* tmpl, uint32_t* flags, int B, int stride);
extern "C" __global__ void zkc_top_check(TopCheckArgs a, const uint32_t* wtns, uint32_t* flags, int stride, int off);
extern "C" __global__ void zkc_input_depths(const uint32_t* inputs, int nInputs, int n, uint32_t* out);

// ---- zkc_witness.hip: witness generation and batched Poseidon (launched from zkc_api.hip) ----
extern "C" __global__ void zkc_witness_chains(WitnessLayout L, PoseidonTable tab, const uint32_t* inputs, uint32_t* wtns, int32_t* status, int B, int tmpl_mode);
extern "C" __global__ void zkc_witness_chains_wave(WitnessLayout L, PoseidonTable tab, const uint32_t* inputs, uint32_t* wtns, int32_t* status, int B, int tmpl_mode);
extern "C" __global__ void zkc_witness_fill(const uint4* tmpl, uint4* wtns, int nWires, int B);
extern "C" __global__ void zkc_witness_tostd(uint32_t* wtns, size_t nwires_total);
extern "C" __global__ void zkc_poseidon_batch_kernel(PoseidonTable tab, const uint32_t* in, uint32_t* out, int nin, size_t B);

// ---- zkc_witness.hip: census trees and voters' input blocks (launched from zkc_census.hip and zkc_tree.hip) ----
extern "C" __global__ void zkc_census_hash(PoseidonTable tab, int kind, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n);
extern "C" __global__ void zkc_tree_leaves(PoseidonTable tab, const uint32_t* slot, const uint32_t* key, const uint32_t* value, uint32_t count, uint32_t* val);
extern "C" __global__ void zkc_tree_level(PoseidonTable tab, const uint32_t* trip, uint32_t count, uint32_t* val);
extern "C" __global__ void zkc_tree_narrow(PoseidonTable tab, const uint32_t* trip, const uint32_t* off, uint32_t ndepths, uint32_t count, uint32_t* val);
extern "C" __global__ void zkc_census_scatter(const uint32_t* val, const uint2* pairs, size_t count, uint32_t* out);
extern "C" __global__ void zkc_census_scalars(const uint32_t* eid, const uint32_t* nullifier, const uint32_t* avail, const uint32_t* vhash, const uint32_t* sik_root,
                                              const uint32_t* census_root, const uint32_t* address, const uint32_t* password, const uint32_t* signature,
                                              const uint32_t* vweight, size_t n, int nIn, uint32_t* out);

// ---- zkc_witness.hip: proof checking (launched from zkc_smt_check.hip) ----
extern "C" __global__ void zkc_smt_check(PoseidonTable tab, const uint32_t* keys, const uint32_t* values, const uint32_t* roots, uint32_t root_stride, const uint32_t* off,
                                         const uint32_t* sib, uint32_t count, int32_t* status);
extern "C" __global__ void zkc_smt_check_wave(PoseidonTable tab, const uint32_t* keys, const uint32_t* values, const uint32_t* roots, uint32_t root_stride,
                                              const uint32_t* off, const uint32_t* sib, uint32_t count, int32_t* status);
extern "C" __global__ void zkc_smt_check_absent(PoseidonTable tab, const uint32_t* keys, const uint32_t* old_keys, const uint32_t* values, const uint32_t* old0,
                                                const uint32_t* roots, uint32_t root_stride, const uint32_t* off, const uint32_t* sib, uint32_t count, int32_t* status);
extern "C" __global__ void zkc_smt_check_absent_wave(PoseidonTable tab, const uint32_t* keys, const uint32_t* old_keys, const uint32_t* values, const uint32_t* old0,
                                                     const uint32_t* roots, uint32_t root_stride, const uint32_t* off, const uint32_t* sib, uint32_t count, int32_t* status);

// ---- zkc_r1cs.hip: witnesses checked against a resident constraint system ----
extern "C" __global__ void zkc_r1cs_range(const Fr* wtns_std, size_t wtns_stride, uint32_t nWires, uint32_t* flag);
extern "C" __global__ void zkc_r1cs_check_rows(const uint4* rows, const uint32_t* jdptr, const uint32_t* col, const Fr* val, const Fr* wtns_std, size_t wtns_stride,
                                               const Fr* wm_all, size_t wm_stride, uint32_t nCons, uint32_t nlong, uint32_t* first, uint32_t* count, const uint32_t* flag);

}  // namespace zkc
