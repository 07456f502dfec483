// zkc_kernels.h -- the one declaration of every kernel that is launched from a file other than the one that defines it (product code).
//
// The kernels have C linkage, so the parameter list is not part of the symbol: a launch through a declaration that disagrees with the definition in another .hip file links
// and then packs the wrong bytes into the kernel arguments.  Hence the launching files AND the defining file include this header: C++ allows one function of a given name with
// C linkage, so a definition that disagrees with it fails to compile ("conflicting types").  No .hip file declares a kernel by hand (tests/test_kernel_decls_cpu.py); a kernel
// used only inside its own file is not listed.  Needs only zkc_device.h and zkc_field.h: no host-side header reaches the kernel files through it.
#pragma once
#include "zkc_field.h"
#include "zkc_device.h"

namespace zkc {

// ---- zkc_ntt.hip (launched from zkc_prove.hip) ----
extern "C" __global__ void zkc_wtns_mont(const Fr* wtns_std, size_t wtns_stride, Fr* wm, size_t wm_stride, uint32_t nv);
extern "C" __global__ void zkc_matvec_jds(const uint32_t* perm, const uint32_t* rowlen, const uint32_t* jdptr, const uint32_t* col, const Fr* val, const Fr* wtns_std,
                                          size_t wtns_stride, Fr* abc, int n, uint32_t nlong, const Fr* wm_all, size_t wm_stride);
extern "C" __global__ void zkc_pointwise_mul(Fr* abc, int n);
extern "C" __global__ void zkc_join_abc(const Fr* abc, uint32_t* p_std, int n);

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

}  // namespace zkc
