// zkc_census_host.h -- what the host sides of the census code share (zkc_census.hip, zkc_tree.hip, zkc_smt_check.hip): small helpers over 32-byte words, the layout of
// a voter's circuit-input block, and the two routines behind both the static builder and the resident tree (defined in zkc_census.hip): hashing a tree's inner nodes
// from (node, left, right) triples, and assembling voters' input blocks.  Product code, host only.
#pragma once
#include "zkc_internal.h"      // brings zkc_device.h and zkc_field.h
#include "zkc_host_util.h"     // clk, ms_since
#include <cstring>

namespace zkc {

inline bool below_r(const uint8_t* v) { uint32_t t[8]; memcpy(t, v, 32); return fp_std_lt_p<FrParams>(t); }
inline bool all_below_r(const void* v, size_t count) {
    for (size_t i = 0; i < count; i++) if (!below_r((const uint8_t*)v + 32 * i)) return false;
    return true;
}
inline bool is_zero(const uint8_t* v) { uint64_t w[4]; memcpy(w, v, 32); return (w[0] | w[1] | w[2] | w[3]) == 0; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int key_bit(const uint8_t* key, int d) { return (key[d >> 3] >> (d & 7)) & 1; }          // path bit d of a 32-byte key (LSB first)

// A voter's block of circuit inputs in 32-byte slots, census.circom:51-67 order: the twelve scalars, then the census and the SIK sibling list, nLevels + 1 slots each
// (zkc_circuit_n_inputs(nLevels) slots in all).  zkc_census_scalars and the witness kernels (zkc_witness.hip) read the same order on the device.
struct InputBlock {
    static constexpr size_t kScalars = 12;
    size_t census_sibs, sik_sibs, nIn;
    explicit InputBlock(int nLevels) : census_sibs(kScalars), sik_sibs(kScalars + (size_t)nLevels + 1), nIn(kScalars + 2 * ((size_t)nLevels + 1)) {}
};

// n voters' data on the device, n x 32 B each, standard form (eid 2 x 32 B, vote_hash n x 2 x 32 B); sik and nullifier are outputs of zkc_voter_hashes
struct VoterArrays { uint32_t *eid, *address, *password, *signature, *avail, *vote_weight, *vote_hash, *sik, *nullifier; };

}  // namespace zkc

// val[node] = H(val[left], val[right]) for M (node, left, right) triples at d_trip, grouped by depth, deepest first: the k-th deepest depth is triples off[k] .. off[k + 1]
// (D + 1 entries, off[D] = M; h_off on the host, d_off its device copy).  Launches only, on ctx->stream: the caller has checked every reference against val's size.
void zkc_hash_levels(zkc_ctx* ctx, const uint32_t* d_trip, const uint32_t* d_off, const uint32_t* h_off, int D, uint32_t M, uint32_t* d_val);
// v.sik = H(address, password, signature) and v.nullifier = H(signature, password, electionId) of n voters (census.circom:74-77, :105-109), on ctx->stream
int zkc_voter_hashes(zkc_ctx* ctx, const zkc::VoterArrays& v, size_t n);
// n input blocks into d_out (device, n x nIn x 32 B): zeroed, the scalars from v and the roots val_c[root_c], val_s[root_s], then the siblings by (slot of d_out, reference)
// pairs, np from val_c and nq from val_s (device lists).  Blocks to inputs_out, roots to roots_out (host, either may be NULL).  Ends with the stream synchronised.
int zkc_write_input_blocks(zkc_ctx* ctx, const zkc::VoterArrays& v, size_t n, const zkc::InputBlock& L, const uint32_t* val_c, uint32_t root_c, const uint32_t* val_s,
                           uint32_t root_s, const uint2* pairs_c, size_t np, const uint2* pairs_s, size_t nq, uint32_t* d_out, void* inputs_out, uint8_t* roots_out);
