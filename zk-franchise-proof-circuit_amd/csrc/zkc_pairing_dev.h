// zkc_pairing_dev.h -- the batch verifiers' device side (zkc_pairing_dev.hip) as csrc/zkc_verify_batch.hip calls it.  Host code; the caller holds the context's lock.
#pragma once
#include <vector>
#include "zkc_prover.h"
#include "zkc_pairing.h"

namespace zkc {
// The product tree of a round of n pairs, level by level: m[0] = ceil(n / 2) pair products, m[k + 1] = ceil(m[k] / 2), down to one node; off[k] = nodes below level k.
// Node t of level k covers the pairs [t << (k + 1), min(n, (t + 1) << (k + 1))); an odd level hands its last node up unchanged.
struct TreeShape {
    uint32_t n; std::vector<uint32_t> m, off; size_t nodes = 0;
    explicit TreeShape(uint32_t pairs) : n(pairs) { for (uint32_t k = (n + 1) / 2;; k = (k + 1) / 2) { m.push_back(k); off.push_back((uint32_t)nodes); nodes += k; if (k <= 1) break; } }
};
uint32_t verify_chunk();        // pairs per round of kernels ($ZKC_VERIFY_CHUNK)
uint32_t verify_n_lines();      // lines of one Miller loop = products per tree node
int miller_membership_begin(zkc_ctx* ctx, const G2Affine* h_Q, uint32_t N);
void miller_join(zkc_ctx* ctx);
int miller_product_dev(zkc_ctx* ctx, const G1XYZZ* d_P, uint32_t N, pairing::Fq12* product, int* bad, std::vector<pairing::Fq12>* tops = nullptr);
int miller_membership_each(zkc_ctx* ctx, uint32_t N, int32_t* h_flag);
int g2_membership_first_bad(zkc_ctx* ctx, const G2Affine* d_Q, uint32_t N, uint32_t* bad);      // the membership kernel over the caller's device points: the smallest index outside G2
int miller_sum_trees(zkc_ctx* ctx, const G1XYZZ* d_C, uint32_t N, std::vector<G1XYZZ>& h);
int miller_round_levels(zkc_ctx* ctx, const G1XYZZ* d_P, uint32_t N, uint32_t c);
int miller_nodes_fetch(zkc_ctx* ctx, uint32_t n, const uint32_t (*node)[2], size_t count, pairing::Fq12* out);
pairing::Fq12 miller_walk(const pairing::Fq12* acc);
}  // namespace zkc
