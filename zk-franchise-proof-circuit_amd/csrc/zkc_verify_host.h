// zkc_verify_host.h -- what the two verifier files share: zkc_verify.hip (one proof, CPU only) defines all of it, zkc_verify_batch.hip (the batch verifiers, which take a
// context) uses it.  Internal to the library: nothing here is exported.
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "zkc_prover.h"
#include "zkc_pairing.h"
#include "zkc_host_util.h"

#pragma GCC visibility push(hidden)
namespace zkc {
// points in the standard form of the C ABI: rd_*_std / wr_*_std (zkc_host_util.h)
// an element of Fq12 as zkc_pairing_bin writes it: 12 x 32 B standard form, c0.a0.(c0, c1) c0.a1 c0.a2 c1.a0 c1.a1 c1.a2
void fq12_to_std(const pairing::Fq12& e, uint8_t out[384]);

// a verification key made ready once (zkc_verify.hip): points read and checked, gamma, delta and beta prepared, the Miller value of (alpha, beta) computed
struct VkReady {
    std::vector<uint8_t> bytes; int nPublic = 0;
    G1Affine alpha; G2Affine beta, gamma, delta; std::vector<G1Affine> ic;
    pairing::G2Prepared pgamma, pdelta, pbeta; pairing::Fq12 m_alpha_beta;
    std::vector<G1Affine> ic_mult;                 // k IC_j for k = 1..15, j = 1..nPublic (row j - 1): the public-input combination takes one addition per 4 bits of a signal
};
std::shared_ptr<const VkReady> vk_ready(const uint8_t* vk, int nPublic, int* code);      // NULL: *code = -ZKC_ERR_FORMAT, the text in zkc_verify_last_error
// sum_j k_j P_j over a handful of points (the public-input combination vk_x): one doubling chain shared by all scalars, mixed additions
G1XYZZ g1_sum_of_products(const G1Affine* pts, const uint32_t (*k)[8], int n);

// n weights of 128 bits as n x 8 little-endian words, from the verifiers' generator: seeded by seed32 (reproducible: tests) or, NULL, from the OS (zkc_verify_batch.hip)
std::vector<uint32_t> verify_weights(const uint8_t* seed32, size_t n);

std::string& verify_error();                       // the calling thread's text behind zkc_verify_last_error
int vfail(int code, const std::string& m);         // sets that text, returns code
}  // namespace zkc
#pragma GCC visibility pop
