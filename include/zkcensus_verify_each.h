/* zkcensus_verify_each.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): the batch verifier with a verdict per proof.
 *
 * ---- f4: zkc_verify_batch says whether ALL N proofs of a batch are valid; zkc_verify_batch_each says WHICH are not, for a counting node that must drop the one forged
 * ballot among thousands and keep the rest.  Arguments, layouts, seed32, the cache of prepared keys, error codes and zkc_verify_last_error() are zkc_verify_batch's;
 * verdict receives N values of the enumeration below.  ZKC_ERR_BAD_ARG (negated, before any device work): what zkc_verify_batch refuses, and verdict == NULL.
 * Returns 1 when every verdict is ZKC_PROOF_VALID, 0 when at least one is not, <0 = -ZKC_ERR_* (the verdicts are undefined then).  For the same inputs and seed the
 * return value is zkc_verify_batch's.
 * A proof that fails a format check (in zkc_verify_batch's order: coordinates, curves, then the public signals, so MALFORMED wins over PUBLIC_RANGE; B outside the
 * order-r subgroup is found on the device and is MALFORMED too) gets its verdict and is replaced by a neutral member -- A, B, C at infinity, no share in the weighted
 * sums -- for everything that follows.  The first pass is then zkc_verify_batch's own: a batch whose check passes costs what it costs there and is done.  A batch whose
 * check fails is searched: the per-step products of every round of pairs are the upper levels of a product tree whose every node is the Miller value of a dyadic range
 * of proofs, and the same random-linear-combination check runs on any node (its products, the sums of its members' weights, one final exponentiation: about one single
 * verification of host work).  The descent tests a bad node's left child; if it passes, the right child is bad without a test, otherwise the right child is tested too;
 * a bad range of at most two proofs is verified singly (zkc_verify_bin's path).  The levels below a round's top exist only after that round has been recomputed with
 * every level kept (34 KB of device memory per proof of the round, released with the verifier's work space).  Independent checks run on up to 16 host threads.
 * Budget: once the range checks of a call reach max(16, N / 4) the descent stops and every proof still undecided is verified singly, so the worst case is at most 1.25 x
 * the cost of N single verifications -- the only bound on a batch with many bad members.
 * Soundness: every check of a call uses the call's ONE weight vector; a tree has fewer than 2N dyadic ranges, so by a union bound a verdict is wrong with probability
 * about 2N x 2^-128 (seed32 fresh and unpredictable, as for zkc_verify_batch).
 * Environment: ZKC_VERIFY_BATCH_GPU and ZKC_VERIFY_CHUNK as for zkc_verify_batch.  With the Miller loops on host threads (0, or N < 128 by default) there is no tree: a
 * failing batch is verified singly on host threads.
 * zkc_verify_each_stats: of the context's last zkc_verify_batch_each -- out[0] range checks made beyond the first whole-batch check, out[1] proofs verified singly,
 * out[2] rounds whose product tree was rebuilt with its levels kept, out[3] 1 if the budget ended the descent.  ZKC_ERR_BAD_ARG for a NULL argument. ---- */
#ifndef ZKCENSUS_VERIFY_EACH_H
#define ZKCENSUS_VERIFY_EACH_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
    ZKC_PROOF_VALID = 0,
    ZKC_PROOF_INVALID = 1,        /* well-formed, the pairing equation fails */
    ZKC_PROOF_MALFORMED = 2,      /* a coordinate >= q, A / B / C off its curve, or B outside the order-r subgroup of the twist */
    ZKC_PROOF_PUBLIC_RANGE = 3    /* a public signal >= r */
};
int zkc_verify_batch_each(zkc_ctx* ctx, const uint8_t* vk, int nPublic, const uint8_t* pubs, const uint8_t* proofs, int N, const uint8_t* seed32,
                          int32_t* verdict /* N */);
int zkc_verify_each_stats(zkc_ctx* ctx, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
