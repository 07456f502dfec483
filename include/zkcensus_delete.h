/* zkcensus_delete.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): census trees that shrink, and non-membership proofs.
 *
 * ---- f1: voters removed from a resident census tree (arbo Delete) and keys proven absent (arbo GenProof of an absent key; circomlib SMTVerifier with fnc = 1).  The
 * conventions are zkcensus.h's for zkc_tree_* and zkc_smt_check_proofs: 32-byte little-endian words in standard form, host buffers, ZKC_TREE_* statuses and ZKC_SMT_*
 * verdicts, the per-tree mutex, a HIP failure during a change marking the tree broken.
 * zkc_tree_delete      : arbo Delete.  status: OK, KEY_ABSENT (also a key deleted earlier in the same batch), NOT_BELOW_R (key >= r).  Batches as for zkc_tree_add: the
 *                        entries apply one by one in order, a rejected entry changes nothing.  The tree stays equal to zkc_smt_build over its current set: a leaf left
 *                        alone below its parent is lifted to the first ancestor with a non-empty other side (or to the root) and the chain nodes it passes are freed;
 *                        deleting the last leaf leaves root 0.  Freed node references and leaf rows are reused by later adds, so a census that churns at constant size
 *                        stays at constant size.  zkc_tree_stats reports a delete as it reports an add.
 * zkc_tree_gen_absence_proof: arbo GenProof for absent keys: root, and per key siblings / depths laid out as zkc_tree_gen_proof lays them out (may be NULL), old_keys /
 *                        old_values (n x 32 B) and is_old0 (n x int32): where the key's path ends -- an empty child (is_old0 = 1, old key and value 0) or the leaf of
 *                        another key (is_old0 = 0, that leaf's key and value).  status n x int32: OK (absent, proof written), KEY_EXISTS (the key is present: zeroed
 *                        outputs; see zkc_tree_gen_proof), NOT_BELOW_R.  An empty tree gives root 0, depth 0 and is_old0 = 1.
 * zkc_tree_refs        : out[0] = live node references (inner nodes and leaves), out[1] = allocated references (the length of the host arrays, free entries included).
 * zkc_smt_check_absence: exclusion proofs as zkc_tree_gen_absence_proof writes them, checked as zkc_smt_check_proofs checks membership: keys, old_keys, old_values
 *                        n x 32 B, is_old0 n x int32 (0 or 1), siblings and roots as there.  depth as there; cur = 0 when is_old0, else H(old_key, old_value, 1); then
 *                        the climb from depth - 1 down to 0 with the KEY's path bits; valid iff cur == root.  Host checks before any hashing, in this order: the field
 *                        checks (key, old key, old value, every sibling, the root), the last-slot rule, ZKC_SMT_KEY_PRESENT (!is_old0 and old_key == key),
 *                        ZKC_SMT_OFF_PATH (!is_old0 and old_key leaves the key's first depth path bits).  ZKC_ERR_BAD_ARG (before any device work) as there, and for
 *                        an is_old0 entry that is not 0 or 1.  zkc_smt_check_stats reports it as it reports zkc_smt_check_proofs. ---- */
#ifndef ZKCENSUS_DELETE_H
#define ZKCENSUS_DELETE_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_tree_delete(zkc_tree* tree, const void* keys, size_t n, int32_t* status);
int zkc_tree_gen_absence_proof(zkc_tree* tree, const void* keys, size_t n, uint8_t root[32], void* siblings, int32_t* depths, void* old_keys, void* old_values,
                               int32_t* is_old0, int32_t* status);
int zkc_tree_refs(zkc_tree* tree, size_t out[2]);
int zkc_smt_check_absence(zkc_ctx* ctx, int nLevels, size_t n, const void* keys, const void* old_keys, const void* old_values, const int32_t* is_old0,
                          const void* siblings, const void* roots, int per_proof_roots, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
