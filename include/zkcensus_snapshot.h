/* zkcensus_snapshot.h -- part of the C ABI of libzkcensus.so (included by zkcensus.h, which it needs): frozen views of a resident census tree.
 *
 * ---- f1: snapshots of a census tree (arbo Tree.Snapshot), so that an election can freeze censusRoot and sikRoot when it opens and hand out every voter's siblings for
 * those roots until it closes, while the census goes on changing.  The conventions are zkcensus.h's for zkc_tree_*.
 * zkc_tree_snapshot    : *out = a read-only view of tree at its current version (tree may itself be a snapshot: the new view has the same version).  O(1), no device
 *                        work: the view shares every node with the live tree.  Later changes copy the paths they modify (each node a snapshot still reads is cloned
 *                        before it is written, and the clones are the nodes the change rehashes anyway), so memory grows only with what changes after the snapshot:
 *                        about (depth + 2) node references, 32 B of device memory each, per changed key while the snapshot is held.  ZKC_ERR_HIP on a broken tree.
 * zkc_tree_snapshot_count: *live = the number of live snapshots of tree's store (the live tree and all its snapshots share one store).
 * On a snapshot handle, zkc_tree_root, zkc_tree_size, zkc_tree_get, zkc_tree_gen_proof, zkc_tree_gen_absence_proof and zkc_tree_census_inputs (either tree or both may be
 *                        snapshots, of the same store or not) answer for the snapshot's version, byte for byte what they give on a tree built fresh from the snapshot's
 *                        set; zkc_tree_refs and zkc_tree_stats report the shared store (references retired by a change but still read by a snapshot count as live).
 *                        zkc_tree_add / update / delete on a snapshot return ZKC_ERR_BAD_ARG before anything is touched, statuses unwritten.
 * Lifetime             : zkc_tree_free releases any handle; the store lives until its last handle is freed, so freeing the live tree first leaves its snapshots usable.
 *                        Releasing a snapshot frees the node references and leaf rows only it still held, for later changes to reuse.  Every handle of a store shares the
 *                        store's mutex.  Both functions return ZKC_ERR_BAD_ARG for a NULL argument and then write nothing. ---- */
#ifndef ZKCENSUS_SNAPSHOT_H
#define ZKCENSUS_SNAPSHOT_H
#include "zkcensus.h"
#ifdef __cplusplus
extern "C" {
#endif

int zkc_tree_snapshot(zkc_tree* tree, zkc_tree** out);
int zkc_tree_snapshot_count(zkc_tree* tree, size_t* live);

#ifdef __cplusplus
}
#endif
#endif
