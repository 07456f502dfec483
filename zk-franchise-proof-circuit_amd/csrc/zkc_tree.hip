// zkc_tree.hip -- f1: a census tree that grows in place (arbo NewTree / Add / AddBatch / Update / Get / GenProof; internal/helpers.go:36-85), beside the static builder of
// zkc_census.hip.  A Vocdoni census gains voters as they register; rebuilding the whole trie and rehashing every node per change costs what zkc_smt_build costs.  Here:
//
// - The trie stays on the host as flat arrays indexed by node reference (no pointers): per inner node its two child references and its depth, per leaf its key and value.
//   Leaves and inner nodes share one reference space; 0 is the empty subtree.  A leaf keeps its reference when a later key pushes it down a chain, so its hash stays valid.
// - The hashes stay on the device in ONE array val[reference] (val[0] = 0), doubled in place when full.  The device holds no child table: per batch the host uploads the
//   whole description of the work -- the changed leaves as (slot, key, value) and the dirty inner nodes as (node, left, right) triples grouped by depth, deepest first --
//   and rehashes only those: zkc_tree_leaves, then zkc_hash_levels (zkc_census.hip, shared with the static builder): one zkc_tree_level launch per depth with more than
//   a wave of dirty nodes and one zkc_tree_narrow launch per maximal run of narrower depths (the top of the tree, and the one-child chains below two keys with a long
//   common path prefix: up to nLevels levels in one launch instead of one launch each).  Kernels live in zkc_witness.hip beside poseidon_trace29, declared in zkc_kernels.h.
//
// arbo semantics as zkc_smt_build pins them: leaf = H(key, value, 1), node = H(left, right), path bit i = bit i of the key (LSB first), an empty subtree is 0, a subtree
// holding one leaf is that leaf's hash; inner nodes sit at depths 0 .. nLevels - 1.  Inserting walks from the root along the key bits: at an empty child the leaf goes
// there; at a leaf with another key, a chain of inner nodes (one child each, except the last) runs down to the first bit where the two keys differ.
//
// Deleting (arbo Delete) keeps that canonical form: the leaf goes; when its sibling is a leaf, that leaf is lifted past its parent and every ancestor whose other child is
// empty (those chain nodes are freed), up to the first ancestor with a non-empty other side or the root; when its sibling is an inner node, the parent stays as a one-child
// chain node.  A leaf's hash does not depend on its depth, so a lifted leaf is not rehashed.  Freed references and leaf rows go on free lists that later inserts take from
// first -- but only after the call's commit, so a reference freed and reused within one batch can never be hashed as the inner node it was.
//
// Snapshots (arbo Tree.Snapshot): a zkc_tree is a handle -- a root, a leaf count, a version -- on a shared, reference-counted store that holds everything above.  The
// live handle changes the store; a snapshot handle is a read-only view pinning the version it was taken at.  Every reference carries its birth version; a change runs at
// version V + 1 when a snapshot pins the last committed version V (at V otherwise), and a reference born at or below the newest live snapshot's version is pinned: a
// change never writes its children, its leaf row or val at it.  It copies the path instead: each pinned inner node the entry modifies is cloned (same children, same
// depth) and relinked under its already-owned parent or as the root; an update of a pinned leaf takes a new leaf row and reference.  A leaf pushed down a chain or lifted
// by a delete is not copied (its hash does not depend on its depth).  The clones are the nodes the commit rehashes anyway, so path copying adds no hashing.  A pinned
// reference a change would free is retired with its [birth, death) versions instead; releasing a snapshot frees the retired references no live snapshot falls into.
// Without a live snapshot nothing is pinned and every change takes the path it took before snapshots existed, reference for reference.
#include "zkc_census_host.h"
#include "zkc_kernels.h"
#include <algorithm>
#include <mutex>
#include <set>
#include <vector>

using namespace zkc;

namespace {
// what every handle of one tree shares: the trie, the device values, the buffers, the mutex
struct zkc_store {
    zkc_ctx* ctx = nullptr;
    int nLevels = 0;
    std::mutex mu;
    bool broken = false;                     // a HIP call failed while the tree changed: host trie and device values may disagree
    // host trie by reference: inner node -> a = left, b = right, depth 0 .. nLevels - 1; leaf -> a = leaf index, depth = LEAF.  Reference 0 (empty) is a placeholder.
    std::vector<uint32_t> a{0}, b{0};
    std::vector<uint8_t> depth{0}, dirty{0};
    std::vector<uint8_t> keys, vals;         // per leaf index, 32 B each
    std::vector<uint32_t> free_refs, free_rows;             // free references / leaf rows, taken first by new_ref / new_leaf
    std::vector<uint32_t> freed_refs, freed_rows;           // freed by the current call: they join the free lists after its commit
    std::vector<uint32_t> dirty_nodes, dirty_leaves, path;
    // device
    uint32_t* d_val = nullptr; size_t cap = 0;              // val capacity, in references
    void* d_stage = nullptr; size_t d_stage_sz = 0;         // a call's uploads
    uint8_t* h_stage = nullptr; size_t h_stage_sz = 0;      // their pinned host copy
    void* d_out = nullptr; size_t d_out_sz = 0;             // gen_proof / census_inputs output blocks
    double ms[2] = {0, 0};
    // versions (snapshots; see the top of the file)
    size_t handles = 0;                      // the live handle and the snapshots: the store goes with the last of them
    uint32_t cur = 0;                        // the version the running change stamps
    std::vector<uint32_t> birth{0};          // per reference: the version that made it (a leaf row is born with its leaf's reference)
    std::multiset<uint32_t> snaps;           // the versions of the live snapshots
    uint64_t pin_lim = 0;                    // references born below this are pinned: the newest snapshot's version + 1, 0 without snapshots
    struct Retired { uint32_t ref, birth, death; };
    std::vector<Retired> retired;            // pinned references a change dropped: freed when no snapshot version lies in [birth, death)
};
}  // namespace

struct zkc_tree {
    zkc_store* s = nullptr;
    uint32_t root = 0;
    size_t leaves = 0;
    uint32_t version = 0;                    // a snapshot's pinned version; the live tree's last committed one, which a snapshot of it pins
    bool is_snapshot = false;
};

namespace {
constexpr uint8_t LEAF = 0xff;
constexpr uint8_t FREED = 0xfe;               // depth of a reference freed by the current call (never a real depth: nLevels <= 253)
constexpr uint64_t MAX_REFS = 0xfffffff0ull;
const char* const BROKEN = "zkc_tree: the tree is broken by an earlier device failure";

inline const uint8_t* leaf_key(const zkc_store* s, uint32_t r) { return s->keys.data() + 32 * (size_t)s->a[r]; }
inline uint8_t* leaf_val(zkc_store* s, uint32_t r) { return s->vals.data() + 32 * (size_t)s->a[r]; }
inline uint32_t child(const zkc_store* s, uint32_t node, int side) { return side ? s->b[node] : s->a[node]; }
inline void set_child(zkc_tree* t, uint32_t node, int side, uint32_t r) { if (!node) t->root = r; else (side ? t->s->b[node] : t->s->a[node]) = r; }
inline bool pinned(const zkc_store* s, uint32_t r) { return s->birth[r] < s->pin_lim; }
uint32_t new_ref(zkc_store* s, uint32_t a, uint32_t b, uint8_t depth) {
    if (!s->free_refs.empty()) {                 // a reference freed by an earlier call: not dirty, not in this call's lists
        const uint32_t r = s->free_refs.back(); s->free_refs.pop_back();
        s->a[r] = a; s->b[r] = b; s->depth[r] = depth; s->dirty[r] = 0; s->birth[r] = s->cur;
        return r;
    }
    s->a.push_back(a); s->b.push_back(b); s->depth.push_back(depth); s->dirty.push_back(0); s->birth.push_back(s->cur);
    return (uint32_t)(s->a.size() - 1);
}
uint32_t new_leaf(zkc_store* s, const uint8_t* key, const uint8_t* val) {
    uint32_t li;
    if (!s->free_rows.empty()) {
        li = s->free_rows.back(); s->free_rows.pop_back();
        memcpy(s->keys.data() + 32 * (size_t)li, key, 32); memcpy(s->vals.data() + 32 * (size_t)li, val, 32);
    } else {
        li = (uint32_t)(s->keys.size() / 32);
        s->keys.insert(s->keys.end(), key, key + 32); s->vals.insert(s->vals.end(), val, val + 32);
    }
    return new_ref(s, li, 0, LEAF);
}
// r (and its leaf row) onto the given lists: a running change frees into freed_refs / freed_rows, which join the free lists only after its commit (free_ref); with no
// change running, unpin frees into the free lists themselves
void free_into(zkc_store* s, uint32_t r, std::vector<uint32_t>& refs, std::vector<uint32_t>& rows) {
    if (s->depth[r] == LEAF) rows.push_back(s->a[r]);
    s->depth[r] = FREED; s->a[r] = s->b[r] = 0;
    refs.push_back(r);
}
void free_ref(zkc_store* s, uint32_t r) { free_into(s, r, s->freed_refs, s->freed_rows); }
// a reference the change drops: freed, or retired untouched while a snapshot may still read it
void release(zkc_store* s, uint32_t r) {
    if (pinned(s, r)) s->retired.push_back({r, s->birth[r], s->cur}); else free_ref(s, r);
}
// the first k inner nodes of s->path, which the entry is about to modify, owned by this version: each pinned one is cloned, relinked under its (already owned) parent or
// as the root, retired, and replaced in s->path by its clone
void own_path(zkc_tree* t, const uint8_t* key, size_t k) {
    zkc_store* s = t->s;
    if (!s->pin_lim) return;
    for (size_t i = 0; i < k; i++) {
        const uint32_t r = s->path[i];
        if (!pinned(s, r)) continue;
        const uint32_t c = new_ref(s, s->a[r], s->b[r], s->depth[r]);
        set_child(t, i ? s->path[i - 1] : 0, i ? key_bit(key, (int)i - 1) : 0, c);
        release(s, r);
        s->path[i] = c;
    }
}
inline void mark(zkc_store* s, uint32_t r, std::vector<uint32_t>& list) { if (!s->dirty[r]) { s->dirty[r] = 1; list.push_back(r); } }
void mark_path(zkc_store* s) { for (uint32_t r : s->path) mark(s, r, s->dirty_nodes); }

// the walk from t's root along the key's path bits: returns where it ends, a leaf (of this key or another) or an empty child (0); t->s->path = the inner nodes passed,
// root first, so the end hangs below path[d - 1] on side key bit d - 1 with d = path.size() (below the root handle when d = 0)
uint32_t descend(zkc_tree* t, const uint8_t* key) {
    zkc_store* s = t->s;
    s->path.clear();
    uint32_t r = t->root;
    for (int d = 0; r && s->depth[r] != LEAF; d++) { s->path.push_back(r); r = child(s, r, key_bit(key, d)); }
    return r;
}
// the leaf reference of `key` in t's tree (0: absent); t->s->path as descend leaves it
uint32_t find(zkc_tree* t, const uint8_t* key) {
    const uint32_t r = descend(t, key);
    return r && memcmp(leaf_key(t->s, r), key, 32) == 0 ? r : 0;
}
int32_t add_one(zkc_tree* t, const uint8_t* key, const uint8_t* val) {
    if (!below_r(key) || !below_r(val)) return ZKC_TREE_NOT_BELOW_R;
    zkc_store* s = t->s;
    const uint32_t r = descend(t, key); const int d = (int)s->path.size();
    // r: the empty child or the leaf at depth d where the walk ended, below path[d - 1] on side key bit d - 1 (the root when d = 0)
    if (r == 0) {                                                                  // an empty child: the leaf goes here
        own_path(t, key, d);
        const uint32_t l = new_leaf(s, key, val);
        set_child(t, d ? s->path[d - 1] : 0, d ? key_bit(key, d - 1) : 0, l); mark_path(s); mark(s, l, s->dirty_leaves);
        return ZKC_TREE_OK;
    }
    const uint8_t* other = leaf_key(s, r);
    if (memcmp(other, key, 32) == 0) return ZKC_TREE_KEY_EXISTS;
    int e = d; while (e < s->nLevels && key_bit(key, e) == key_bit(other, e)) e++;
    if (e >= s->nLevels) return ZKC_TREE_COLLISION;
    // a chain of inner nodes at depths d .. e: one child each down to e, where the old leaf r and the new one part
    own_path(t, key, d);
    const uint32_t l = new_leaf(s, key, val);
    uint32_t up = d ? s->path[d - 1] : 0; int up_side = d ? key_bit(key, d - 1) : 0;
    for (int c = d; c <= e; c++) {
        const uint32_t nd = new_ref(s, 0, 0, (uint8_t)c);
        set_child(t, up, up_side, nd); s->path.push_back(nd);
        up = nd; up_side = key_bit(key, c);
    }
    set_child(t, up, up_side, l); set_child(t, up, !up_side, r);
    mark_path(s); mark(s, l, s->dirty_leaves);
    return ZKC_TREE_OK;
}
// arbo Delete (see the top of the file): the leaf goes, a leaf left alone below its parent climbs past every ancestor whose other child is empty, the rest is marked dirty
int32_t delete_one(zkc_tree* t, const uint8_t* key) {
    if (!below_r(key)) return ZKC_TREE_NOT_BELOW_R;
    zkc_store* s = t->s;
    const uint32_t l = find(t, key);
    if (!l) return ZKC_TREE_KEY_ABSENT;
    release(s, l);
    const std::vector<uint32_t>& p = s->path;
    if (p.empty()) { t->root = 0; return ZKC_TREE_OK; }
    int j = (int)p.size() - 1;                                 // p[j] is the leaf's parent, the leaf on side key bit j
    const uint32_t other = child(s, p[j], !key_bit(key, j));
    if (other && s->depth[other] != LEAF) {
        own_path(t, key, (size_t)j + 1);
        set_child(t, p[j], key_bit(key, j), 0);
        for (int i = 0; i <= j; i++) mark(s, p[i], s->dirty_nodes);
        return ZKC_TREE_OK;
    }
    // `other` (a leaf; 0 never occurs in the canonical form) replaces p[j] and every chain ancestor above it that holds nothing else
    release(s, p[j]);
    while (j > 0 && child(s, p[j - 1], !key_bit(key, j - 1)) == 0) release(s, p[--j]);
    if (j == 0) { t->root = other; return ZKC_TREE_OK; }
    own_path(t, key, (size_t)j);
    set_child(t, p[j - 1], key_bit(key, j - 1), other);
    for (int i = 0; i < j; i++) mark(s, p[i], s->dirty_nodes);
    return ZKC_TREE_OK;
}
int32_t update_one(zkc_tree* t, const uint8_t* key, const uint8_t* val) {
    if (!below_r(key) || !below_r(val)) return ZKC_TREE_NOT_BELOW_R;
    zkc_store* s = t->s;
    uint32_t l = find(t, key);
    if (!l) return ZKC_TREE_KEY_ABSENT;
    const size_t d = s->path.size();
    own_path(t, key, d);
    if (pinned(s, l)) {                                        // a snapshot reads the old value: a new leaf row and reference take its place
        const uint32_t nl = new_leaf(s, key, val);
        set_child(t, d ? s->path[d - 1] : 0, d ? key_bit(key, (int)d - 1) : 0, nl);
        release(s, l);
        l = nl;
    } else {
        memcpy(leaf_val(s, l), val, 32);
    }
    mark_path(s); mark(s, l, s->dirty_leaves);
    return ZKC_TREE_OK;
}

// room for `bytes` of uploads: device buffer and its pinned host copy (nothing of an earlier call is in flight: every call ends synchronised)
int stage(zkc_store* s, size_t bytes) {
    zkc_ctx* ctx = s->ctx; int rc;
    if ((rc = zkc_ensure(ctx, &s->d_stage, &s->d_stage_sz, bytes))) return rc;
    if (s->h_stage_sz < bytes) {
        if (s->h_stage) { ZKC_HIP_CHECK(ctx, hipHostFree(s->h_stage)); s->h_stage = nullptr; s->h_stage_sz = 0; }
        const size_t sz = std::max(bytes, (size_t)1 << 20);
        ZKC_HIP_CHECK(ctx, hipHostMalloc((void**)&s->h_stage, sz));
        s->h_stage_sz = sz;
    }
    return ZKC_OK;
}
// val holds at least `need` references: double it, copying the old values on the stream
int grow(zkc_store* s, size_t need) {
    if (need <= s->cap) return ZKC_OK;
    zkc_ctx* ctx = s->ctx;
    size_t cap = std::max<size_t>(s->cap, 1024); while (cap < need) cap *= 2;
    uint32_t* nv = nullptr;
    ZKC_HIP_CHECK(ctx, hipMalloc((void**)&nv, 32 * cap));
    if (s->d_val) {
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(nv, s->d_val, 32 * s->cap, hipMemcpyDeviceToDevice, ctx->stream));
        ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ZKC_HIP_CHECK(ctx, hipFree(s->d_val));
    } else {
        ZKC_HIP_CHECK(ctx, hipMemsetAsync(nv, 0, 32, ctx->stream));                    // val[0]: the empty subtree
    }
    s->d_val = nv; s->cap = cap;
    return ZKC_OK;
}

// hash what the entries of this call changed: the dirty leaves, then the dirty inner nodes deepest first.  Clears the dirty lists.
int commit(zkc_store* s, clk::time_point t0) {
    zkc_ctx* ctx = s->ctx;
    for (uint32_t r : s->dirty_leaves) s->dirty[r] = 0;
    for (uint32_t r : s->dirty_nodes) s->dirty[r] = 0;
    if (!s->freed_refs.empty()) {                // references this call freed: nothing hashes them (they are reused only after this commit)
        auto gone = [s](uint32_t r) { return s->depth[r] == FREED; };
        s->dirty_leaves.erase(std::remove_if(s->dirty_leaves.begin(), s->dirty_leaves.end(), gone), s->dirty_leaves.end());
        s->dirty_nodes.erase(std::remove_if(s->dirty_nodes.begin(), s->dirty_nodes.end(), gone), s->dirty_nodes.end());
    }
    const size_t K = s->dirty_leaves.size(), M = s->dirty_nodes.size();
    if (!K && !M) { s->ms[0] = ms_since(t0); s->ms[1] = 0; return ZKC_OK; }
    // the dirty nodes by depth, deepest first (depth d is the (D - 1 - d)-th deepest): the k-th deepest depth's triples are off[k] .. off[k + 1], off[D] = M
    int D = 0; for (uint32_t r : s->dirty_nodes) D = std::max(D, s->depth[r] + 1);
    std::vector<uint32_t> off(D + 1, 0);
    for (uint32_t r : s->dirty_nodes) off[D - s->depth[r]]++;
    for (int k = 0; k < D; k++) off[k + 1] += off[k];
    // one upload: [slots K][keys K x 32 B][values K x 32 B][triples M x 3][offsets: position of the k-th deepest depth, D + 1]
    const size_t o_keys = align256(4 * K), o_vals = o_keys + align256(32 * K), o_trip = o_vals + align256(32 * K), o_off = o_trip + align256(12 * M), total = o_off + 4 * ((size_t)D + 1);
    int rc;
    if ((rc = stage(s, total))) return rc;
    uint8_t* h = s->h_stage;
    uint32_t* hs = (uint32_t*)h; uint32_t* ht = (uint32_t*)(h + o_trip); uint32_t* ho = (uint32_t*)(h + o_off);
    const uint64_t nref = s->a.size();
    for (size_t i = 0; i < K; i++) {
        const uint32_t r = s->dirty_leaves[i];
        hs[i] = r; memcpy(h + o_keys + 32 * i, leaf_key(s, r), 32); memcpy(h + o_vals + 32 * i, leaf_val(s, r), 32);
    }
    { std::vector<uint32_t> fill(off.begin(), off.end() - 1);
      for (uint32_t r : s->dirty_nodes) { uint32_t* q = ht + 3 * (size_t)fill[D - 1 - s->depth[r]]++; q[0] = r; q[1] = s->a[r]; q[2] = s->b[r]; } }
    memcpy(ho, off.data(), 4 * ((size_t)D + 1));
    // every reference a kernel will follow is below the number of references (and so below val's capacity, grown to it next)
    for (size_t i = 0; i < K; i++) if (hs[i] == 0 || hs[i] >= nref) return zkc_fail(ctx, ZKC_ERR_GENERIC, "zkc_tree: leaf slot out of range");
    for (size_t i = 0; i < 3 * M; i++) if (ht[i] >= nref || (i % 3 == 0 && ht[i] == 0)) return zkc_fail(ctx, ZKC_ERR_GENERIC, "zkc_tree: node reference out of range");
    s->dirty_leaves.clear(); s->dirty_nodes.clear();
    s->ms[0] = ms_since(t0);
    const clk::time_point t1 = clk::now();
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = grow(s, nref))) return rc;
    uint8_t* dst = (uint8_t*)s->d_stage;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(dst, h, total, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* dt = (const uint32_t*)(dst + o_trip); const uint32_t* dof = (const uint32_t*)(dst + o_off);
    if (K) hipLaunchKernelGGL(zkc_tree_leaves, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, ctx->stream, ctx->ptab, (const uint32_t*)dst, (const uint32_t*)(dst + o_keys),
                              (const uint32_t*)(dst + o_vals), (uint32_t)K, s->d_val);
    zkc_hash_levels(ctx, dt, dof, ho, D, (uint32_t)M, s->d_val);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    s->ms[1] = ms_since(t1);
    return ZKC_OK;
}

enum Op { ADD, UPDATE, DELETE };
int change(zkc_tree* t, const void* keys, const void* values, size_t n, int32_t* status, Op op) {
    const bool add = op == ADD;
    if (!t || t->is_snapshot || (n && (!keys || (op != DELETE && !values) || !status)))
        return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, t && t->is_snapshot ? "zkc_tree_add / update / delete: the tree is a read-only snapshot"
                                                                                     : "zkc_tree_add / update / delete: bad argument");
    zkc_store* s = t->s;
    std::lock_guard<std::mutex> g(s->mu);
    zkc_ctx* ctx = s->ctx;
    ZKC_LOCK(ctx);
    if (s->broken) return zkc_fail(ctx, ZKC_ERR_HIP, BROKEN);
    // with a live snapshot, updates and deletes allocate too (path copies): at most nLevels clones and one leaf per entry
    if ((add || s->pin_lim) && s->a.size() + (uint64_t)n * (s->nLevels + 2) > MAX_REFS) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree_add: the tree would exceed 2^32 nodes");
    const bool snapped = s->snaps.count(t->version) != 0;        // a snapshot pins the last committed version: this change makes the next one
    if (snapped && t->version == UINT32_MAX) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree: out of versions");
    s->cur = t->version + (snapped ? 1 : 0);
    const clk::time_point t0 = clk::now();
    const uint8_t* k = (const uint8_t*)keys; const uint8_t* v = (const uint8_t*)values;
    for (size_t i = 0; i < n; i++) {
        status[i] = op == ADD ? add_one(t, k + 32 * i, v + 32 * i) : op == UPDATE ? update_one(t, k + 32 * i, v + 32 * i) : delete_one(t, k + 32 * i);
        if (status[i] == ZKC_TREE_OK && op != UPDATE) { if (add) t->leaves++; else t->leaves--; }
    }
    const int rc = commit(s, t0);
    if (rc) { s->broken = true; return rc; }
    s->free_refs.insert(s->free_refs.end(), s->freed_refs.begin(), s->freed_refs.end()); s->freed_refs.clear();
    s->free_rows.insert(s->free_rows.end(), s->freed_rows.begin(), s->freed_rows.end()); s->freed_rows.clear();
    t->version = s->cur;
    return ZKC_OK;
}
// after a snapshot's release: the newest live snapshot, and the retired references no live snapshot version falls into go on the free lists (no change is running)
void unpin(zkc_store* s) {
    s->pin_lim = s->snaps.empty() ? 0 : (uint64_t)*s->snaps.rbegin() + 1;
    size_t k = 0;
    for (const zkc_store::Retired& e : s->retired) {
        const auto it = s->snaps.lower_bound(e.birth);
        if (it != s->snaps.end() && *it < e.death) { s->retired[k++] = e; continue; }
        free_into(s, e.ref, s->free_refs, s->free_rows);
    }
    s->retired.resize(k);
}
int read_root(zkc_tree* t, uint8_t root[32]) {
    zkc_ctx* ctx = t->s->ctx;
    if (!t->root) { memset(root, 0, 32); return ZKC_OK; }
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(root, t->s->d_val + 8 * (size_t)t->root, 32, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKC_OK;
}
// (dst, ref) pairs of the non-zero siblings on s->path for a key: dst = base + level
void sibling_pairs(const zkc_store* s, const uint8_t* key, size_t base, std::vector<uint2>& out) {
    for (size_t l = 0; l < s->path.size(); l++) {
        const uint32_t c = child(s, s->path[l], !key_bit(key, (int)l));
        if (c) out.push_back(make_uint2((uint32_t)(base + l), c));
    }
}
// the zero-padded sibling lists of a gen_proof call: `words` 32-byte words, the (dst, ref) pairs' values from val scattered in on the device, copied to `siblings`
int write_siblings(zkc_store* s, const std::vector<uint2>& pairs, size_t words, void* siblings) {
    zkc_ctx* ctx = s->ctx; int rc;
    const size_t out_bytes = 32 * words;
    if ((rc = zkc_ensure(ctx, &s->d_out, &s->d_out_sz, out_bytes)) || (rc = stage(s, pairs.size() * sizeof(uint2) + 8))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(s->d_out, 0, out_bytes, ctx->stream));
    if (!pairs.empty()) {
        memcpy(s->h_stage, pairs.data(), pairs.size() * sizeof(uint2));
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(s->d_stage, s->h_stage, pairs.size() * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(zkc_census_scatter, dim3((unsigned)((pairs.size() + 255) / 256)), dim3(256), 0, ctx->stream, s->d_val, (const uint2*)s->d_stage, pairs.size(),
                           (uint32_t*)s->d_out);
        ZKC_HIP_CHECK(ctx, hipGetLastError());
    }
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(siblings, s->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKC_OK;
}
// what zkc_tree_gen_proof and zkc_tree_gen_absence_proof share (`name`: the entry point, for the error text): the locks, the broken and 32-bit slot checks, then per
// key per_key(i, key), which fills that key's outputs and says whether its sibling list, for the path its walk left in s->path, goes out; then the root and the siblings
template <class PerKey>
int gen_proofs(zkc_tree* t, const char* name, const void* keys, size_t n, uint8_t root[32], void* siblings, PerKey per_key) {
    zkc_store* s = t->s;
    std::lock_guard<std::mutex> g(s->mu);
    zkc_ctx* ctx = s->ctx;
    ZKC_LOCK(ctx);
    if (s->broken) return zkc_fail(ctx, ZKC_ERR_HIP, BROKEN);
    const size_t stride = (size_t)s->nLevels + 1;
    if ((uint64_t)n * stride >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, std::string(name) + ": too many keys for 32-bit slots");
    std::vector<uint2> pairs;
    for (size_t i = 0; i < n; i++) {
        const uint8_t* key = (const uint8_t*)keys + 32 * i;
        if (per_key(i, key) && siblings) sibling_pairs(s, key, i * stride, pairs);
    }
    int rc;
    if ((rc = read_root(t, root))) return rc;
    if (!siblings || !n) return ZKC_OK;
    return write_siblings(s, pairs, n * stride, siblings);
}
}  // namespace

extern "C" int zkc_tree_create(zkc_ctx* ctx, int nLevels, zkc_tree** out) {
    if (out) *out = nullptr;
    if (!ctx || !out || nLevels < 1 || nLevels > 253) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree_create: bad argument");
    ZKC_LOCK(ctx);
    zkc_tree* t = new zkc_tree;
    t->s = new zkc_store;
    t->s->ctx = ctx; t->s->nLevels = nLevels; t->s->handles = 1;
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = grow(t->s, 1)) == ZKC_OK) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = zkc_fail(ctx, ZKC_ERR_HIP, std::string("zkc_tree_create: ") + hipGetErrorString(e));
    }
    if (rc) { zkc_tree_free(t); return rc; }
    *out = t;
    return ZKC_OK;
}

extern "C" void zkc_tree_free(zkc_tree* t) {
    if (!t) return;
    zkc_store* s = t->s;
    bool last;
    {
        std::lock_guard<std::mutex> g(s->mu);
        if (t->is_snapshot) { s->snaps.erase(s->snaps.find(t->version)); unpin(s); }
        last = --s->handles == 0;
    }
    delete t;
    if (!last) return;
    {
        ZKC_LOCK(s->ctx);
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
        if (s->d_val) (void)hipFree(s->d_val);
        if (s->d_stage) (void)hipFree(s->d_stage);
        if (s->d_out) (void)hipFree(s->d_out);
        if (s->h_stage) (void)hipHostFree(s->h_stage);
    }
    delete s;
}

extern "C" int zkc_tree_snapshot(zkc_tree* t, zkc_tree** out) {
    if (!t || !out) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_snapshot: bad argument");
    zkc_store* s = t->s;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->broken) return zkc_fail(s->ctx, ZKC_ERR_HIP, BROKEN);
    zkc_tree* c = new zkc_tree;
    c->s = s; c->root = t->root; c->leaves = t->leaves; c->is_snapshot = true;
    c->version = t->version;
    s->snaps.insert(c->version);
    s->pin_lim = (uint64_t)*s->snaps.rbegin() + 1;
    s->handles++;
    *out = c;
    return ZKC_OK;
}

extern "C" int zkc_tree_snapshot_count(zkc_tree* t, size_t* live) {
    if (!t || !live) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_snapshot_count: bad argument");
    std::lock_guard<std::mutex> g(t->s->mu);
    *live = t->s->snaps.size();
    return ZKC_OK;
}

extern "C" int zkc_tree_add(zkc_tree* t, const void* keys, const void* values, size_t n, int32_t* status) { return change(t, keys, values, n, status, ADD); }
extern "C" int zkc_tree_update(zkc_tree* t, const void* keys, const void* values, size_t n, int32_t* status) { return change(t, keys, values, n, status, UPDATE); }
extern "C" int zkc_tree_delete(zkc_tree* t, const void* keys, size_t n, int32_t* status) { return change(t, keys, nullptr, n, status, DELETE); }

extern "C" int zkc_tree_root(zkc_tree* t, uint8_t root[32]) {
    if (!t || !root) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_root: bad argument");
    std::lock_guard<std::mutex> g(t->s->mu);
    ZKC_LOCK(t->s->ctx);
    if (t->s->broken) return zkc_fail(t->s->ctx, ZKC_ERR_HIP, BROKEN);
    return read_root(t, root);
}

extern "C" int zkc_tree_size(zkc_tree* t, size_t* leaves) {
    if (!t || !leaves) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_size: bad argument");
    std::lock_guard<std::mutex> g(t->s->mu);
    *leaves = t->leaves;
    return ZKC_OK;
}

extern "C" int zkc_tree_refs(zkc_tree* t, size_t out[2]) {
    if (!t || !out) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_refs: bad argument");
    zkc_store* s = t->s;
    std::lock_guard<std::mutex> g(s->mu);
    out[0] = s->a.size() - 1 - s->free_refs.size(); out[1] = s->a.size();
    return ZKC_OK;
}

extern "C" int zkc_tree_stats(zkc_tree* t, double ms[2]) {
    if (!t || !ms) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_stats: bad argument");
    std::lock_guard<std::mutex> g(t->s->mu);
    ms[0] = t->s->ms[0]; ms[1] = t->s->ms[1];
    return ZKC_OK;
}

extern "C" int zkc_tree_get(zkc_tree* t, const void* keys, size_t n, void* values_out, int32_t* exists) {
    if (!t || (n && (!keys || !values_out || !exists))) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_get: bad argument");
    zkc_store* s = t->s;
    std::lock_guard<std::mutex> g(s->mu);
    if (s->broken) return zkc_fail(s->ctx, ZKC_ERR_HIP, BROKEN);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* key = (const uint8_t*)keys + 32 * i; uint8_t* v = (uint8_t*)values_out + 32 * i;
        const uint32_t l = find(t, key);
        exists[i] = l != 0;
        if (l) memcpy(v, leaf_val(s, l), 32); else memset(v, 0, 32);
    }
    return ZKC_OK;
}

extern "C" int zkc_tree_gen_proof(zkc_tree* t, const void* keys, size_t n, uint8_t root[32], void* siblings, int32_t* depths, int32_t* exists) {
    if (!t || !root || (n && (!keys || !exists))) return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_gen_proof: bad argument");
    return gen_proofs(t, "zkc_tree_gen_proof", keys, n, root, siblings, [&](size_t i, const uint8_t* key) {
        const uint32_t l = find(t, key);
        exists[i] = l != 0;
        if (depths) depths[i] = l ? (int32_t)t->s->path.size() : 0;
        return l != 0;
    });
}

// arbo GenProof for absent keys (circomlib SMTVerifier, fnc = 1): where the key's path ends -- an empty child (is_old0 = 1) or a leaf of another key (is_old0 = 0, its
// key and value) -- and the siblings of that path, laid out as zkc_tree_gen_proof lays them out
extern "C" int zkc_tree_gen_absence_proof(zkc_tree* t, const void* keys, size_t n, uint8_t root[32], void* siblings, int32_t* depths, void* old_keys, void* old_values,
                                          int32_t* is_old0, int32_t* status) {
    if (!t || !root || (n && (!keys || !old_keys || !old_values || !is_old0 || !status)))
        return zkc_fail(t ? t->s->ctx : nullptr, ZKC_ERR_BAD_ARG, "zkc_tree_gen_absence_proof: bad argument");
    return gen_proofs(t, "zkc_tree_gen_absence_proof", keys, n, root, siblings, [&](size_t i, const uint8_t* key) {
        zkc_store* s = t->s;
        uint8_t* ok = (uint8_t*)old_keys + 32 * i; uint8_t* ov = (uint8_t*)old_values + 32 * i;
        memset(ok, 0, 32); memset(ov, 0, 32); is_old0[i] = 0;
        if (depths) depths[i] = 0;
        if (!below_r(key)) { status[i] = ZKC_TREE_NOT_BELOW_R; return false; }
        const uint32_t r = descend(t, key);
        if (r && memcmp(leaf_key(s, r), key, 32) == 0) { status[i] = ZKC_TREE_KEY_EXISTS; return false; }
        status[i] = ZKC_TREE_OK;
        if (r) { memcpy(ok, leaf_key(s, r), 32); memcpy(ov, leaf_val(s, r), 32); } else is_old0[i] = 1;
        if (depths) depths[i] = (int32_t)s->path.size();
        return true;
    });
}

// zkc_census_inputs for n voters of two resident trees (include/zkcensus.h): the SIK and nullifier hashed on the GPU, availableWeight and both sibling lists from the trees.
// Either tree may be a snapshot, and both may be handles of one store (a census snapshot and its live tree): the stores' mutexes are taken, each once.
extern "C" int zkc_tree_census_inputs(zkc_tree* census, zkc_tree* sik, size_t n, const uint8_t election_id[64], const void* address, const void* password, const void* signature,
                                      const void* vote_weight, const void* vote_hash, void* inputs_out, void* d_inputs_out, uint8_t roots_out[64], int32_t* status) {
    zkc_store* cs = census ? census->s : nullptr; zkc_store* ss = sik ? sik->s : nullptr;
    zkc_ctx* ctx = cs ? cs->ctx : ss ? ss->ctx : nullptr;
    if (!census || !sik || cs->ctx != ss->ctx || cs->nLevels != ss->nLevels || cs->nLevels < 3 || n == 0 || n > (1u << 24) || !election_id || !address ||
        !password || !signature || !vote_weight || !vote_hash || (!inputs_out && !d_inputs_out) || !status)
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree_census_inputs: bad argument");
    const uint8_t *addr = (const uint8_t*)address, *pw = (const uint8_t*)password, *sg = (const uint8_t*)signature, *vw = (const uint8_t*)vote_weight, *vh = (const uint8_t*)vote_hash;
    if (!all_below_r(election_id, 2) || !all_below_r(addr, n) || !all_below_r(pw, n) || !all_below_r(sg, n) || !all_below_r(vw, n) || !all_below_r(vh, 2 * n))
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree_census_inputs: a value is not below the field order");
    std::unique_lock<std::mutex> gc(cs->mu, std::defer_lock), gs(ss->mu, std::defer_lock);
    if (cs == ss) gc.lock(); else std::lock(gc, gs);
    ZKC_LOCK(ctx);
    if (cs->broken || ss->broken) return zkc_fail(ctx, ZKC_ERR_HIP, BROKEN);
    const InputBlock L(cs->nLevels); const size_t nIn = L.nIn;
    if ((uint64_t)n * nIn >= (1ull << 32)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_tree_census_inputs: too many voters for 32-bit slots");
    // the trees: per voter its stored weight and stored SIK, its two sibling lists (kept per voter until the SIK check says whether it goes out)
    std::vector<uint8_t> avail(32 * n, 0), stored_sik(32 * n, 0);
    std::vector<uint2> pc, ps; std::vector<size_t> pc_end(n), ps_end(n);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* key = addr + 32 * i;
        status[i] = ZKC_TREE_OK;
        const uint32_t lc = find(census, key);
        if (!lc) status[i] = ZKC_TREE_NOT_IN_CENSUS;
        else { memcpy(&avail[32 * i], leaf_val(cs, lc), 32); sibling_pairs(cs, key, i * nIn + L.census_sibs, pc); }
        const uint32_t ls = find(sik, key);
        if (!ls) { if (!status[i]) status[i] = ZKC_TREE_NOT_IN_SIK; }
        else { memcpy(&stored_sik[32 * i], leaf_val(ss, ls), 32); sibling_pairs(ss, key, i * nIn + L.sik_sibs, ps); }
        pc_end[i] = pc.size(); ps_end[i] = ps.size();
    }
    // uploads: election id, address, password, signature, availableWeight, voteWeight, voteHash; then SIK and nullifier out; then the pairs (at most pc + ps + 12 n: the scalar slots of refused voters)
    const size_t o_eid = 0, o_addr = 256, o_pw = o_addr + align256(32 * n), o_sig = o_pw + align256(32 * n), o_av = o_sig + align256(32 * n), o_vw = o_av + align256(32 * n),
                 o_vh = o_vw + align256(32 * n), o_sik = o_vh + align256(64 * n), o_null = o_sik + align256(32 * n), o_pc = o_null + align256(32 * n),
                 o_ps = o_pc + align256(8 * (pc.size() + L.kScalars * n)), total = o_ps + 8 * ps.size() + 8;
    int rc;
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = stage(cs, total))) return rc;
    uint8_t* h = cs->h_stage; uint8_t* d = (uint8_t*)cs->d_stage;
    memcpy(h + o_eid, election_id, 64); memcpy(h + o_addr, addr, 32 * n); memcpy(h + o_pw, pw, 32 * n); memcpy(h + o_sig, sg, 32 * n);
    memcpy(h + o_av, avail.data(), 32 * n); memcpy(h + o_vw, vw, 32 * n); memcpy(h + o_vh, vh, 64 * n);
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d, h, o_sik, hipMemcpyHostToDevice, ctx->stream));
    auto D = [&](size_t o) { return (uint32_t*)(d + o); };
    const VoterArrays v{D(o_eid), D(o_addr), D(o_pw), D(o_sig), D(o_av), D(o_vw), D(o_vh), D(o_sik), D(o_null)};
    if ((rc = zkc_voter_hashes(ctx, v, n))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(h + o_sik, d + o_sik, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    // the voters that go out: their sibling pairs; the ones that do not: their twelve scalar slots zeroed again, from val[0] = 0 (their sibling slots stay zero)
    uint2* hp = (uint2*)(h + o_pc); uint2* hq = (uint2*)(h + o_ps); size_t np = 0, nq = 0;
    for (size_t i = 0; i < n; i++) {
        if (!status[i] && memcmp(h + o_sik + 32 * i, &stored_sik[32 * i], 32) != 0) status[i] = ZKC_TREE_SIK_MISMATCH;
        if (status[i]) { for (size_t k = 0; k < L.kScalars; k++) hp[np++] = make_uint2((uint32_t)(i * nIn + k), 0); continue; }
        for (size_t j = i ? pc_end[i - 1] : 0; j < pc_end[i]; j++) hp[np++] = pc[j];
        for (size_t j = i ? ps_end[i - 1] : 0; j < ps_end[i]; j++) hq[nq++] = ps[j];
    }
    if (np) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d + o_pc, h + o_pc, 8 * np, hipMemcpyHostToDevice, ctx->stream));
    if (nq) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d + o_ps, h + o_ps, 8 * nq, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* d_out = (uint32_t*)d_inputs_out;
    if (!d_out) { if ((rc = zkc_ensure(ctx, &cs->d_out, &cs->d_out_sz, 32 * n * nIn))) return rc; d_out = (uint32_t*)cs->d_out; }
    return zkc_write_input_blocks(ctx, v, n, L, cs->d_val, census->root, ss->d_val, sik->root, (const uint2*)(d + o_pc), np, (const uint2*)(d + o_ps), nq, d_out, inputs_out,
                                  roots_out);
}
