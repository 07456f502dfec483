// zkc_census.hip -- f1: the census / voter generator in native code.
//
// The reference builds its test census with arbo (internal/helpers.go:36-85 GenTree: arbo.NewTree{HashFunctionPoseidon}, Add per voter, GenProof, UnpackSiblings, zero padding
// to nLevels + 1) and fills the circuit inputs from it (internal/inputs.go:33-98 MockInputs; ts_inputs/src/inputs.ts:38-88).  Rounds 1-4 did that in Python over a batched GPU
// Poseidon: 10 s for the 8 192-voter census of BASELINE configs[2..3], most of it Python lists and one host round trip per tree level.  Here: the trie over the keys is split
// on the host in C++ (sort by path, binary-search the split of every node: microseconds per thousand leaves), every hash runs on the GPU -- leaves in one launch, inner nodes
// depth by depth, bottom-up (zkc_hash_levels, the launches the resident tree of zkc_tree.hip makes for its dirty nodes), values never leaving HBM -- and every voter's sibling list is scattered straight into its 334 x 32-byte input block on the device.
//
// arbo tree semantics (pinned by the reference's one arbo-built path, tests/test_gpu_census.py): leaf = H(key, value, 1); node = H(left, right); path bit i =
// bit i (LSB first) of the key; an empty subtree is 0; a subtree holding a single leaf is that leaf's hash (a leaf sits at the first depth where its path is unique).
// A static build (all leaves at once), not arbo's incremental Add: the tree is the same, the order of insertion does not matter to a Merkle radix tree.
#include "zkc_census_host.h"
#include "zkc_kernels.h"
#include <algorithm>
#include <array>
#include <vector>

using namespace zkc;

namespace {
constexpr uint32_t WAVE = 64;                // a depth with at most this many nodes to hash is narrow

// the radix trie over n keys: the inner nodes as (node, left, right) triples of references grouped by depth, deepest first, which is what zkc_hash_levels takes and
// what the resident tree uploads per batch; for every leaf the (depth, sibling reference) pairs of its path.
// References index the tree's value array: 0 = empty, 1 + i = leaf i, 1 + n + j = inner node j.
struct Trie {
    size_t n = 0; std::vector<uint32_t> trip, off{0};                                    // the k-th deepest depth is triples off[k] .. off[k + 1]; off.back() = their number
    uint32_t root = 0;
    size_t nodes() const { return trip.size() / 3; }
    struct Sib { uint32_t leaf, level, ref; }; std::vector<Sib> sibs;                    // non-zero siblings only
    std::vector<int32_t> leaf_depth;                                                       // 1 + the deepest level at which leaf i has an inner node above it (0: alone in the tree)
};
inline uint64_t bitrev64(uint64_t x) {
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1); x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4); return __builtin_bswap64(x);
}
// false: two keys agree on their first max_levels path bits (arbo: the tree cannot hold both)
bool trie_build(const uint8_t* keys, size_t n, int max_levels, Trie& t, std::string& err) {
    t = Trie(); t.n = n; t.leaf_depth.assign(n, 0);
    if (n == 0) return true;
    // leaves in path order: sort by the key read bit by bit from the LSB, i.e. by the bit-reversed 256-bit key
    std::vector<std::array<uint64_t, 4>> rk(n); std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) { uint64_t w[4]; memcpy(w, keys + 32 * i, 32); for (int k = 0; k < 4; k++) rk[i][k] = bitrev64(w[k]); idx[i] = (uint32_t)i; }
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return rk[a] < rk[b]; });
    for (size_t i = 0; i + 1 < n; i++) if (rk[idx[i]] == rk[idx[i + 1]]) { err = "zkc census: duplicate key"; return false; }
    std::vector<uint32_t> left, right, depth;                          // per inner node j, in the order the split makes them
    // work list: the range [lo, hi) of idx whose subtree reference becomes child `side` of `node` (child references go in through indices, not pointers: the vectors grow)
    struct Pend { uint32_t lo, hi, depth, node, side; };
    std::vector<Pend> pend; pend.push_back({0, (uint32_t)n, 0, 0xffffffffu, 0});
    auto ref_of = [&](uint32_t lo, uint32_t hi, uint32_t d, bool& ok) -> uint32_t {
        if (hi == lo) return 0;
        if (hi - lo == 1) return 1 + idx[lo];
        if ((int)d >= max_levels) { ok = false; return 0; }
        const uint32_t nid = (uint32_t)left.size();
        left.push_back(0); right.push_back(0); depth.push_back(d);
        // the split: first position whose key has bit `d` set (within the range every key shares the bits below `d`, so the range is partitioned)
        uint32_t a = lo, b = hi; while (a < b) { const uint32_t m = (a + b) / 2; if (key_bit(keys + 32 * (size_t)idx[m], (int)d)) b = m; else a = m + 1; }
        pend.push_back({lo, a, d + 1, nid, 0}); pend.push_back({a, hi, d + 1, nid, 1});
        return 1 + (uint32_t)n + nid;
    };
    std::vector<std::array<uint32_t, 3>> range;                        // per node: lo, mid, hi
    bool ok = true;
    for (size_t q = 0; q < pend.size() && ok; q++) {
        const Pend p = pend[q];
        const size_t before = left.size();
        const uint32_t r = ref_of(p.lo, p.hi, p.depth, ok);
        if (left.size() > before) { const Pend& l = pend[pend.size() - 2]; range.push_back({l.lo, l.hi, p.hi}); }
        if (p.node == 0xffffffffu) t.root = r; else (p.side ? right : left)[p.node] = r;
    }
    if (!ok) { err = "zkc census: two keys collide on the first " + std::to_string(max_levels) + " bits of their paths"; return false; }
    const size_t nn = left.size();
    uint32_t D = 0; for (size_t j = 0; j < nn; j++) D = std::max(D, depth[j] + 1);
    // the triples by depth, deepest first: depth d is the (D - 1 - d)-th deepest
    t.off.assign(D + 1, 0);
    for (size_t j = 0; j < nn; j++) t.off[D - depth[j]]++;
    for (uint32_t k = 0; k < D; k++) t.off[k + 1] += t.off[k];
    t.trip.resize(3 * nn);
    { std::vector<uint32_t> fill(t.off.begin(), t.off.end() - 1);
      for (size_t j = 0; j < nn; j++) { uint32_t* q = &t.trip[3 * (size_t)fill[D - 1 - depth[j]]++]; q[0] = 1 + (uint32_t)n + (uint32_t)j; q[1] = left[j]; q[2] = right[j]; } }
    // sibling lists: the members of node j's left range see its right child, and the other way round (zero siblings are what the zeroed block already holds)
    for (size_t j = 0; j < nn; j++) {
        const uint32_t lo = range[j][0], mid = range[j][1], hi = range[j][2], d = depth[j];
        for (uint32_t k = lo; k < hi; k++) {
            const uint32_t leaf = idx[k], sib = k < mid ? right[j] : left[j];
            if (sib) t.sibs.push_back({leaf, d, sib});
            if ((int32_t)d + 1 > t.leaf_depth[leaf]) t.leaf_depth[leaf] = (int32_t)d + 1;
        }
    }
    return true;
}
// `bytes` of host memory into a fresh device buffer, on ctx->stream (the source stays alive until the stream is next synchronised)
int upload(zkc_ctx* ctx, DevBuf& d, const void* src, size_t bytes) {
    int rc; if ((rc = d.alloc(ctx, bytes))) return rc;
    if (bytes) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return ZKC_OK;
}
// val (device, (1 + n + nodes) x 32 B): leaf hashes from (d_keys, d_values), then the inner nodes from the uploaded triples and offsets of t; all on ctx->stream.
// The triples' references are below 1 + n + nodes by construction (trie_build).
int tree_hash(zkc_ctx* ctx, const Trie& t, const uint32_t* d_trip, const uint32_t* d_off, const uint32_t* d_keys, const uint32_t* d_values, uint32_t* d_val) {
    const size_t n = t.n;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_val, 0, 32, ctx->stream));
    if (n) hipLaunchKernelGGL(zkc_census_hash, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, ctx->ptab, 0, d_keys, d_values, (const uint32_t*)nullptr, d_val + 8, n);
    zkc_hash_levels(ctx, d_trip, d_off, t.off.data(), (int)t.off.size() - 1, (uint32_t)t.nodes(), d_val);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    return ZKC_OK;
}
// the sibling lists as (destination element, value reference) pairs, on the host in `h` and uploaded to `d`: element = 32-byte slot of the output array; leaf i's
// level-l sibling goes to i * stride + base + l.  `h` is pageable: the caller keeps it until the stream is synchronised.
int upload_sibling_pairs(zkc_ctx* ctx, const Trie& t, size_t stride, size_t base, std::vector<uint2>& h, DevBuf& d) {
    h.resize(t.sibs.size());
    for (size_t k = 0; k < t.sibs.size(); k++) { const size_t dst = (size_t)t.sibs[k].leaf * stride + base + t.sibs[k].level; if (dst >> 32) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc census: too many voters for 32-bit slots"); h[k] = make_uint2((uint32_t)dst, t.sibs[k].ref); }
    return upload(ctx, d, h.data(), h.size() * sizeof(uint2));
}
}  // namespace

void zkc_hash_levels(zkc_ctx* ctx, const uint32_t* d_trip, const uint32_t* d_off, const uint32_t* h_off, int D, uint32_t M, uint32_t* d_val) {
    for (int k = 0; k < D;) {                        // k-th deepest depth
        const uint32_t c = h_off[k + 1] - h_off[k];
        if (c > WAVE) {
            hipLaunchKernelGGL(zkc_tree_level, dim3((c + 63) / 64), dim3(64), 0, ctx->stream, ctx->ptab, d_trip + 3 * (size_t)h_off[k], c, d_val);
            k++;
        } else {
            int j = k; while (j < D && h_off[j + 1] - h_off[j] <= WAVE) j++;
            hipLaunchKernelGGL(zkc_tree_narrow, dim3(1), dim3(64), 0, ctx->stream, ctx->ptab, d_trip, d_off + k, (uint32_t)(j - k), M, d_val);
            k = j;
        }
    }
}

int zkc_voter_hashes(zkc_ctx* ctx, const VoterArrays& v, size_t n) {
    const unsigned g64 = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(zkc_census_hash, dim3(g64), dim3(64), 0, ctx->stream, ctx->ptab, 1, v.address, v.password, v.signature, v.sik, n);          // census.circom:74-77
    hipLaunchKernelGGL(zkc_census_hash, dim3(g64), dim3(64), 0, ctx->stream, ctx->ptab, 2, v.signature, v.password, v.eid, v.nullifier, n);        // :105-109
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    return ZKC_OK;
}

int zkc_write_input_blocks(zkc_ctx* ctx, const VoterArrays& v, size_t n, const InputBlock& L, const uint32_t* val_c, uint32_t root_c, const uint32_t* val_s, uint32_t root_s,
                           const uint2* pairs_c, size_t np, const uint2* pairs_s, size_t nq, uint32_t* d_out, void* inputs_out, uint8_t* roots_out) {
    const size_t bytes = 32 * n * L.nIn;
    const uint32_t* croot = val_c + 8 * (size_t)root_c; const uint32_t* sroot = val_s + 8 * (size_t)root_s;
    ZKC_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, bytes, ctx->stream));
    hipLaunchKernelGGL(zkc_census_scalars, dim3((unsigned)((L.kScalars * n + 255) / 256)), dim3(256), 0, ctx->stream, v.eid, v.nullifier, v.avail, v.vote_hash, sroot, croot,
                       v.address, v.password, v.signature, v.vote_weight, n, (int)L.nIn, d_out);
    if (np) hipLaunchKernelGGL(zkc_census_scatter, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, val_c, pairs_c, np, d_out);
    if (nq) hipLaunchKernelGGL(zkc_census_scatter, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, val_s, pairs_s, nq, d_out);
    ZKC_HIP_CHECK(ctx, hipGetLastError());
    if (inputs_out) ZKC_HIP_CHECK(ctx, hipMemcpyAsync(inputs_out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (roots_out) { ZKC_HIP_CHECK(ctx, hipMemcpyAsync(roots_out, croot, 32, hipMemcpyDeviceToHost, ctx->stream));
                     ZKC_HIP_CHECK(ctx, hipMemcpyAsync(roots_out + 32, sroot, 32, hipMemcpyDeviceToHost, ctx->stream)); }
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return ZKC_OK;
}

// One tree.  keys, values: n x 32 B, host, standard form, < r, keys distinct.  root: 32 B.  siblings (may be NULL): n x (nLevels + 1) x 32 B, leaf i's sibling at level l in
// slot i (nLevels + 1) + l, zero-padded the way internal/helpers.go:72-79 pads arbo's packed siblings.  depths (may be NULL): per leaf the number of levels above it.
extern "C" int zkc_smt_build(zkc_ctx* ctx, const void* keys, const void* values, size_t n, int nLevels, uint8_t root[32], void* siblings, int32_t* depths) {
    if (!ctx || !keys || !values || !root || n == 0 || n > (1u << 28) || nLevels < 1 || nLevels > 253) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_build: bad argument");
    if (!all_below_r(keys, n) || !all_below_r(values, n)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_smt_build: a key or value is not below the field order");
    Trie t; std::string err;
    if (!trie_build((const uint8_t*)keys, n, nLevels, t, err)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, err);
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<uint2> hp;                                             // the pairs' host copy: outlives the device buffers, which are freed first
    DevBuf d_trip, d_off, dk, dv, dval, dout, pairs; int rc;
    const size_t stride = (size_t)nLevels + 1;
    if ((rc = upload(ctx, d_trip, t.trip.data(), 4 * t.trip.size())) || (rc = upload(ctx, d_off, t.off.data(), 4 * t.off.size())) || (rc = upload(ctx, dk, keys, 32 * n)) ||
        (rc = upload(ctx, dv, values, 32 * n)) || (rc = dval.alloc(ctx, 32 * (1 + n + t.nodes())))) return rc;
    if ((rc = tree_hash(ctx, t, d_trip.as<uint32_t>(), d_off.as<uint32_t>(), dk.as<uint32_t>(), dv.as<uint32_t>(), dval.as<uint32_t>()))) return rc;
    ZKC_HIP_CHECK(ctx, hipMemcpyAsync(root, dval.as<uint8_t>() + 32 * (size_t)t.root, 32, hipMemcpyDeviceToHost, ctx->stream));
    if (siblings) {
        if ((rc = dout.alloc(ctx, 32 * n * stride))) return rc;
        ZKC_HIP_CHECK(ctx, hipMemsetAsync(dout.p, 0, 32 * n * stride, ctx->stream));
        if ((rc = upload_sibling_pairs(ctx, t, stride, 0, hp, pairs))) return rc;
        if (!hp.empty()) hipLaunchKernelGGL(zkc_census_scatter, dim3((unsigned)((hp.size() + 255) / 256)), dim3(256), 0, ctx->stream, dval.as<uint32_t>(), pairs.as<uint2>(), hp.size(), dout.as<uint32_t>());
        ZKC_HIP_CHECK(ctx, hipGetLastError());
        ZKC_HIP_CHECK(ctx, hipMemcpyAsync(siblings, dout.p, 32 * n * stride, hipMemcpyDeviceToHost, ctx->stream));
    }
    ZKC_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (depths) memcpy(depths, t.leaf_depth.data(), 4 * n);
    return ZKC_OK;
}

// The circuit inputs of a whole census (internal/inputs.go:33-98 MockInputs for every voter of one election): from the voters' own data -- address, password, signature,
// available and cast weight, vote hash -- the SIK H(address, password, signature) and the nullifier H(signature, password, electionId) of every voter, the census tree
// (address -> available weight) and the SIK tree (address -> SIK), both roots, and every voter's two sibling lists, assembled into n blocks of zkc_circuit_n_inputs(nLevels)
// x 32 B in census.circom:51-67 order.  All arrays n x 32 B (vote_hash n x 2 x 32 B, election_id 2 x 32 B), host, standard form, < r.  The blocks go to inputs_out (host)
// and / or d_inputs_out (device: what zkc_fullprove_batch_dev / zkc_batch_begin take), either may be NULL.  roots_out (may be NULL): census root, SIK root, 2 x 32 B.
extern "C" int zkc_census_inputs(zkc_ctx* ctx, size_t n, int nLevels, const uint8_t election_id[64], const void* address, const void* password, const void* signature,
                                 const void* available_weight, const void* vote_weight, const void* vote_hash, void* inputs_out, void* d_inputs_out, uint8_t* roots_out) {
    if (!ctx || !election_id || !address || !password || !signature || !available_weight || !vote_weight || !vote_hash || n == 0 || n > (1u << 24) || nLevels < 3 || nLevels > 253 || (!inputs_out && !d_inputs_out))
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_census_inputs: bad argument");
    if (!all_below_r(election_id, 2) || !all_below_r(address, n) || !all_below_r(password, n) || !all_below_r(signature, n) || !all_below_r(available_weight, n) || !all_below_r(vote_weight, n) || !all_below_r(vote_hash, 2 * n))
        return zkc_fail(ctx, ZKC_ERR_BAD_ARG, "zkc_census_inputs: a value is not below the field order");
    Trie t; std::string err;
    if (!trie_build((const uint8_t*)address, n, nLevels, t, err)) return zkc_fail(ctx, ZKC_ERR_BAD_ARG, err);      // both trees are keyed by the address: one trie
    ZKC_LOCK(ctx);
    ZKC_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const InputBlock L(nLevels);
    std::vector<uint2> hc, hs;                                         // the pairs' host copies: they outlive the device buffers, which are freed first
    DevBuf d_trip, d_off, d_eid, d_addr, d_pw, d_sig, d_av, d_vw, d_vh, d_sik, d_null, val_c, val_s, own_out, pairs_c, pairs_s; int rc;
    if ((rc = upload(ctx, d_trip, t.trip.data(), 4 * t.trip.size())) || (rc = upload(ctx, d_off, t.off.data(), 4 * t.off.size())) || (rc = upload(ctx, d_eid, election_id, 64)) ||
        (rc = upload(ctx, d_addr, address, 32 * n)) || (rc = upload(ctx, d_pw, password, 32 * n)) || (rc = upload(ctx, d_sig, signature, 32 * n)) ||
        (rc = upload(ctx, d_av, available_weight, 32 * n)) || (rc = upload(ctx, d_vw, vote_weight, 32 * n)) || (rc = upload(ctx, d_vh, vote_hash, 64 * n))) return rc;
    const size_t nval = 1 + n + t.nodes();
    if ((rc = d_sik.alloc(ctx, 32 * n)) || (rc = d_null.alloc(ctx, 32 * n)) || (rc = val_c.alloc(ctx, 32 * nval)) || (rc = val_s.alloc(ctx, 32 * nval))) return rc;
    uint32_t* d_out = (uint32_t*)d_inputs_out;
    if (!d_out) { if ((rc = own_out.alloc(ctx, 32 * n * L.nIn))) return rc; d_out = own_out.as<uint32_t>(); }
    const VoterArrays v{d_eid.as<uint32_t>(), d_addr.as<uint32_t>(), d_pw.as<uint32_t>(), d_sig.as<uint32_t>(), d_av.as<uint32_t>(), d_vw.as<uint32_t>(), d_vh.as<uint32_t>(),
                        d_sik.as<uint32_t>(), d_null.as<uint32_t>()};
    if ((rc = zkc_voter_hashes(ctx, v, n))) return rc;
    if ((rc = tree_hash(ctx, t, d_trip.as<uint32_t>(), d_off.as<uint32_t>(), v.address, v.avail, val_c.as<uint32_t>()))) return rc;      // census tree: address -> available weight
    if ((rc = tree_hash(ctx, t, d_trip.as<uint32_t>(), d_off.as<uint32_t>(), v.address, v.sik, val_s.as<uint32_t>()))) return rc;        // SIK tree: address -> SIK
    if ((rc = upload_sibling_pairs(ctx, t, L.nIn, L.census_sibs, hc, pairs_c)) || (rc = upload_sibling_pairs(ctx, t, L.nIn, L.sik_sibs, hs, pairs_s))) return rc;
    return zkc_write_input_blocks(ctx, v, n, L, val_c.as<uint32_t>(), t.root, val_s.as<uint32_t>(), t.root, pairs_c.as<uint2>(), hc.size(), pairs_s.as<uint2>(), hs.size(),
                                  d_out, inputs_out, roots_out);
}
