"""Synthetic census / voter generator: arbo-compatible Poseidon sparse Merkle trees with sibling
extraction, SIK and nullifier derivation.  Mirrors internal/helpers.go:36-85 (GenTree: arbo.NewTree{Poseidon}, Add,
GenProof, UnpackSiblings, zero padding) and internal/inputs.go:33-98 (MockInputs); encodings per
ts_inputs/src/inputs.ts:55-88.  All hashing runs on the GPU through zkc_poseidon_batch, one call per tree level.

arbo tree semantics: leaf = H(key, value, 1); node = H(left, right); path bit i = bit i (LSB first) of
the key; an empty subtree is 0; a subtree holding a single leaf is that leaf's hash (the leaf sits at the first level
where its path is unique)."""
import ctypes
import hashlib
from .inputs import R_MOD, bytes_to_arbo  # noqa: F401 (bytes_to_arbo is part of this module's surface)

ELECTION_ID_HEX = '7faeab7a7d250527d614e952ae8e446825bd1124c6def410844c7c383d1519a6'   # internal/inputs.go:60, example.ts:341


def poseidon_batch(ctx, rows):
    """rows: list of equal-length tuples of ints (2, 3 or 4 inputs) -> list of ints, hashed on the GPU."""
    if not rows:
        return []
    n = len(rows[0])
    buf = b''.join(int(x).to_bytes(32, 'little') for r in rows for x in r)
    out = ctypes.create_string_buffer(32 * len(rows))
    ctx._check(ctx._lib.zkc_poseidon_batch(ctx._h, n, buf, len(rows), out))
    raw = out.raw
    return [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(len(rows))]


class SparseMerkleTree:
    """Static build over a list of (key, value) pairs; records for every leaf its sibling path."""

    def __init__(self, ctx, keys, values, max_levels=160):
        assert len(set(keys)) == len(keys), 'duplicate keys'
        self.n = len(keys)
        leaf_hash = poseidon_batch(ctx, [(k, v, 1) for k, v in zip(keys, values)])
        # top-down split into the radix trie; node = (depth, members) ; children by key bit `depth`
        nodes = []            # (depth, left_id, right_id, members)   id -1 = empty, -(2+i) = single leaf i
        def ref(members, depth):
            if not members:
                return -1
            if len(members) == 1:
                return -(2 + members[0])
            if depth >= max_levels:
                raise ValueError('keys collide on the first %d bits' % max_levels)
            nid = len(nodes); nodes.append(None)
            l = [m for m in members if not (keys[m] >> depth) & 1]; r = [m for m in members if (keys[m] >> depth) & 1]
            nodes[nid] = [depth, None, None, members]
            pending.append((nid, l, r, depth))
            return nid
        pending = []
        import sys
        root_ref = ref(list(range(self.n)), 0)
        while pending:                                   # iterative expansion (no recursion depth issues)
            nid, l, r, depth = pending.pop()
            nodes[nid][1] = ref(l, depth + 1); nodes[nid][2] = ref(r, depth + 1)
        # bottom-up hashing, one GPU batch per depth
        val = {}
        def value_of(rid):
            return 0 if rid == -1 else leaf_hash[-rid - 2] if rid < -1 else val[rid]
        by_depth = {}
        for nid, nd in enumerate(nodes):
            by_depth.setdefault(nd[0], []).append(nid)
        for depth in sorted(by_depth, reverse=True):
            ids = by_depth[depth]
            hs = poseidon_batch(ctx, [(value_of(nodes[i][1]), value_of(nodes[i][2])) for i in ids])
            for i, h in zip(ids, hs):
                val[i] = h
        self.root = value_of(root_ref)
        # sibling paths
        self.siblings = [[] for _ in range(self.n)]
        for nd in nodes:
            depth, lref, rref, members = nd
            lv, rv = value_of(lref), value_of(rref)
            for m in members:
                sib = lv if (keys[m] >> depth) & 1 else rv
                path = self.siblings[m]
                while len(path) < depth:
                    path.append(0)
                if len(path) == depth:
                    path.append(sib)
                else:
                    path[depth] = sib
        for p in self.siblings:                          # drop trailing zeros (GenProof packs only used levels)
            while p and p[-1] == 0:
                p.pop()


def _voter_data(n_voters, election_id_hex):
    """the deterministic raw data of the synthetic census (addresses, passwords, signatures, weights)."""
    eid = bytes_to_arbo(bytes.fromhex(election_id_hex))
    u32 = lambda i: int(i).to_bytes(4, 'little')
    address = [int.from_bytes(hashlib.sha256(b'addr' + u32(i)).digest()[:20], 'little') for i in range(n_voters)]
    password = [int.from_bytes(hashlib.sha256(b'pw' + u32(i)).digest()[:11], 'big') % R_MOD for i in range(n_voters)]
    signature = [int.from_bytes(hashlib.sha256(b'sigA' + u32(i)).digest() + hashlib.sha256(b'sigB' + u32(i)).digest(), 'big') % R_MOD
                 for i in range(n_voters)]
    avail = [1 + (i % 100) for i in range(n_voters)]
    return eid, address, password, signature, avail


def census_inputs(ctx, election_id, address, password, signature, available_weight, vote_weight, vote_hash, nLevels=160, d_out_ptr=None):
    """[r5] The native census builder (zkc_census_inputs, csrc/zkc_census.hip): every voter's circuit inputs -- SIK, nullifier, both trees, roots, sibling lists -- as flat
    334 x 32-byte blocks, all hashing and the sibling scatter on the GPU.  Lists of ints (vote_hash: pairs).  Returns (flat bytes, census root, sik root); with d_out_ptr
    the blocks are ALSO left at that device address."""
    n = len(address)
    le = lambda xs: b''.join(int(x).to_bytes(32, 'little') for x in xs)
    nIn = 12 + 2 * (nLevels + 1)
    out = ctypes.create_string_buffer(32 * nIn * n); roots = ctypes.create_string_buffer(64)
    ctx._check(ctx._lib.zkc_census_inputs(ctx._h, n, nLevels, le(election_id), le(address), le(password), le(signature), le(available_weight), le(vote_weight),
                                          le(x for pair in vote_hash for x in pair), ctypes.cast(out, ctypes.c_void_p), d_out_ptr, roots))
    return out.raw, int.from_bytes(roots.raw[:32], 'little'), int.from_bytes(roots.raw[32:], 'little')


def synthetic_census_flat(ctx, n_voters, nLevels=160, election_id_hex=ELECTION_ID_HEX, d_out_ptr=None):
    """The synthetic census of SURVEY.md 8(d) config 3 through the native builder: (flat input blocks, census root, sik root).  8 192 voters in well under a second
    (the Python builder below, kept as a cross-check, takes ten)."""
    eid, address, password, signature, avail = _voter_data(n_voters, election_id_hex)
    vh = [bytes_to_arbo(a.to_bytes((a.bit_length() + 7) // 8 or 1, 'big')) for a in avail]                  # internal/inputs.go:81
    return census_inputs(ctx, eid, address, password, signature, avail, [1] * n_voters, vh, nLevels, d_out_ptr)


class FlatVoters:
    """The 12-key input objects of a flat block array, made on demand (a decimal string per value costs more than the GPU spends on the voter's proof: only the voters
    somebody looks at are converted)."""

    def __init__(self, flat, nLevels=160):
        self.flat, self.nLevels, self.nIn = flat, nLevels, 12 + 2 * (nLevels + 1)

    def __len__(self):
        return len(self.flat) // (32 * self.nIn)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        b = self.flat[32 * self.nIn * i:32 * self.nIn * (i + 1)]
        v = [str(int.from_bytes(b[32 * k:32 * k + 32], 'little')) for k in range(self.nIn)]
        n = self.nLevels + 1
        return {'electionId': v[0:2], 'nullifier': v[2], 'availableWeight': v[3], 'voteHash': v[4:6], 'sikRoot': v[6], 'censusRoot': v[7], 'address': v[8], 'password': v[9],
                'signature': v[10], 'voteWeight': v[11], 'censusSiblings': v[12:12 + n], 'sikSiblings': v[12 + n:12 + 2 * n]}


def synthetic_census(ctx, n_voters, nLevels=160, election_id_hex=ELECTION_ID_HEX):
    """deterministic census of n_voters as a sequence of 12-key circuit input objects (decimal strings, siblings zero-padded to nLevels + 1 like
    internal/inputs.go:52,72).  [r5] Built by the native builder (zkc_census_inputs); the objects are made on demand from its flat blocks (FlatVoters: indexing and slicing give
    dicts / lists of dicts, `.flat` the blocks themselves).  synthetic_census_py is the Python builder of rounds 1-4, kept as the cross-check
    (tests/test_gpu_census.py: byte-equal over whole censuses)."""
    flat, _, _ = synthetic_census_flat(ctx, n_voters, nLevels, election_id_hex)
    return FlatVoters(flat, nLevels)


def synthetic_census_py(ctx, n_voters, nLevels=160, election_id_hex=ELECTION_ID_HEX):
    """The same census through SparseMerkleTree above (Python lists, one batched GPU Poseidon call per tree level): ten seconds for 8 192 voters."""
    eid, address, password, signature, avail = _voter_data(n_voters, election_id_hex)
    sik = poseidon_batch(ctx, list(zip(address, password, signature)))                     # census.circom:74-77
    nullifier = poseidon_batch(ctx, [(s, p, int(eid[0]), int(eid[1])) for s, p in zip(signature, password)])   # :105-109
    census = SparseMerkleTree(ctx, address, avail, nLevels)
    siktree = SparseMerkleTree(ctx, address, sik, nLevels)
    pad = lambda s: [str(x) for x in s] + ['0'] * (nLevels + 1 - len(s))
    out = []
    for i in range(n_voters):
        vh = bytes_to_arbo(avail[i].to_bytes((avail[i].bit_length() + 7) // 8 or 1, 'big'))   # internal/inputs.go:81
        out.append({
            'electionId': list(eid), 'nullifier': str(nullifier[i]), 'availableWeight': str(avail[i]), 'voteHash': vh,
            'sikRoot': str(siktree.root), 'censusRoot': str(census.root),
            'address': str(address[i]), 'password': str(password[i]), 'signature': str(signature[i]), 'voteWeight': '1',
            'censusSiblings': pad(census.siblings[i]), 'sikSiblings': pad(siktree.siblings[i]),
        })
    return out


def deep_voters(ctx, n_voters, nLevels=160, depth=None, seed=160):
    """n_voters valid voters whose leaves sit `depth` levels down BOTH trees (default nLevels: the bottom), every sibling on the way non-zero: no level of
    their witnesses equals the voter-independent empty-subtree template, so the prover's constant folding removes nothing -- the worst case a real census
    cannot produce (8 192 voters put leaves 13-17 levels deep) but a foreign or adversarial witness can.  Each voter gets its own pair of roots: the
    proofs are independent anyway.  Hashing on the GPU, one zkc_poseidon_batch call per level."""
    import random
    rng = random.Random(seed); depth = nLevels if depth is None else depth
    eid = bytes_to_arbo(bytes.fromhex(ELECTION_ID_HEX))
    address = [rng.getrandbits(160) for _ in range(n_voters)]
    password = [rng.getrandbits(88) for _ in range(n_voters)]
    signature = [rng.getrandbits(512) % R_MOD for _ in range(n_voters)]
    avail = [1 + rng.randrange(100) for _ in range(n_voters)]
    sik = poseidon_batch(ctx, list(zip(address, password, signature)))
    nullifier = poseidon_batch(ctx, [(s, p, int(eid[0]), int(eid[1])) for s, p in zip(signature, password)])

    def climb(values):
        sibs = [[rng.randrange(1, R_MOD) for _ in range(depth)] for _ in range(n_voters)]
        cur = poseidon_batch(ctx, [(k, v, 1) for k, v in zip(address, values)])
        for lvl in range(depth - 1, -1, -1):
            cur = poseidon_batch(ctx, [(sibs[v][lvl], cur[v]) if (address[v] >> lvl) & 1 else (cur[v], sibs[v][lvl]) for v in range(n_voters)])
        return cur, sibs
    croot, csib = climb(avail); sroot, ssib = climb(sik)
    pad = lambda s: [str(x) for x in s] + ['0'] * (nLevels + 1 - len(s))
    return [{'electionId': list(eid), 'nullifier': str(nullifier[i]), 'availableWeight': str(avail[i]), 'voteHash': ['1', '2'], 'sikRoot': str(sroot[i]),
             'censusRoot': str(croot[i]), 'address': str(address[i]), 'password': str(password[i]), 'signature': str(signature[i]), 'voteWeight': '1',
             'censusSiblings': pad(csib[i]), 'sikSiblings': pad(ssib[i])} for i in range(n_voters)]


def _le(xs):
    """ints -> concatenated 32-byte little-endian words (bytes pass through unchanged)"""
    return bytes(xs) if isinstance(xs, (bytes, bytearray)) else b''.join(int(x).to_bytes(32, 'little') for x in xs)


def smt_build(ctx, keys, values, nLevels=160, siblings=True):
    """One static tree over (key, value) pairs (zkc_smt_build): (root, siblings bytes n x (nLevels + 1) x 32 or None, depths)."""
    kb, vb = _le(keys), _le(values)
    n = len(kb) // 32
    root = ctypes.create_string_buffer(32); dep = (ctypes.c_int32 * n)()
    sib = ctypes.create_string_buffer(32 * n * (nLevels + 1)) if siblings else None
    ctx._check(ctx._lib.zkc_smt_build(ctx._h, kb, vb, n, nLevels, root, sib, dep))
    return int.from_bytes(root.raw, 'little'), (sib.raw if siblings else None), list(dep)


SMT_VALID, SMT_ROOT_MISMATCH, SMT_NOT_BELOW_R, SMT_LAST_SIBLING, SMT_KEY_PRESENT, SMT_OFF_PATH = range(6)   # ZKC_SMT_*: the verdicts of check_proofs / check_absence


def check_proofs(ctx, keys, values, siblings, roots, nLevels=160):
    """arbo CheckProof over a batch on the GPU (zkc_smt_check_proofs): one SMT_* verdict per proof.  keys, values: ints or packed 32-byte words; siblings: bytes,
    n x (nLevels + 1) x 32, zero-padded as smt_build and CensusTree.gen_proof return them; roots: one int shared by every proof, or a list of n ints (one root per proof)."""
    kb, vb = _le(keys), _le(values)
    n = len(kb) // 32
    per = isinstance(roots, (list, tuple))
    rb = _le(roots) if per else _le([roots])
    assert len(vb) == len(kb) and len(siblings) == 32 * n * (nLevels + 1) and (not per or len(rb) == len(kb)), 'keys, values, siblings and roots differ in length'
    st = (ctypes.c_int32 * max(n, 1))()
    ctx._check(ctx._lib.zkc_smt_check_proofs(ctx._h, int(nLevels), n, kb, vb, siblings if isinstance(siblings, bytes) else bytes(siblings), rb, int(per), st))
    return list(st)[:n]


def check_absence(ctx, keys, old_keys, old_values, is_old0, siblings, roots, nLevels=160):
    """Exclusion proofs checked in a batch on the GPU (zkc_smt_check_absence; circomlib SMTVerifier with fnc = 1): one SMT_* verdict per proof.  keys, old_keys,
    old_values: ints or packed 32-byte words; is_old0: n ints (0 or 1); siblings and roots as for check_proofs -- the outputs of CensusTree.gen_absence_proof."""
    kb, okb, ovb = _le(keys), _le(old_keys), _le(old_values)
    n = len(kb) // 32
    per = isinstance(roots, (list, tuple))
    rb = _le(roots) if per else _le([roots])
    assert len(okb) == len(ovb) == len(kb) and len(is_old0) == n and len(siblings) == 32 * n * (nLevels + 1) and (not per or len(rb) == len(kb)), \
        'keys, old keys, old values, is_old0, siblings and roots differ in length'
    o0 = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in is_old0])
    st = (ctypes.c_int32 * max(n, 1))()
    ctx._check(ctx._lib.zkc_smt_check_absence(ctx._h, int(nLevels), n, kb, okb, ovb, o0, siblings if isinstance(siblings, bytes) else bytes(siblings), rb, int(per), st))
    return list(st)[:n]


def check_stats(ctx):
    """(host ms, host-to-device ms, kernel ms) of the context's last check_proofs or check_absence"""
    ms = (ctypes.c_double * 3)()
    ctx._check(ctx._lib.zkc_smt_check_stats(ctx._h, ms))
    return ms[0], ms[1], ms[2]


class CensusTree:
    """A census tree that grows and shrinks in place (zkc_tree_*, csrc/zkc_tree.hip): arbo Add / Update / Delete / Get / GenProof on a resident tree, the trie on the host, the hashes on the
    GPU, each call rehashing only the nodes it changed.  Keys and values: lists of ints, or bytes of n x 32-byte little-endian words.  Statuses: ZKC_TREE_* (STATUS below).
    Closed with its context at the latest (a context outlives its trees).  snapshot() gives a read-only view of the tree as it is now, which later changes leave alone."""

    OK, KEY_EXISTS, KEY_ABSENT, COLLISION, NOT_BELOW_R, NOT_IN_CENSUS, NOT_IN_SIK, SIK_MISMATCH = range(8)

    def __init__(self, ctx, nLevels=160, _handle=None):
        self.ctx, self.nLevels, self._lib = ctx, nLevels, ctx._lib
        self._snapshot = _handle is not None
        h = _handle
        if h is None:
            h = ctypes.c_void_p()
            ctx._check(self._lib.zkc_tree_create(ctx._h, int(nLevels), ctypes.byref(h)))
        self._h = h
        ctx._keys.append(self)            # the context closes what lives on it before itself

    def close(self):
        if getattr(self, '_h', None):
            if getattr(self.ctx, '_h', None):
                self._lib.zkc_tree_free(self._h)
            self._h = None
            if self in self.ctx._keys:
                self.ctx._keys.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _change(self, fn, keys, values):
        kb, vb = _le(keys), _le(values)
        n = len(kb) // 32
        assert len(vb) == len(kb), 'keys and values differ in length'
        st = (ctypes.c_int32 * n)()
        self.ctx._check(fn(self._h, kb, vb, n, st))
        return list(st)

    def add(self, keys, values):
        """arbo Add / AddBatch: per-entry statuses; the rejected entries change nothing."""
        return self._change(self._lib.zkc_tree_add, keys, values)

    def update(self, keys, values):
        return self._change(self._lib.zkc_tree_update, keys, values)

    def delete(self, keys):
        """arbo Delete: per-entry statuses (OK, KEY_ABSENT, NOT_BELOW_R); the rejected entries change nothing"""
        kb = _le(keys); n = len(kb) // 32
        st = (ctypes.c_int32 * n)()
        self.ctx._check(self._lib.zkc_tree_delete(self._h, kb, n, st))
        return list(st)

    def snapshot(self):
        """arbo Tree.Snapshot: a read-only CensusTree of this tree's current version (zkc_tree_snapshot).  It shares every node with this tree, answers root / len / get /
        gen_proof / gen_absence_proof / census_inputs_from_trees for that version while this tree goes on changing, and refuses changes.  Close it (or use it as a context
        manager) to release what only it still holds; it stays usable after this tree is closed."""
        h = ctypes.c_void_p()
        self.ctx._check(self._lib.zkc_tree_snapshot(self._h, ctypes.byref(h)))
        return CensusTree(self.ctx, self.nLevels, _handle=h)

    @property
    def is_snapshot(self):
        return self._snapshot

    def snapshot_count(self):
        """the number of live snapshots of this tree (the live tree and its snapshots count the same ones)"""
        n = ctypes.c_size_t()
        self.ctx._check(self._lib.zkc_tree_snapshot_count(self._h, ctypes.byref(n)))
        return n.value

    def refs(self):
        """(live node references, allocated references): the second stays bounded while the census churns at constant size"""
        out = (ctypes.c_size_t * 2)()
        self.ctx._check(self._lib.zkc_tree_refs(self._h, out))
        return out[0], out[1]

    @property
    def root(self):
        r = ctypes.create_string_buffer(32)
        self.ctx._check(self._lib.zkc_tree_root(self._h, r))
        return int.from_bytes(r.raw, 'little')

    def __len__(self):
        n = ctypes.c_size_t()
        self.ctx._check(self._lib.zkc_tree_size(self._h, ctypes.byref(n)))
        return n.value

    def stats(self):
        """(host trie ms, device ms) of the last add, update or delete"""
        ms = (ctypes.c_double * 2)()
        self.ctx._check(self._lib.zkc_tree_stats(self._h, ms))
        return ms[0], ms[1]

    def get(self, keys):
        """(values, exists): the stored value of every key (0 where absent)"""
        kb = _le(keys); n = len(kb) // 32
        out = ctypes.create_string_buffer(32 * n + 1); ex = (ctypes.c_int32 * n)()
        self.ctx._check(self._lib.zkc_tree_get(self._h, kb, n, ctypes.cast(out, ctypes.c_void_p), ex))
        raw = out.raw
        return [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(n)], [bool(x) for x in ex]

    def check_proofs(self, keys, values, siblings, root=None):
        """check_proofs at this tree's nLevels against `root` (None: the tree's current root; one int; or a list of n ints); the tree is not touched"""
        return check_proofs(self.ctx, keys, values, siblings, self.root if root is None else root, self.nLevels)

    def gen_proof(self, keys):
        """(root, siblings, depths, exists): siblings as bytes, n x (nLevels + 1) x 32, zero-padded like zkc_smt_build; the root they belong to"""
        kb = _le(keys); n = len(kb) // 32
        r = ctypes.create_string_buffer(32); sib = ctypes.create_string_buffer(32 * n * (self.nLevels + 1) + 1)
        dep = (ctypes.c_int32 * n)(); ex = (ctypes.c_int32 * n)()
        self.ctx._check(self._lib.zkc_tree_gen_proof(self._h, kb, n, r, ctypes.cast(sib, ctypes.c_void_p), dep, ex))
        return int.from_bytes(r.raw, 'little'), sib.raw[:32 * n * (self.nLevels + 1)], list(dep), [bool(x) for x in ex]

    def gen_absence_proof(self, keys):
        """arbo GenProof for absent keys: (root, siblings, depths, old_keys, old_values, is_old0, statuses).  siblings as gen_proof lays them out; old_keys / old_values:
        lists of ints (the leaf the key's path ran into, 0 when it ended at an empty child: is_old0 = 1).  A present key gets KEY_EXISTS and zeroed outputs."""
        kb = _le(keys); n = len(kb) // 32
        r = ctypes.create_string_buffer(32); sib = ctypes.create_string_buffer(32 * n * (self.nLevels + 1) + 1)
        ok = ctypes.create_string_buffer(32 * n + 1); ov = ctypes.create_string_buffer(32 * n + 1)
        dep = (ctypes.c_int32 * n)(); o0 = (ctypes.c_int32 * n)(); st = (ctypes.c_int32 * n)()
        self.ctx._check(self._lib.zkc_tree_gen_absence_proof(self._h, kb, n, r, ctypes.cast(sib, ctypes.c_void_p), dep, ctypes.cast(ok, ctypes.c_void_p),
                                                             ctypes.cast(ov, ctypes.c_void_p), o0, st))
        words = lambda raw: [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(n)]
        return (int.from_bytes(r.raw, 'little'), sib.raw[:32 * n * (self.nLevels + 1)], list(dep), words(ok.raw), words(ov.raw), list(o0), list(st))

    def check_absence(self, keys, old_keys, old_values, is_old0, siblings, root=None):
        """check_absence at this tree's nLevels against `root` (None: the tree's current root; one int; or a list of n ints); the tree is not touched"""
        return check_absence(self.ctx, keys, old_keys, old_values, is_old0, siblings, self.root if root is None else root, self.nLevels)


def census_inputs_from_trees(ctx, census_tree, sik_tree, election_id, address, password, signature, vote_weight, vote_hash, d_out_ptr=None):
    """census_inputs for n voters of two resident trees (zkc_tree_census_inputs): census_tree maps address -> available weight, sik_tree address -> SIK; either may be a
    snapshot (CensusTree.snapshot), whose frozen root and siblings the blocks then carry.  Returns
    (flat bytes, census root, sik root, statuses); a voter whose status is not CensusTree.OK gets a zeroed block.  vote_hash: pairs."""
    address = _le(address); n = len(address) // 32
    nIn = 12 + 2 * (census_tree.nLevels + 1)
    out = ctypes.create_string_buffer(32 * nIn * n); roots = ctypes.create_string_buffer(64); st = (ctypes.c_int32 * n)()
    ctx._check(ctx._lib.zkc_tree_census_inputs(census_tree._h, sik_tree._h, n, _le(election_id), _le(address), _le(password), _le(signature), _le(vote_weight),
                                               _le(x for pair in vote_hash for x in pair), ctypes.cast(out, ctypes.c_void_p), d_out_ptr, roots, st))
    return out.raw, int.from_bytes(roots.raw[:32], 'little'), int.from_bytes(roots.raw[32:], 'little'), list(st)
