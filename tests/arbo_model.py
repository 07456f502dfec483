"""A GPU-free model of the census trees: what the root, the sibling lists and the absence proofs of a key set MUST be, computed in plain Python over the oracle's
Poseidon.  A plain module beside census_lib.py: no fixtures, no import of the product package.

arbo's conventions, as zkcensus_amd/census.py states them: leaf = H(key, value, 1); node = H(left, right); path bit i = bit i of the key, LSB first; an empty subtree
is 0; a subtree holding one leaf is that leaf's hash (a leaf sits at the first depth where its path is unique); two keys that agree on their first nLevels bits collide.

The tree is made by partitioning the key set on the path bit, depth by depth, with an explicit work list (a chain below two keys parting at bit 252 is 253 nodes long:
no recursion).  Every hash goes through one memo keyed by its inputs, so a subtree that two trees share -- before and after a delete, say -- is hashed once."""
import oracle_lib as ol

R = ol.R
_memo = {}
_trees = {}


def H(*xs):
    h = _memo.get(xs)
    if h is None:
        if len(_memo) > 400000:
            _memo.clear()
        h = _memo[xs] = ol.poseidon(list(xs))
    return h


class _Tree:
    """refs: 0 = empty, -(1 + i) = leaf keys[i], 1 + j = inner node j (nodes[j] = [depth, left ref, right ref]); children are made after their parent"""

    def __init__(self, kv, nl):
        if not (isinstance(nl, int) and 1 <= nl <= 253):
            raise ValueError('nLevels %r is not in 1..253' % (nl,))
        self.nl, self.keys, self.vals = nl, list(kv), list(kv.values())
        for x in self.keys + self.vals:
            if not 0 <= x < R:
                raise ValueError('a key or value is not below r')
        keys, nodes, work = self.keys, [], []

        def ref(members, depth, parent, side):
            if len(members) == 1:
                r = -(1 + members[0])
            elif not members:
                r = 0
            else:
                if depth >= nl:
                    raise ValueError('keys %s collide on their first %d bits' % (', '.join(hex(keys[m]) for m in members[:2]), nl))
                nodes.append([depth, 0, 0])
                r = len(nodes)
                work.append((r, members, depth))
            if parent:
                nodes[parent - 1][1 + side] = r
            return r
        self.root_ref = ref(list(range(len(keys))), 0, 0, 0)
        while work:
            r, members, depth = work.pop()
            ref([m for m in members if not (keys[m] >> depth) & 1], depth + 1, r, 0)
            ref([m for m in members if (keys[m] >> depth) & 1], depth + 1, r, 1)
        self.nodes = nodes
        self.hash = [0] * len(nodes)
        for j in range(len(nodes) - 1, -1, -1):                       # children have larger indices: they are hashed first
            self.hash[j] = H(self.value(nodes[j][1]), self.value(nodes[j][2]))
        self.root = self.value(self.root_ref)

    def value(self, r):
        return 0 if r == 0 else self.hash[r - 1] if r > 0 else H(self.keys[-r - 1], self.vals[-r - 1], 1)

    def walk(self, key):
        """(where the key's path ends: 0 or a leaf ref; the siblings passed, root first)"""
        r, sibs = self.root_ref, []
        while r > 0:
            d, left, right = self.nodes[r - 1]
            bit = (key >> d) & 1
            sibs.append(self.value(left if bit else right))
            r = right if bit else left
        return r, sibs


def _tree(kv, nl):
    k = (nl, tuple(kv.items()))
    t = _trees.get(k)
    if t is None:
        if len(_trees) > 64:
            _trees.clear()
        t = _trees[k] = _Tree(kv, nl)
    return t


def root(kv, nl):
    return _tree(kv, nl).root


def proof(kv, nl, key):
    """(the nl + 1 zero-padded siblings, depth, exists) -- an absent key gets no siblings and depth 0, as zkc_tree_gen_proof gives them"""
    t = _tree(kv, nl)
    r, sibs = t.walk(key)
    if r == 0 or t.keys[-r - 1] != key:
        return [0] * (nl + 1), 0, False
    return sibs + [0] * (nl + 1 - len(sibs)), len(sibs), True


def absence_proof(kv, nl, key):
    """(siblings, depth, old_key, old_value, is_old0) of an absent key, as zkc_tree_gen_absence_proof documents them: where the key's path ends -- an empty child
    (is_old0 = 1, old key and value 0) or the leaf of another key (is_old0 = 0, that leaf's key and value); an empty tree gives depth 0 and is_old0 = 1"""
    t = _tree(kv, nl)
    r, sibs = t.walk(key)
    if r and t.keys[-r - 1] == key:
        raise KeyError('the key is present')
    pad = sibs + [0] * (nl + 1 - len(sibs))
    return (pad, len(sibs), 0, 0, 1) if r == 0 else (pad, len(sibs), t.keys[-r - 1], t.vals[-r - 1], 0)


def inner_nodes_per_depth(kv, nl):
    """the number of inner nodes at each depth 0 .. nl - 1"""
    out = [0] * nl
    for d, _, _ in _tree(kv, nl).nodes:
        out[d] += 1
    return out
