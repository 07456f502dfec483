"""Voters at the value edges of the witness kernels (csrc/zkc_witness.hip branches on the values themselves: key = 0, the `v > c` arm of the alias check, key bits
above nLevels, bits 252 / 253 of the LessEqThan(252) sum, the shared inversion over the siblings).  A plain module like census_lib.py -- no fixtures -- so that the CPU
tests (oracle and R1CS) and the GPU tests (both witness kernels, the prover, the batch verifier's inputs) run the same inputs.  Valid by construction the way
tools/census_gen.py: random_voter is: both roots are climbed from the sibling paths over the oracle's Poseidon."""
import functools, os, random, sys
import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, 'tools'))
from census_gen import climb, EID      # noqa: E402

R = ol.R
P252 = 1 << 252
ZKC_W_ERR_WEIGHT = 1                   # include/zkcensus.h

# ---- the case lists (data) ----
ADDRESSES = [                          # each with weights (1, 1)
    ('addr_0', 0), ('addr_1', 1), ('addr_r-1', R - 1), ('addr_r-2', R - 2),
    ('addr_2^253', 1 << 253), ('addr_2^253-1', (1 << 253) - 1), ('addr_2^252', 1 << 252), ('addr_2^160-1', (1 << 160) - 1),
    ('addr_r-1-2^200', R - 1 - (1 << 200)),
    ('addr_1010', int('10' * 127, 2)),                      # 0x2aaa...a, 254 bits, below r
    ('addr_0101', int('01' * 127, 2) % R),                  # 0x1555...5
    ('addr_ones128<<100', ((1 << 128) - 1) << 100),
]
# (availableWeight, voteWeight, status): 0 = accepted, 1 = ZKC_W_ERR_WEIGHT.  LessEqThan(252) decomposes voteWeight + 2^252 - availableWeight - 1 IN THE FIELD and asks for
# bit 252 clear, which is only "vote <= available" while both are below 2^252: (3, r - 1) wraps to 2^252 - 5 and is accepted by the reference circuit.
WEIGHTS = [
    (1, 0, 0), (1, 1, 0), (0, 0, 0), (P252 - 1, P252 - 1, 0), (P252 - 1, 0, 0), (1 << 251, 1 << 251, 0),
    (5, 6, 1), (0, 1, 1), (P252 - 2, P252 - 1, 1),
    (P252, 1, 0), (R - 1, 3, 1), (3, R - 1, 0), (R - 1, R - 1, 0), (P252, P252, 0), (0, P252, 1), (0, P252 - 1, 1),
]
WRAP = (3, R - 1)
WEIGHTS_FROM_2P252 = tuple(w for w in WEIGHTS if max(w[0], w[1]) >= P252)      # every pair with a value at or above 2^252


def weight_name(a, v):
    def s(x):
        for base, name in ((R, 'r'), (P252, '2^252'), (1 << 251, '2^251')):
            if abs(x - base) <= 5 and x:
                return name + ('%+d' % (x - base) if x != base else '')
        return str(x)
    return 'w_%s_%s' % (s(a), s(v))


def edge_voter(rng, nLevels, address, avail, vote, depth_c, depth_s, password=None, signature=None, election_id=None, sibling=None):
    """One voter whose roots are climbed from its own sibling paths (tools/census_gen.py: climb), with every value under the caller's control.
    depth_c / depth_s: 1 + the index of the last non-zero sibling (cut at nLevels).  sibling: None -- non-zero siblings drawn from [1, r), a fifth of those below the top
    left zero; an integer -- every sibling below the depth is that value; 'top' -- exactly one non-zero sibling, at depth - 1, zeros below."""
    H = ol.poseidon
    password = rng.getrandbits(88) if password is None else password
    signature = rng.getrandbits(512) % R if signature is None else signature
    eid = EID if election_id is None else tuple(election_id)

    def sibs(d):
        d = min(d, nLevels); s = [0] * (nLevels + 1)
        for i in range(d):
            draw = 0 if (rng.random() < 0.2 and i != d - 1) else rng.randrange(1, R)          # drawn in every mode: the other fields do not move with `sibling`
            s[i] = draw if sibling is None else (draw if i == d - 1 else 0) if sibling == 'top' else int(sibling)
        return s
    cs, ss = sibs(depth_c), sibs(depth_s)
    sik = H([address, password, signature])
    return {
        'electionId': [str(eid[0]), str(eid[1])], 'nullifier': str(H([signature, password, eid[0], eid[1]])),
        'availableWeight': str(avail), 'voteHash': [str(rng.getrandbits(128)), str(rng.getrandbits(128))],
        'sikRoot': str(climb(H, address, sik, ss)), 'censusRoot': str(climb(H, address, avail, cs)),
        'address': str(address), 'password': str(password), 'signature': str(signature), 'voteWeight': str(vote),
        'censusSiblings': [str(x) for x in cs], 'sikSiblings': [str(x) for x in ss],
    }


def _mk(name, nLevels, status=0, **kw):
    """Deterministic per (name, nLevels): every test that asks for a case gets the same voter."""
    rng = random.Random('%s/%d' % (name, nLevels))
    address, avail = rng.getrandbits(160), rng.randrange(1, 101)                          # the ordinary values of census_gen.random_voter
    vote = rng.randrange(0, avail + 1)
    kw.setdefault('address', address)
    if 'avail' not in kw:
        kw['avail'], kw['vote'] = avail, vote
    return name, edge_voter(rng, nLevels, **kw), status


@functools.lru_cache(maxsize=None)
def address_cases(nLevels, depth):
    return tuple(_mk('%s@d%d' % (n, depth), nLevels, address=a, avail=1, vote=1, depth_c=depth, depth_s=depth) for n, a in ADDRESSES)


@functools.lru_cache(maxsize=None)
def weight_cases(nLevels, depth=3, which=None):
    return tuple(_mk(weight_name(a, v), nLevels, status=st, avail=a, vote=v, depth_c=depth, depth_s=depth) for a, v, st in (which or tuple(WEIGHTS)))


@functools.lru_cache(maxsize=None)
def field_cases(nLevels, depth=3):
    nl, d = nLevels, depth
    return (
        _mk('password_0', nl, password=0, depth_c=d, depth_s=d), _mk('password_r-1', nl, password=R - 1, depth_c=d, depth_s=d),
        _mk('signature_0', nl, signature=0, depth_c=d, depth_s=d), _mk('signature_r-1', nl, signature=R - 1, depth_c=d, depth_s=d),
        _mk('eid_0_0', nl, election_id=(0, 0), depth_c=d, depth_s=d), _mk('eid_r-1_r-1', nl, election_id=(R - 1, R - 1), depth_c=d, depth_s=d),
        _mk('siblings_r-1', nl, sibling=R - 1, depth_c=d, depth_s=d + 1), _mk('siblings_1', nl, sibling=1, depth_c=d + 1, depth_s=d),
        _mk('sibling_top_only', nl, sibling='top', depth_c=min(nl, 2 * d + 1), depth_s=min(nl, 2 * d)),
        _mk('addr_0_depths_0_nl', nl, address=0, depth_c=0, depth_s=nl), _mk('addr_0_depths_nl_0', nl, address=0, depth_c=nl, depth_s=0),
        _mk('addr_2^253_depth_nl', nl, address=1 << 253, depth_c=nl, depth_s=nl),
    )


def all_cases(nLevels, depth=3):
    """(name, voter, status) for the whole list: addresses, weight pairs, other fields."""
    return list(address_cases(nLevels, depth)) + list(weight_cases(nLevels, depth)) + list(field_cases(nLevels, depth))


def by_name(cases, *names):
    d = {c[0]: c for c in cases}
    return [d[n] for n in names]


def wires(w):
    return [int.from_bytes(w[32 * i:32 * i + 32], 'little') for i in range(len(w) // 32)]
