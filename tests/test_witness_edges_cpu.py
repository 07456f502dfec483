"""CPU: the two independent restatements of the circuit -- the oracle (oracle/witness.c) and the R1CS generator (zkcensus_amd/r1cs.py) -- at the value edges of
tests/edge_voters.py.  For every case the oracle's status is the pinned one, and the oracle's witness satisfies every constraint exactly when that status is 0: what the GPU
suite (tests/test_gpu_witness_edges.py) compares the kernels with is therefore the circuit's own behaviour, including the accepted wrap (availableWeight 3, voteWeight r - 1)."""
import pytest
import oracle_lib as ol
import edge_voters as ev
from zkcensus_amd import r1cs

R, P252 = ol.R, 1 << 252


@pytest.fixture(scope='module')
def circuit():
    built = {}

    def get(nl):                       # one build per size and module (8 s at nLevels = 253)
        if nl not in built:
            built[nl] = r1cs.build(nl)[1]
        return built[nl]
    return get


def check_cases(cs, nl, cases):
    assert cases
    for name, voter, status in cases:
        rc, w = ol.witness(voter, nLevels=nl)
        assert rc == status, (nl, name)
        assert (cs.check(ev.wires(w)) == -1) == (status == 0), (nl, name)


def test_case_lists_are_whole():
    assert len(ev.ADDRESSES) == 12 and len({a for _, a in ev.ADDRESSES}) == 12 and all(0 <= a < R for _, a in ev.ADDRESSES)
    assert len(ev.WEIGHTS) == 16 and len({w[:2] for w in ev.WEIGHTS}) == 16
    assert len(ev.WEIGHTS_FROM_2P252) == 6
    cases = ev.all_cases(10)
    assert len(cases) == 40 and len({c[0] for c in cases}) == 40
    assert ev.all_cases(10)[5][1] == ev.all_cases(10)[5][1] and ev.address_cases(10, 3)[0][1]['address'] == '0'
    v = dict(ev.field_cases(10)[8][1])                                                   # exactly one non-zero sibling per tree, at the top of the path
    assert [int(x) != 0 for x in v['censusSiblings']] == [i == 6 for i in range(11)] and [int(x) != 0 for x in v['sikSiblings']] == [i == 5 for i in range(11)]
    assert {int(x) for x in ev.field_cases(10)[6][1]['censusSiblings']} == {0, R - 1}


def test_status_table_is_the_circuits():
    """The pinned statuses derived again from LessEqThan(252) as circomlib states it: n2b of in[0] + 2^252 - in[1] with in = (voteWeight, availableWeight + 1), 253 bits,
    out = 1 - bit 252 -- over the field, so the sum wraps for operands at and above 2^252."""
    for avail, vote, status in ev.WEIGHTS:
        x = (vote + P252 - (avail + 1)) % R
        assert x < (1 << 254)
        assert (1 if x >> 252 else 0) == status, (avail, vote)
        assert (status == 0) == (vote <= avail) or max(avail, vote) >= P252              # below 2^252 the circuit is the comparison it is named after
    assert (ev.WRAP[1] + P252 - ev.WRAP[0] - 1) % R == P252 - 5                          # the wrap: bit 252 clear, accepted
    assert ev.WRAP + (0,) in ev.WEIGHTS


def test_every_case_nl10(circuit):
    check_cases(circuit(10), 10, ev.all_cases(10))


def test_subset_nl160(circuit):
    cases = ev.by_name(ev.address_cases(160, 3), 'addr_0@d3', 'addr_2^253@d3') + ev.by_name(ev.weight_cases(160), ev.weight_name(*ev.WRAP))
    check_cases(circuit(160), 160, cases)


@pytest.mark.parametrize('depth', [3, 253])
def test_addresses_nl253(circuit, depth):
    """nLevels = 253: every key bit steers a level and bit 253 is the one Num2Bits solves for; the n2bNew bits above the depth and the alias check see keys of 254 bits."""
    check_cases(circuit(253), 253, ev.address_cases(253, depth))


def test_weights_from_2p252_nl253(circuit):
    check_cases(circuit(253), 253, ev.weight_cases(253, 3, ev.WEIGHTS_FROM_2P252))
