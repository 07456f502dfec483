"""GPU: the jagged-diagonal sparse rows (csrc/zkc_jds.h) through both of their kernels at a domain of 16 -- zkc_matvec_jds (the prover's buildABC, rows = (matrix, constraint))
and zkc_r1cs_check_rows (the witness check, rows = A | B | C merged).  The random circuits of test_generic_circuit.py never have more than 4 terms in a row, so the
wave-per-row branch of either kernel is otherwise reached only through the census circuit.  One satisfiable system of 8 constraints over 199 wires: A rows around the prover's
long-row threshold (16) and far above it, merged rows around the check's (48), coefficients 1 and r - 1 (the marked units) beside random ones."""
import random
import pytest
import oracle_lib as ol
import closed_form as cf
from test_generic_circuit import setup_key
from zkcensus_amd import r1cs
from zkcensus_amd.r1cs import R, lc_eval

pytestmark = pytest.mark.gpu
N_IN = 190                                           # input wires 1 .. N_IN; wire N_IN appears in the 130-term row alone
SEED = 20261
# (terms of A, of B, of C) per constraint; merged lengths 5, 47, 48, 49, 86, 133, 20, 7
SHAPE = [(1, 3, 1), (15, 31, 1), (16, 31, 1), (17, 31, 1), (64, 20, 2), (130, 2, 1), (2, 17, 1), (3, 1, 3)]
LONGEST = 5


def build_system():
    rng = random.Random(SEED)
    nW = 1 + N_IN + len(SHAPE)
    wit = [1] + [rng.randrange(1, R) for _ in range(N_IN)] + [0] * len(SHAPE)
    cs = r1cs.R1CS(nW, 2)

    def lc(n, must=None):
        ws = rng.sample(range(0, N_IN), n - (must is not None)) + ([must] if must is not None else [])
        out = {}
        for i, w in enumerate(ws):
            out[w] = (1, R - 1, rng.randrange(2, R - 1))[i % 3 if n > 2 else 2 * (i % 2)]
        return out
    for k, (na, nb, nc) in enumerate(SHAPE):
        out = N_IN + 1 + k
        a, b = lc(na, N_IN if k == LONGEST else None), lc(nb)
        rest = lc(nc - 1) if nc > 1 else {}
        coef = (1, R - 1, rng.randrange(2, R - 1))[k % 3]
        wit[out] = (lc_eval(a, wit) * lc_eval(b, wit) - lc_eval(rest, wit)) * pow(coef, -1, R) % R
        c = dict(rest); c[out] = coef
        assert (len(a), len(b), len(c)) == (na, nb, nc)
        cs.add(a, b, c)
    assert cs.check(wit) == -1
    assert [len(a) for a, _, _ in cs.cons][:6] == [1, 15, 16, 17, 64, 130]
    assert {47, 48, 49} <= {len(a) + len(b) + len(c) for a, b, c in cs.cons}
    coefs = {v for con in cs.cons for side in con for v in side.values()}
    assert 1 in coefs and R - 1 in coefs and len(coefs) > 50
    return cs, wit


@pytest.fixture(scope='module')
def system(tmp_path_factory):
    cs, wit = build_system()
    path = str(tmp_path_factory.mktemp('sparse_rows') / 'rows.r1cs')
    cs.write(path)
    return cs, wit, path


def test_prover_and_witness_check_on_long_rows(system):
    import zkcensus_amd
    cs, wit, path = system
    w = b''.join(x.to_bytes(32, 'little') for x in wit)
    zk, _ = setup_key(path, SEED)
    ctx = zkcensus_amd.Context(0)
    try:
        pk = zkcensus_amd.ProvingKey(ctx, zk)
        assert pk.n_vars == cs.nWires and pk.n_public == 2
        for r, s in ((1, 2), (R - 3, 12345678901234567890)):
            proof, pub = pk.prove(w, r, s)
            a, b, c = cf.proof_scalars(path, SEED, w, r, s)
            assert proof == cf.proof_from_scalars(ol, a, b, c), 'GPU proof over long sparse rows differs from the closed form'
            assert pub == w[32:96]
        pk.close()
        with r1cs.Device(ctx, path) as dev:
            assert dev.info == (cs.nWires, 2, len(SHAPE))
            assert dev.check(w) == ([r1cs.SATISFIED], [0])
            bad = list(wit); bad[N_IN] = (bad[N_IN] + 1) % R          # a wire of the 130-term row and of no other
            assert cs.check(bad) == LONGEST
            assert dev.check(b''.join(x.to_bytes(32, 'little') for x in bad)) == ([LONGEST], [1])
    finally:
        ctx.close()
