"""LGN's whole propagation on the GPU (clsr_amd/lgn.py: Propagation -- two fused layers forward, the gate and two layers
over the transposed graph backward, the fixed-order reduction of d W_k | d b_k) against the float64 oracle
(tests/lgn_oracle.py) on the fixtures of tests/lgn_cases.py: the reference's own graph of the golden data, and a synthetic
graph in which one user row and one item row run through the split path in both directions.

Every value is held to the oracle's propagated fp32 bound (SLACK * gamma_n * the absolute-value graph, stated once in the
oracle); tests/test_lgn_cpu.py holds that no pre-activation of these fixtures is undecidable, so no comparison hangs on
a gate."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lgn_cases as K  # noqa: E402
from clsr_amd.lgn import Propagation  # noqa: E402

DEV = "cuda:0"


def _within(got, exp, bound, name):
    got = got.detach().double().cpu().reshape(-1)
    err = (got - exp.reshape(-1)).abs()
    bound = bound.reshape(-1)
    assert not torch.isnan(got).any(), name
    print("%s: max err %.3e, bound there %.3e, max |exp| %.3e" % (name, float(err.max()), float(bound[err.argmax()]),
                                                                   float(exp.abs().max())))
    assert bool((err <= bound).all()), "%s: error exceeds the propagated fp32 bound by %.3e" % (name, float((err - bound).max()))


def _run(name, training=True):
    c = K.case(name)
    prop = Propagation(c["graph"], c["C"], device=DEV)
    dev = lambda t: t.to(DEV)
    F = prop.forward(dev(c["E0"]), [dev(W) for W in c["Ws"]], [dev(b) for b in c["bs"]], training=training)
    if not training:
        torch.cuda.synchronize()
        return c, prop, F.clone()
    dE0, dW, db = prop.backward(dev(c["dF"]))
    torch.cuda.synchronize()
    return c, prop, [F.clone(), dE0.clone()] + [t.clone() for t in dW + db]


@pytest.mark.parametrize("name", ["golden", "skewed"])
def test_propagation_matches_oracle(name):
    c, prop, (F, dE0, dW0, dW1, db0, db1) = _run(name)
    fwd = c["fwd"]
    _within(F, fwd["F"], fwd["e_F"], "F")
    for k in range(2):
        _within(prop._bufs["S%d" % k], fwd["S"][k], fwd["e_S"][k], "S_%d" % k)
        _within(prop._bufs["E%d" % (k + 1)], fwd["E"][k + 1], fwd["e_Z"][k], "E_%d" % (k + 1))
    x_dE0, x_dW, x_db, e_dE0, e_dW, e_db = c["bwd"]
    _within(dE0, x_dE0, e_dE0, "dE_0")
    for k, (gW, gb) in enumerate(((dW0, db0), (dW1, db1))):
        _within(gW, x_dW[k], e_dW[k], "dW_%d" % k)
        _within(gb, x_db[k], e_db[k], "db_%d" % k)
    if name == "skewed":
        assert prop.fwd.nlong == 2 and prop.bwd.nlong == 2 and prop.fwd.nchunks >= 6


def test_scoring_pass_gives_the_same_F_and_keeps_no_state():
    c, prop, F = _run("golden", training=False)
    _, _, ref = _run("golden")
    assert torch.equal(F, ref[0])
    assert "S0" not in prop._bufs
    with pytest.raises(ValueError, match="training=True"):
        prop.backward(c["dF"].to(DEV))


def test_two_passes_are_bit_identical():
    a, b = _run("skewed")[2], _run("skewed")[2]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_limits_are_refused_by_name():
    c = K.case("golden")
    with pytest.raises(NotImplementedError, match="item_embedding_dim \\+ cate_embedding_dim must be a positive multiple of 4"):
        Propagation(c["graph"], 42, device=DEV)
    with pytest.raises(NotImplementedError, match="at most 128"):
        Propagation(c["graph"], 132, device=DEV)
    prop = Propagation(c["graph"], c["C"], device=DEV)
    with pytest.raises(ValueError, match="2 layers"):
        prop.forward(c["E0"].to(DEV), [c["Ws"][0].to(DEV)], [c["bs"][0].to(DEV)])
    with pytest.raises(ValueError, match="contiguous fp32"):
        prop.forward(c["E0"].double().to(DEV), [W.to(DEV) for W in c["Ws"]], [b.to(DEV) for b in c["bs"]])
