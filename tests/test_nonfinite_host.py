"""The non-finite rule of tests/nonfinite_util.py can fail: for every case tests/test_gpu_nonfinite.py runs, the float64 reference itself
(rounded to float32, as a kernel would return it) passes `check`, and the same operation emulated with the device's former arithmetic -
the ReLU `v > 0 ? v : 0`, the 2x2 pooling nested from fmax - is rejected for dropping the NaN.  The premises are checked here as well, on
the CPU, for every shape: the NaN reaches a proper, non-empty subset of the outputs, and the maps a scale is taken from keep every
pixel's largest magnitude inside one power-of-two bucket."""
import pytest
import torch

from tests import exact_util as E
from tests import nonfinite_util as N

GEOMS = E.conv_geometries()
OTHERS = N.other_cases()


def as_kernel(outs):
    return {p: tuple(t.float() for t in ts) for p, ts in outs.items()}


def holds_the_rule(case):
    refs = N.references(case)
    N.check_case(as_kernel(refs), refs, case.name)
    emulations = ([dict(relu=N.drop_relu)] if case.relu else []) + ([dict(pool=N.drop_pool)] if case.pool else [])
    for kw in emulations:
        with torch.no_grad():
            got = as_kernel(case.outputs(**{**N.GOOD, **kw}))
        with pytest.raises(N.RuleViolation, match="finite where the reference is NaN"):
            N.check("nan", got["nan"][0], got["clean"][0], refs["nan"][0], refs["clean"][0], what=f"{case.name}, {list(kw)[0]} dropping NaN")
    if hasattr(case, "forward_maps"):
        N.handoff_premise(case)


@pytest.mark.parametrize("g", GEOMS, ids=[g.name for g in GEOMS])
def test_conv_layer_cases(g):
    for ep in E.EPILOGUES:
        holds_the_rule(N.ConvCase(g, ep))


@pytest.mark.parametrize("name", list(OTHERS))
def test_other_cases(name):
    holds_the_rule(OTHERS[name]())


def test_the_rule_on_a_toy():
    """Each clause on four hand-made tensors: a dropped NaN, a moved bit outside the reach, an Inf where the reference is finite, and
    the premises (an empty reach, a reach that is everything)."""
    clean = torch.tensor([1.0, 2.0, 3.0, 4.0])
    ref_nan = torch.tensor([1.0, N.NAN, 3.0, 4.0]).double()
    good = torch.tensor([1.0, N.NAN, 3.0, 4.0])
    reach = N.check("nan", good, clean, ref_nan, clean.double())
    assert reach.tolist() == [False, True, False, False]
    with pytest.raises(N.RuleViolation, match="finite where"):
        N.check("nan", torch.tensor([1.0, 0.0, 3.0, 4.0]), clean, ref_nan, clean.double())
    with pytest.raises(N.RuleViolation, match="outside the reach"):
        N.check("nan", torch.tensor([1.0, N.NAN, 3.0000002, 4.0]), clean, ref_nan, clean.double())
    with pytest.raises(N.RuleViolation, match="outside the reach"):
        N.check("nan", torch.tensor([1.0, N.NAN, N.NAN, 4.0]), clean, ref_nan, clean.double())
    with pytest.raises(N.BrokenPremise):
        N.check("nan", clean, clean, clean.double(), clean.double())
    with pytest.raises(N.BrokenPremise):
        N.check("nan", clean, clean, torch.full((4,), N.NAN).double(), clean.double())
    # Inf: element 1 is reached and non-finite, element 2 is reached and finite again (a ReLU's 0 that equals the clean value)
    ref_inf = torch.tensor([1.0, N.INF, 3.0, 4.0]).double()
    reach = torch.tensor([False, True, True, False]).numpy()
    N.check("inf", torch.tensor([1.0, N.NAN, N.NAN, 4.0]), clean, ref_inf, clean.double(), reach=reach)
    N.check("inf", torch.tensor([1.0, N.INF, 3.0, 4.0]), clean, ref_inf, clean.double(), reach=reach)
    with pytest.raises(N.RuleViolation, match="finite where"):
        N.check("inf", torch.tensor([1.0, 9.0, 3.0, 4.0]), clean, ref_inf, clean.double(), reach=reach)
    with pytest.raises(N.RuleViolation, match="Inf where the reference is finite"):
        N.check("inf", torch.tensor([1.0, N.INF, -N.INF, 4.0]), clean, ref_inf, clean.double(), reach=reach)
    with pytest.raises(N.RuleViolation, match="outside the reach"):
        N.check("inf", torch.tensor([1.0, N.INF, 3.0, N.NAN]), clean, ref_inf, clean.double(), reach=reach)
    with pytest.raises(N.RuleViolation, match="outside the reach"):       # without a reach: where the references are equal
        N.check("inf", torch.tensor([1.0, N.INF, N.NAN, 4.0]), clean, ref_inf, clean.double())
