"""The cases of tests/test_gpu_conv_exact.py, checked on the host: the data really is exactly representable (tests/exact_util.py's
three preconditions), the specification of csrc/split_arith.hpp - emulated in torch, float64 products - then returns the float64 result
bit for bit, and the data is SENSITIVE: dropping any kept product, shifting a tap, dropping the last k-block or zeroing a halo column
(arithmetic on CPU tensors, nothing is injected into a kernel) changes at least one output of the class meant to see it.  No GPU."""
import pytest
import torch

from tests import exact_util as E
from tests.exact_util import BF16X6, F16X3, F32, PRECISIONS

GEOMS = E.conv_geometries()
KEY_PRECISIONS = {"A": PRECISIONS, "D": (F32, BF16X6), "C24": (F32, BF16X6), "E": (F32, BF16X6), "B": (F16X3,), "C16": (F16X3,)}


def check_case(case, precisions, light=False):
    """Preconditions and emulator == float64 at every precision (f16x3: also under a bound 4x above the maximum).  Returns the reference.
    light: the product itself - the same operands - was checked in full on a sibling case with another epilogue: precondition 2 is not
    repeated and the emulator runs at f16x3 only."""
    ref, headroom = E.preconditions(case, () if light else precisions)
    assert bool(ref.any()), f"{case.name}: an all-zero result checks nothing"
    for p in ((F16X3,) if light else precisions):
        assert torch.equal(case.forward(E.Emulator(p)), ref), f"{case.name}: the {p} specification differs from float64"
        if p == F16X3 and not light:
            assert headroom is not None and headroom >= E.MIN_HEADROOM_BITS
            assert torch.equal(case.forward(E.Emulator(p, bound=4.0)), ref), f"{case.name}: {p} under a 4x bound differs from float64"
    return ref


def must_change(case, mul, ref, fault):
    assert not torch.equal(case.forward(mul), ref), f"{case.name}: {fault} changes no output"


def dropped_products_change(case, precisions, ref, side):
    """Each kept product that involves a piece of the operand carrying the pattern (side 0: a, side 1: b), dropped in turn."""
    for p in precisions:
        for i in range(E.NPIECES[p]):
            drop = (i, 0) if side == 0 else (0, i)
            must_change(case, E.Emulator(p, drop=drop), ref, f"{p} without a{drop[0]} b{drop[1]}")


def indexing_faults_change(case, ref, halo=True, last_k=True):
    must_change(case, E.FaultShiftedTap(), ref, "a tap shifted by one")
    if last_k:
        must_change(case, E.FaultLastKBlock(), ref, "the last k-block dropped")
    if halo:
        must_change(case, E.FaultHaloColumn(), ref, "a halo column zeroed")


@pytest.mark.parametrize("g", GEOMS, ids=[g.name for g in GEOMS])
def test_conv_layer_cases(g):
    for key, precisions in KEY_PRECISIONS.items():
        case = E.ConvLayerCase(g, key)
        ref = check_case(case, precisions)
        if key == "A":
            indexing_faults_change(case, ref)
        elif key == "E":
            for drop in ((0, 0), (0, 1), (1, 0), (1, 1)):
                must_change(case, E.Emulator(BF16X6, drop=drop), ref, f"bf16x6 without a{drop[0]} b{drop[1]}")
        else:
            dropped_products_change(case, precisions, ref, side=0 if key in ("B", "D") else 1)
    for ep in E.EPILOGUES[1:]:
        check_case(E.ConvLayerCase(g, "A", ep), PRECISIONS, light=True)


@pytest.mark.parametrize("g", E.conv_geometries(own_batch=True), ids=lambda g: g.name)
def test_conv_layer_cases_at_their_lists_batch(g):
    """The same geometries and generators at the batch their list runs them at: the sensitivity was shown at batch 2."""
    for key, precisions in KEY_PRECISIONS.items():
        check_case(E.ConvLayerCase(g, key), precisions)
    for ep in E.EPILOGUES[1:]:
        check_case(E.ConvLayerCase(g, "A", ep), PRECISIONS, light=True)


@pytest.mark.parametrize("name", ["3x3 s2 odd size", "4x4 convT s4 p1 op2", "1x3 dil 2 cin 13"])
def test_one_tap_short_cut_is_the_dense_convolution(name):
    g = next(g for g in GEOMS if g.name == name)
    for key in ("D", "C24", "E", "B", "C16"):
        case = E.ConvLayerCase(g, key)
        a, b = case.x.double(), case.w.double()
        assert torch.equal(case.op(a, b), case.op(a, b, dense=True))


def test_conv_geometries_cover_the_lists_of_test_gpu_conv():
    names = " | ".join(g.name for g in GEOMS)
    for part in ("3x3 s1 64->64", "3x3 s2 odd size", "4x4 convT s2 p1", "4x4 convT s4 p1 op2", "7x7 s2 p3 384->64", "split-K 16", "on 6x6 (split-K)",
                 "cin 13", "3x3 cin 3", "f16: ", "tap pairs: ", "direct: ", "small cin: "):
        assert part in names, part
    assert all(g.B == 2 for g in GEOMS)


@pytest.mark.parametrize("g", [g for g in GEOMS if (g.kh, g.stride) == (7, 2) and not g.transposed and g.cin >= 32 and g.H <= 50], ids=lambda g: g.name)
def test_stem_case_past_the_batch_limit(g):
    check_case(E.ConvLayerCase(g, "A", batch=5), PRECISIONS)


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("C,H,W,L", E.RUN_GEOMS + [(64, H, W, L) for H, W, L in E.TILE_GEOMS])
def test_run_cases(C, H, W, L, kind):
    case = E.RunCase(C, H, W, L, kind)
    ref = check_case(case, (F16X3,))
    indexing_faults_change(case, ref, last_k=False)
    for w, bn, scale, shift in case.layers:      # the folded epilogue is what the class promises
        assert set(scale.tolist()) <= {0.5, 1.0} and torch.equal(shift * 2, (shift * 2).round())


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("C,H,W,d", E.PAIR_GEOMS)
def test_pair_cases(C, H, W, d, kind):
    for with_res in (False, True):
        case = E.pair_case(C, H, W, d, with_res, kind)
        ref = check_case(case, (BF16X6, F16X3))
        indexing_faults_change(case, ref, last_k=False)
    case = E.block_case(C, H, W, d, kind)
    ref = check_case(case, (BF16X6, F16X3))
    indexing_faults_change(case, ref, last_k=False)


@pytest.mark.parametrize("kind", E.R_KINDS)
@pytest.mark.parametrize("C,H,W,dils", E.CHAIN_GEOMS)
def test_chain_cases(C, H, W, dils, kind):
    case = E.chain_case(C, H, W, dils, kind)
    ref = check_case(case, (BF16X6, F16X3))
    indexing_faults_change(case, ref, last_k=False)


@pytest.mark.parametrize("key", E.FP32_CLASSES)
def test_deconv_and_upconv_cases(key):
    for geom in E.DECONV_GEOMS:
        case = E.DeconvCase(*geom, key)
        ref = check_case(case, (F32,))
        if key == "A":
            indexing_faults_change(case, ref)
    for geom in E.UPCONV_GEOMS:
        case = E.UpconvCase(*geom, key)
        ref = check_case(case, (F32,))
        if key == "A":
            must_change(case, E.FaultLastKBlock(), ref, "the last k-block dropped")
            must_change(case, E.FaultHaloColumn(), ref, "a column zeroed")


@pytest.mark.parametrize("geom", E.WGRAD_GEOMS)
def test_wgrad_cases(geom):
    case = E.WgradCase(*geom[:6], "A", *geom[6:])
    ref = check_case(case, (BF16X6, F16X3))
    indexing_faults_change(case, ref)
    for key, p in (("D", BF16X6), ("B", F16X3)):
        case = E.WgradCase(*geom[:6], key, *geom[6:])
        ref = check_case(case, (p,))
        dropped_products_change(case, (p,), ref, side=0)


@pytest.mark.parametrize("g", E.TRAIN_CONV_GEOMS, ids=lambda g: g.name)
def test_train_conv_cases(g):
    """One step of hipnn.conv2d: every one of the three products (forward, data gradient, weight gradient) is exactly representable at
    both training precisions, and a shifted tap, a dropped k-block and a zeroed halo column each change dx."""
    case = E.TrainConvCase(g)
    y, dx, dw = case.legs()
    refs = [check_case(leg, (BF16X6, F16X3)) for leg in (y, dx, dw)]
    assert all(torch.equal(a, b) for a, b in zip(case.forward(E.Plain()), refs))
    assert tuple(refs[0].shape) == tuple(case.dy.shape) and tuple(refs[1].shape) == tuple(case.x.shape) and tuple(refs[2].shape) == tuple(case.w.shape)
    indexing_faults_change(dx, refs[1])
    # the reference IS autograd's: the three products are the step's y and its two gradients
    xr, wr = case.x.double().requires_grad_(True), case.w.double().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, None, g.stride, (g.ph, g.pw), (g.dh, g.dw))
    gx, gw = torch.autograd.grad(yr, (xr, wr), case.dy.double())
    assert torch.equal(yr.detach(), refs[0]) and torch.equal(gx, refs[1]) and torch.equal(gw, refs[2])


def test_one_step_chunk_case():
    case = E.ConvLayerCase(E.ONE_STEP_GEOM, "A")
    ref = check_case(case, (BF16X6, F16X3))
    must_change(case, E.FaultLastKBlock(), ref, "the last k-block dropped")
    # what the race this case is for does: the third chunk where the first one belongs
    a = case.x.double().clone()
    a[:, :16] = a[:, 32:48]
    assert not torch.equal(case.op(a, case.w.double()), ref)


@pytest.mark.parametrize("geom", E.TRAIN_CONVT_GEOMS)
def test_train_conv_transpose_cases(geom):
    case = E.TrainConvTCase(*geom)
    y, dx = case.legs()
    refs = [check_case(leg, (BF16X6, F16X3)) for leg in (y, dx)]
    assert tuple(refs[1].shape) == tuple(case.x.shape)
    indexing_faults_change(y, refs[0])
    indexing_faults_change(dx, refs[1])
    B, cin, cout, k, s, p, op, H, W = geom
    xr = case.x.double().requires_grad_(True)
    yr = torch.nn.functional.conv_transpose2d(xr, case.w.double(), None, s, p, op)
    assert torch.equal(yr.detach(), refs[0]) and torch.equal(torch.autograd.grad(yr, xr, case.dy.double())[0], refs[1])


def test_train_conv_geometries_name_who_takes_each_leg():
    """The table's last two columns restate the conditions of hipnn._Conv2d.backward and hipnn._wgrad_hip (LAV_TRAIN_WGRAD_MINPIX=1)."""
    for g in E.TRAIN_CONV_GEOMS:
        case = E.TrainConvCase(g)
        oph, opw = case.out_pad
        oh, ow = case.fwd.out_hw()
        strided_off = dict(g.env).get("LAV_TRAIN_DGRAD_STRIDED") == "torch" and g.stride != 1
        dgrad = "lib" if (oph == opw and 0 <= oph < g.stride and (g.dh, g.dw) == (1, 1) and not strided_off) else "torch"
        assert g.dgrad == (dgrad if g.x_grad else None), g.name
        wgrad = (g.kh == g.kw and ((g.kh == 3 and g.stride in (1, 2)) or (g.kh == 7 and g.stride == 2)) and (g.ph, g.pw) == (g.kh // 2, g.kh // 2)
                 and (g.dh, g.dw) == (1, 1) and g.W % (4 * g.stride) == 0 and g.H % g.stride == 0 and g.cin % 64 == 0 and g.cout % 64 == 0
                 and (oh, ow) == (g.H // g.stride, g.W // g.stride))
        assert g.wgrad == ("lib" if wgrad else "torch"), g.name
    took = lambda leg, who: sorted({g.name[0] for g in E.TRAIN_CONV_GEOMS if getattr(g, leg) == who})
    assert took("dgrad", "lib") == list("abcfghijlm") and took("dgrad", "torch") == list("dek")
    assert took("wgrad", "lib") == list("abefm") and took("wgrad", "torch") == list("cdghijkl")


@pytest.mark.parametrize("H,W,B", [(H, W, 1) for H, W in E.BACKBONE_CANVASES] + [E.BACKBONE_CANVASES[0] + (2,)])
def test_backbone_cases(H, W, B):
    from lav_amd.lidar import ConvBackbone
    bb = ConvBackbone(64)
    params = E.fill_backbone(bb)
    case = E.BackboneCase(params, B, H, W)
    ref = check_case(case, PRECISIONS)
    must_change(case, E.FaultShiftedTap(), ref, "a tap shifted by one")
    must_change(case, E.FaultHaloColumn(), ref, "a halo column zeroed")
    assert tuple(ref.shape) == (B, 384, H // 2, W // 2)
    assert all(m.eps == 0.0 for m in bb.modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_emulator_sees_what_the_classes_are_for():
    """The specification itself: class D data at f16x3 is NOT exact (22 of 24 bits), a 24-bit pattern against a two-piece weight loses
    a1 b1 at f16x3, and an extra tap on one output channel can make a float64 result that fp32 cannot hold - the precondition reports it."""
    g = next(g for g in GEOMS if g.name.startswith("3x3 s1 64->64"))
    case = E.ConvLayerCase(g, "D")
    ref = case.forward(E.Plain())
    assert not torch.equal(case.forward(E.Emulator(F16X3)), ref)
    with pytest.raises(AssertionError, match="precondition 2"):
        E.preconditions(case, F16X3)
    case = E.ConvLayerCase(g, "B")
    idx = tuple(int(v) for v in (case.w[0] != 0).nonzero()[0])
    other = ((idx[0] + 1) % g.cin, idx[1], idx[2])
    case.w[0][other] = 1.0                      # a second tap on output channel 0: two 21-bit terms of unrelated exponents
    with pytest.raises(AssertionError, match="precondition"):
        E.preconditions(case, F16X3)
