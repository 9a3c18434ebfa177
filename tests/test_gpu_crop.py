"""The four rotated-crop kernels of crop.hip (k_crop_rotate, k_crop_rotate_staged, k_crop_rotate_bwd, k_crop_rotate_bwd_general)
read out as matrices.  The crop is linear in the map, so on a small geometry the forward's weights come out bit for bit from a
crop of identity maps (one channel per map pixel) and the backward's from one-hot output gradients (one channel per output pixel):

  * the backward matrix EQUALS the forward matrix (crop.hip: "the transpose of the forward, not an approximation of it") - one
    missed candidate of any size, anywhere, fails it; no tolerance;
  * the forward matrix is the same through every entry point and from both forward kernels;
  * crops that share a map are summed in index order in float32, across the kernel's passes of 256 crops too;
  * the forward matrix is within the float32 error of the formula of tests/crop_util.crop_matrix_f64 (float64; itself checked
    on the host in tests/test_crop_host.py).

Geometries and the kernel each one reaches: tests/crop_util.GEOMETRIES.  (28, 20, 14) is the one that reaches the general backward
on its own - it takes a map with H > W - and the only one with 4 candidates per axis."""
import numpy as np
import pytest
import torch

from lav_amd import ops
from tests import crop_util as cu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PPM = cu.PPM
GEOMS = list(cu.GEOMETRIES)
KNOBS = {"fwd_general": "LAV_CROP_FWD_GENERAL", "bwd_general": "LAV_CROP_BWD_GENERAL"}    # (read by the library on every call)
# the library's own choice of kernels at every geometry; the square ones (staged / staged) again with each general kernel forced
CASES = [(g, "dispatch") for g in GEOMS] + [(g, k) for g in cu.SQUARE for k in KNOBS]
BWD_CASES = [c for c in CASES if c[1] != "fwd_general"]


def case_id(case):
    return f"{cu.geom_id(case[0])}-{case[1]}"


def select(monkeypatch, kernels):
    for name, var in KNOBS.items():
        if name == kernels:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)


def forward_matrix(geom, off, locs, oris, route="indexed"):
    """(n, crop^2, H W): out[i].view(H W, crop^2).T of a crop of the identity maps - each value is one weight x 1.0 plus exact zeros."""
    H, W, crop = geom
    n = locs.shape[0]
    basis = torch.eye(H * W, device=DEV).view(1, H * W, H, W)
    if route == "indexed":
        out = ops.crop_rotate_indexed(basis, torch.zeros(n, dtype=torch.int32, device=DEV), locs, oris, PPM, crop, *off)
    elif route == "shared":
        out = ops.crop_rotate(basis, locs, oris, PPM, crop, *off)
    else:                          # one map per crop (eight at a time: a copy of the basis each)
        out = torch.cat([ops.crop_rotate(basis.expand(sl.stop - sl.start, -1, -1, -1).contiguous(), locs[sl], oris[sl], PPM, crop, *off)
                         for sl in cu.chunks(n)])
    return out.view(n, H * W, crop * crop).transpose(1, 2)


def one_hot_grads(crop, n):
    return torch.eye(crop * crop, device=DEV).view(1, crop * crop, crop, crop).expand(n, -1, -1, -1)


def map_gradient(geom, off, locs, oris, map_index, num_maps):
    """Gradient w.r.t. `num_maps` maps of crop^2 channels for grad_out[i] = eye(crop^2): (num_maps, crop^2, H W).  Every product
    the kernel adds is fmaf(w, 1, acc)."""
    H, W, crop = geom
    feats = torch.zeros((num_maps, crop * crop, H, W), device=DEV, requires_grad=True)
    out = ops.crop_rotate_indexed(feats, map_index, locs, oris, PPM, crop, *off)
    out.backward(one_hot_grads(crop, locs.shape[0]))
    return feats.grad.view(num_maps, crop * crop, H * W)


def backward_matrix(geom, off, locs, oris):
    n = locs.shape[0]
    return map_gradient(geom, off, locs, oris, torch.arange(n, dtype=torch.int32, device=DEV), n)


def difference(got, want, geom, names, what):
    """Where two (n, crop^2, H W) weight tensors differ: how many entries, and the first one spelled out."""
    H, W, crop = geom
    ne = got != want
    i, r, c = (int(v) for v in ne.nonzero()[0])
    return (f"{cu.geom_id(geom)}: {int(ne.sum())} weights differ in {int(ne.flatten(1).any(1).sum())} of {got.shape[0]} matrices; first: {names[i]}, "
            f"output pixel (y {r // crop}, x {r % crop}), map pixel (sy {c // W}, sx {c % W}): {what[0]} {float(got[i, r, c]):.9e}, "
            f"{what[1]} {float(want[i, r, c]):.9e}")


_poses, _matrices = {}, {}


def poses(geom, off):
    if (geom, off) not in _poses:
        locs, oris, kinds = cu.poses(*geom, *off)
        names = [f"pose {i} ({k}, ori {float(o):.4f}, offsets {off})" for i, (k, o) in enumerate(zip(kinds, oris))]
        _poses[geom, off] = (locs, oris, kinds, names)
    return _poses[geom, off]


def matrices(monkeypatch, geom, off):
    """Forward and backward matrices of every pose from the kernels the library picks on its own (computed once per session)."""
    if (geom, off) not in _matrices:
        select(monkeypatch, "dispatch")
        locs, oris, _, _ = poses(geom, off)
        _matrices[geom, off] = (forward_matrix(geom, off, locs.to(DEV), oris.to(DEV)), backward_matrix(geom, off, locs.to(DEV), oris.to(DEV)))
    return _matrices[geom, off]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_matrix_equals_forward_matrix(case, monkeypatch):
    geom, kernels = case
    select(monkeypatch, kernels)
    for off in cu.OFFSETS:
        locs, oris, kinds, names = poses(geom, off)
        fwd = forward_matrix(geom, off, locs.to(DEV), oris.to(DEV))
        bwd = backward_matrix(geom, off, locs.to(DEV), oris.to(DEV))
        assert float(fwd.abs().max()) > 0
        if not torch.equal(bwd, fwd):
            pytest.fail(f"{kernels}: " + difference(bwd, fwd, geom, names, ("backward", "forward")))


@pytest.mark.parametrize("geom", GEOMS, ids=cu.geom_id)
def test_forward_matrix_is_the_same_through_every_route_and_kernel(geom, monkeypatch):
    """lav_crop_rotate with one shared map, with one map per crop, lav_crop_rotate_indexed; the staged and the gathering kernel."""
    for off in cu.OFFSETS:
        locs, oris, kinds, names = poses(geom, off)
        ref, _ = matrices(monkeypatch, geom, off)
        for kernels in ("dispatch", "fwd_general"):
            select(monkeypatch, kernels)
            for route in ("indexed", "shared", "per_sample"):
                got = forward_matrix(geom, off, locs.to(DEV), oris.to(DEV), route)
                if not torch.equal(got, ref):
                    pytest.fail(f"{kernels}, {route}: " + difference(got, ref, geom, names, (route, "indexed (library's choice)")))


@pytest.mark.parametrize("geom", GEOMS, ids=cu.geom_id)
def test_matrix_structure(geom, monkeypatch):
    """A crop entirely off the map is all zeros, forward and backward; an output pixel has at most four weights; where all four
    corners are inside the map they sum to 1 within 4 * 2^-23 (four float32 roundings of products of weights that are themselves
    1 - w).  "Inside" is decided in float64 with a margin of 1e-3 pixels, a hundred times the float32 error of a sample position
    on these maps: rows nearer to the rim than that are not summed (the accuracy test covers them)."""
    H, W, crop = geom
    interior_rows = 0
    for off in cu.OFFSETS:
        locs, oris, kinds, names = poses(geom, off)
        fwd, bwd = matrices(monkeypatch, geom, off)
        for i, kind in enumerate(kinds):
            if kind == "off_map":
                assert not fwd[i].any() and not bwd[i].any(), f"{names[i]}: weights for a crop that is off the map"
        assert int((fwd != 0).sum(dim=2).max()) <= 4
        ix, iy = cu.crop_positions_f64(H, W, crop, locs.numpy(), oris.numpy(), PPM, *off)
        inside = (ix >= 1e-3) & (ix <= W - 1 - 1e-3) & (iy >= 1e-3) & (iy <= H - 1 - 1e-3)
        inside = torch.from_numpy(inside.reshape(len(kinds), -1)).to(DEV)
        sums = fwd.double().sum(dim=2)
        err = (sums - 1.0).abs()[inside]
        interior_rows += int(inside.sum())
        assert err.numel() == 0 or float(err.max()) <= 4 * 2.0 ** -23, f"offsets {off}: row sum off by {float(err.max()):.3e}"
    assert interior_rows > 0


PICK = (0, 9, 18, 27, 44, 5, 14, 36, 47)       # nine of the poses; 27 is half off the map, 36 entirely (adds exact zeros mid-sum)
SHARED = (1, 0, 0, 1, 1, 0, 1, 0, 0)


def ordered_sum(fwd, map_index, num_maps):
    """Sequential float32 sum, in index order, of the forward matrices of the crops of each map (on the CPU)."""
    fwd = fwd.cpu()
    want = torch.zeros((num_maps,) + tuple(fwd.shape[1:]), dtype=torch.float32)
    for i, m in enumerate(map_index):
        want[m] = want[m] + fwd[i]
    return want


@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_crops_sharing_a_map_are_summed_in_index_order(case, monkeypatch):
    geom, kernels = case
    off = cu.OFFSETS[0]
    locs, oris, kinds, names = poses(geom, off)
    pick = torch.tensor(PICK)
    want = ordered_sum(matrices(monkeypatch, geom, off)[0][pick.to(DEV)], SHARED, 2)
    assert float(want[0].abs().max()) > 0 and float(want[1].abs().max()) > 0
    select(monkeypatch, kernels)
    got = map_gradient(geom, off, locs[pick].to(DEV), oris[pick].to(DEV), torch.tensor(SHARED, dtype=torch.int32, device=DEV), 2).cpu()
    if not torch.equal(got, want):
        pytest.fail(f"{kernels}: " + difference(got, want, geom, ["map 0", "map 1"], ("map gradient", "ordered float32 sum")))


@pytest.mark.parametrize("kernels", ["dispatch", "bwd_general"])
def test_more_than_256_crops_in_one_launch(kernels, monkeypatch):
    """300 crops of two maps: the backward takes its crops in passes of 256 and compacts each pass in index order; the sum must
    still be the index-ordered one, and the same bits on every run."""
    geom, off, n = (12, 12, 12), cu.OFFSETS[0], 300
    locs, oris = (t.to(DEV) for t in cu.random_poses(12, 12, n, seed=7))
    map_index = [i % 2 for i in range(n)]
    select(monkeypatch, "dispatch")
    want = ordered_sum(forward_matrix(geom, off, locs, oris), map_index, 2)
    select(monkeypatch, kernels)
    idx = torch.tensor(map_index, dtype=torch.int32, device=DEV)
    first = map_gradient(geom, off, locs, oris, idx, 2)
    second = map_gradient(geom, off, locs, oris, idx, 2)
    assert torch.equal(first, second), "two runs of the backward differ"
    if not torch.equal(first.cpu(), want):
        pytest.fail(f"{kernels}: " + difference(first.cpu(), want, geom, ["map 0", "map 1"], ("map gradient", "ordered float32 sum")))


@pytest.mark.parametrize("geom", GEOMS, ids=cu.geom_id)
def test_forward_matrix_against_float64(geom, monkeypatch):
    """max |A_fwd - crop_matrix_f64| <= min(4 e_ref, 2e-5), where e_ref is the error of the SAME formula evaluated in float32 by
    torch on the CPU (affine_grid + grid_sample) over the same cases - the reference's own float32 error, never the kernel's.
    Both are float32 evaluations of one formula in a different order with a different sinf / cosf: four times the reference's
    error covers that and nothing more.  Measured on an MI355X (printed below; recorded in DESIGN.md 4.5)."""
    H, W, crop = geom
    e_ref, e_ker, worst = 0.0, 0.0, ""
    for off in cu.OFFSETS:
        off = tuple(float(np.float32(v)) for v in off)        # the offsets as the C ABI receives them
        locs, oris, kinds, names = poses(geom, off)
        select(monkeypatch, "dispatch")
        fwd = forward_matrix(geom, off, locs.to(DEV), oris.to(DEV))
        for sl in cu.chunks(len(kinds)):
            exact = cu.crop_matrix_f64(H, W, crop, locs[sl].numpy(), oris[sl].numpy(), PPM, *off)
            ref32 = cu.torch_crop_matrix(H, W, crop, locs[sl], oris[sl], PPM, *off, torch.float32).double().numpy()
            ker = fwd[sl].cpu().double().numpy()
            e_ref = max(e_ref, float(np.abs(ref32 - exact).max()))
            err = np.abs(ker - exact).max(axis=(1, 2))
            if float(err.max()) > e_ker:
                e_ker, worst = float(err.max()), names[sl.start + int(err.argmax())]
    tol = min(4 * e_ref, 2e-5)
    print(f"\n{cu.geom_id(geom)}: e_ref (torch float32 on the CPU vs float64) {e_ref:.3e}, kernel vs float64 {e_ker:.3e} at {worst}, allowed {tol:.3e}")
    assert e_ker <= tol, f"{cu.geom_id(geom)}: kernel {e_ker:.3e} > min(4 x {e_ref:.3e}, 2e-5) at {worst}"


@pytest.mark.parametrize("H,W,crop", [(20, 28, 14), (28, 20, 14)])
def test_non_square_maps_forward_backward_vs_grid_sample_float64(H, W, crop):
    """The data-level comparison of test_gpu_train.py::test_crop_rotate_indexed_forward_backward_vs_grid_sample (its tolerances) on
    the two non-square geometries, against grid_sample in float64: the general forward with the staged backward, and the staged
    forward with the general backward at 4 candidates per axis."""
    from lav_amd.planner_common import crop_feature_torch
    g = torch.Generator().manual_seed(4)
    feat = torch.randn((3, 40, H, W), generator=g)            # 40 channels: one full and one ragged channel block
    idx = torch.tensor([2, 0, 0, 1, 2], dtype=torch.int32)     # maps 0 and 2 are shared by two crops each
    locs = torch.tensor([[0.0, 0.0], [1.5, -3.0], [-2.0, 1.0], [3.0, -2.0], [6.0, -6.0]])          # the last one mostly off the map
    oris = torch.tensor([0.0, 0.4, -1.1, 3.0, 0.2])
    f_ref = feat.double().requires_grad_(True)
    f_gpu = feat.to(DEV).requires_grad_(True)
    out = ops.crop_rotate_indexed(f_gpu, idx.to(DEV), locs.to(DEV), oris.to(DEV), 2.0, crop, 0.0, 0.75)
    ref = crop_feature_torch(f_ref[idx.long()], locs.double(), oris.double(), 2.0, crop, 0.0, 0.75)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-5)
    w = torch.randn(ref.shape, generator=g)
    (out * w.to(DEV)).sum().backward()
    (ref * w.double()).sum().backward()
    np.testing.assert_allclose(f_gpu.grad.cpu().numpy(), f_ref.grad.numpy(), rtol=0, atol=5e-5 * float(f_ref.grad.abs().max()))
    assert all(float(f_ref.grad[m].abs().sum()) > 0 for m in range(3))
    first = f_gpu.grad.clone()
    f_gpu.grad = None
    out2 = ops.crop_rotate_indexed(f_gpu, idx.to(DEV), locs.to(DEV), oris.to(DEV), 2.0, crop, 0.0, 0.75)
    (out2 * w.to(DEV)).sum().backward()
    assert torch.equal(first, f_gpu.grad)                                                       # run-to-run identical bits


_single = {}


def single_data(geom):
    """40 random channels of one map and an output gradient per pose, once per geometry: at 32 channels per workgroup one whole and
    one partial block, at 16 (what the staged forward takes for a single crop) two whole and one partial."""
    if geom not in _single:
        H, W, crop = geom
        g = torch.Generator().manual_seed(11)
        _single[geom] = (torch.randn((1, 40, H, W), generator=g).to(DEV), torch.randn((16, 40, crop, crop), generator=g).to(DEV))
    return _single[geom]


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("geom", [(24, 24, 13), (40, 40, 24)], ids=cu.geom_id)
def test_one_and_two_crops_staged_kernels_equal_the_general_ones(geom, n, monkeypatch):
    """A launch of a single crop (and of two, the first count that takes 32 channels per workgroup again) on random data, which the
    matrix tests above do not make: the staged forward gives the gathering forward's bits and the staged backward the general
    backward's, at 16 of the poses (every third: all six kinds of location), the crops of a launch sharing the one map."""
    assert cu.GEOMETRIES[geom] == ("staged", "staged")
    off = cu.OFFSETS[0]
    locs, oris, kinds, names = poses(geom, off)
    feat, grads = single_data(geom)
    pick = list(range(0, 48, 3))
    assert len(pick) == 16 and {kinds[i] for i in pick} == set(cu.LOC_KINDS)
    largest = 0.0
    for a in range(0, 16, n):
        sel = torch.tensor(pick[a:a + n])
        lo, orr, idx = locs[sel].to(DEV), oris[sel].to(DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        got = {}
        for kernels in ("dispatch", "fwd_general", "bwd_general"):
            select(monkeypatch, kernels)
            f = feat.clone().requires_grad_(True)
            out = ops.crop_rotate_indexed(f, idx, lo, orr, PPM, geom[2], *off)
            out.backward(grads[a:a + n])
            got[kernels] = (out.detach(), f.grad)
        what = ", ".join(names[i] for i in sel.tolist())
        assert torch.equal(got["dispatch"][0], got["fwd_general"][0]), f"{cu.geom_id(geom)}: staged forward != gathering forward at {what}"
        assert torch.equal(got["dispatch"][0], ops.crop_rotate(feat, lo, orr, PPM, geom[2], *off)), f"lav_crop_rotate differs at {what}"
        assert torch.equal(got["dispatch"][1], got["bwd_general"][1]), f"{cu.geom_id(geom)}: staged backward != general backward at {what}"
        largest = max(largest, float(got["dispatch"][1].abs().max()))
    assert largest > 0
