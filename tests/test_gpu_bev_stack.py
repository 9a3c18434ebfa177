"""lav_bev_stack_u8 (csrc/bev_stack.hip) on the GPU against the specification lav_amd.data.bev_stack.bev_stack_numpy.  Every comparison
is bit-exact: single warps over many angles (a contracted multiply-add in the inverse map would move a coordinate), double warps with
shifts, raw and thresholded, zero outputs, the staged and the direct path (which one a case takes is asserted from the launcher's own
rule, ops.bev_stack_tile_paths), batch independence, the five loaders, and train_bev_v2.py --bev-on-device."""
import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.data import bev_stack as S
from lav_amd.data import datasets, image
from tests.bev_stack_util import BEV_AT, LOADER_CASES, assert_same_sample, default_samples, draw, make_routes, run_driver

pytestmark = pytest.mark.gpu
IDENT = np.array(image.IDENTITY_INVERSE_MAP)
ANGLES = (0.0, 90.0, -90.0, 180.0, 1e-3, 7.3, -19.99, 33.3)


def rotation(angle, hw, scale=1.0):
    """Rotation about the point that BEV_CENTER is in a 320 x 320 map: (w / 2, 0.875 h)."""
    return image.inverse_map(image.rotation_matrix_2d((hw[1] / 2, 0.875 * hw[0]), angle, scale))


def dense(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def sparse(shape, seed):
    """Random grey levels on about a sixth of the 8 x 8 blocks, zero elsewhere: a thresholded output that is neither all 0 nor all 1."""
    r = np.random.default_rng(seed)
    n, h, w = shape
    blocks = r.random((n, h // 8 + 1, w // 8 + 1)) < 1 / 6
    mask = np.kron(blocks, np.ones((8, 8), bool))[:, :h, :w]
    return dense(shape, seed + 1) * mask


def run_gpu(planes, coef, shift, threshold=True):
    out = ops.bev_stack_u8(torch.from_numpy(planes).cuda(), coef, shift, threshold)
    assert out.dtype == torch.uint8 and out.shape == planes.shape and out.is_cuda
    return out.cpu().numpy()


def check(planes, coef, shift, threshold, what):
    got, want = run_gpu(planes, coef, shift, threshold), S.bev_stack_numpy(planes, coef, shift, threshold)
    bad = got != want
    print(f"{what}: {got.size} pixels, {int(bad.sum())} differ, {int((want > 0).sum())} non-zero in the reference")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} pixels differ, first at {np.argwhere(bad)[0].tolist()}"
    return got


def paths(coef, shift, hw):
    return [ops.bev_stack_tile_paths(c, s, *hw) for c, s in zip(np.asarray(coef).reshape(-1, 12), np.asarray(shift).reshape(-1, 2))]


# ---------------------------------------------------------------------------------------------------------- single warp
@pytest.mark.parametrize("hw", [(37, 53), (64, 64), (1, 1), (320, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_warp_raw_values(hw):
    """W2 = identity, threshold off: the interpolated values of one warp, one plane per angle in one launch."""
    angles = list(ANGLES)
    if hw == (37, 53):
        angles += np.random.default_rng(53).uniform(-180, 180, 64).tolist()
    n = len(angles)
    coef = np.stack([np.concatenate([rotation(a, hw), IDENT]) for a in angles])
    got = check(dense((n, *hw), seed=hw[0]), coef, np.zeros((n, 2), np.int32), False, f"single warp {hw}, {n} angles")
    assert all(p[2] == 0 for p in paths(coef, np.zeros((n, 2), np.int32), hw))         # every tile staged in LDS (or zero)
    if hw != (1, 1):
        assert got.any()


# ---------------------------------------------------------------------------------------------------------- double warp
SHIFTS = ((0, 0), (32, -32), (-32, 32), (5, -17))
PAIRS = ((7.3, -19.99), (0.0, 12.5), (-33.3, 20.0), (180.0, 1e-3), (1.9, 0.0))      # (W1, W2): both, identity W1, ..., identity W2


@pytest.mark.parametrize("threshold", [False, True], ids=["raw", "thresholded"])
@pytest.mark.parametrize("hw", [(37, 53), (320, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_double_warp_with_shifts(hw, threshold):
    coef = np.stack([np.concatenate([rotation(a1, hw), rotation(a2, hw)]) for a1, a2 in PAIRS for _ in SHIFTS])
    shift = np.array([s for _ in PAIRS for s in SHIFTS], np.int32)
    planes = (sparse if threshold else dense)((len(coef), *hw), seed=hw[1])
    got = check(planes, coef, shift, threshold, f"double warp {hw} threshold={threshold}")
    assert all(p[2] == 0 for p in paths(coef, shift, hw))
    if threshold and hw == (320, 320):
        assert set(np.unique(got)) == {0, 1} and 0.05 < got.mean() < 0.6


# ------------------------------------------------------------------------------------------------------------- zeros
def test_zero_outputs():
    hw = (320, 320)
    far = np.concatenate([IDENT, rotation(10.0, hw)])
    far[4] = 1e6                                      # W1 samples a million pixels right of the image
    off = np.concatenate([rotation(3.0, hw), rotation(10.0, hw)])
    coef = np.stack([far, off, np.concatenate([rotation(3.0, hw), rotation(10.0, hw)])])
    shift = np.array([[0, 0], [0, 400], [5, -17]], np.int32)          # plane 1: the shift leaves the image
    planes = dense((3, *hw), seed=4)
    planes[2] = 0                                     # plane 2: a zero plane (a missing history frame)
    assert paths(coef[:2], shift[:2], hw) == [(50, 0, 0), (50, 0, 0)]
    for threshold in (False, True):
        assert not check(planes, coef, shift, threshold, f"zero outputs threshold={threshold}").any()


# -------------------------------------------------------------------------------------------------------- both paths
def test_staged_and_direct_paths():
    """At 320 x 320.  Staged: rotations - the 64 x 32 tile's footprint in W1(src) is at most 70 x 70 bytes, its footprint in src at most
    101 x 101, inside the 8 KiB + 16 KiB LDS budget whatever the angles (also 90 degrees then 45).  Direct: W1 shrinks the source to a
    third, or to 0.45 about the centre (a source footprint of 3 x 3 or 2.2 x 2.2 times the area, beyond 16 KiB), under a 45 or 20 degree
    W2; the tiles that see nothing of the shrunken image stay zero, those at its rim may still fit."""
    hw = (320, 320)
    staged = np.stack([np.concatenate([rotation(90.0, hw), rotation(45.0, hw)]), np.concatenate([rotation(-12.0, hw), rotation(20.0, hw)])])
    about_centre = image.inverse_map(image.rotation_matrix_2d((160, 160), 30.0, 0.45))
    direct = np.stack([np.concatenate([rotation(90.0, hw, 1 / 3), rotation(45.0, hw)]), np.concatenate([about_centre, rotation(20.0, hw)])])
    shift = np.array([[5, -17], [-32, 32]], np.int32)
    ps, pd = paths(staged, shift, hw), paths(direct, shift, hw)
    print("tiles (zero, staged, direct): staged case", ps, "direct case", pd)
    assert all(p[2] == 0 and p[1] > 0 for p in ps)
    assert all(p[2] >= 5 for p in pd) and sum(p[2] for p in pd) >= 16
    for threshold in (False, True):
        make = sparse if threshold else dense
        assert check(make((2, *hw), seed=8), staged, shift, threshold, f"staged path threshold={threshold}").any()
        assert check(make((2, *hw), seed=9), direct, shift, threshold, f"direct path threshold={threshold}").any()


# -------------------------------------------------------------------------------------------------------------- batch
def test_a_planes_result_does_not_depend_on_its_batch():
    """B = 3, P = 9 at 140 x 150 (three columns and five rows of tiles, partial last ones; larger than the 16 KiB source budget, so a W1 that
    shrinks the source to a fifth takes the direct path), a different record per plane - staged, direct and zero planes mixed: every
    plane equals its own single-plane launch, two launches agree, and the batch matches the specification."""
    hw, r = (140, 150), np.random.default_rng(3)
    coef = np.stack([np.concatenate([rotation(r.uniform(-180, 180), hw, [1.0, 1.0, 0.2][k % 3]), rotation(r.uniform(-20, 20), hw)]) for k in range(27)])
    coef[4, :6] = IDENT
    coef[7, 6:] = IDENT
    coef[11, 4] = -1e5
    shift = r.integers(-32, 33, (27, 2)).astype(np.int32)
    planes = dense((27, *hw), seed=6)
    ps = paths(coef, shift, hw)
    assert any(p[2] > 0 for p in ps) and any(p[2] == 0 and p[1] > 0 for p in ps) and ps[11] == (15, 0, 0)
    shape = (3, 9, *hw)
    got = check(planes.reshape(shape), coef.reshape(3, 9, 12), shift.reshape(3, 9, 2), False, "batch 3 x 9")
    again = run_gpu(planes.reshape(shape), coef.reshape(3, 9, 12), shift.reshape(3, 9, 2), False)
    assert np.array_equal(got, again)
    flat = got.reshape(27, *hw)
    for k in range(27):
        assert np.array_equal(run_gpu(planes[k:k + 1], coef[k:k + 1], shift[k:k + 1], False)[0], flat[k]), k
    assert ops.bev_stack_u8(torch.zeros((0, 9, *hw), dtype=torch.uint8, device="cuda"), np.zeros((0, 9, 12)), np.zeros((0, 9, 2), np.int32)).shape == (0, 9, *hw)


def test_launch_refuses_overlapping_buffers():
    from lav_amd import _lib
    t = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    c = torch.from_numpy(np.tile(np.concatenate([IDENT, IDENT]), (2, 1))).cuda()
    s = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="overlap"):
        _lib.check(_lib.load().lav_bev_stack_u8(t.data_ptr(), c.data_ptr(), s.data_ptr(), t.data_ptr(), 2, 16, 16, 1, 0), "lav_bev_stack_u8")


# ------------------------------------------------------------------------------------------------------------ loaders
@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    return make_routes(str(tmp_path_factory.mktemp("bev_stack_routes_gpu")))


@pytest.mark.parametrize("name,picks", LOADER_CASES)
def test_deferred_loader_and_device_stacker_return_the_default_sample(routes, name, picks):
    want = default_samples(routes, name, picks)
    ds = datasets.LOADERS[name](routes)
    ds.bev_on_device = True
    stacker = S.BevStacker()
    for p in picks:
        got, after = draw(ds, p)
        bev = stacker(got[BEV_AT[name]], device=torch.device("cuda"))
        assert bev.is_cuda and bev.dtype == torch.uint8
        assert_same_sample(name, p, got, want[p][0], bev.cpu().numpy())
        assert after == want[p][1]


def test_device_and_host_stacker_agree_on_a_collated_batch(routes):
    class Args:
        config_path, seed, num_workers, batch_size = routes, 2021, 0, 4
    torch.manual_seed(3)
    np.random.seed(3)
    rec = next(iter(datasets.get_data_loader("temporal_lidar_painted", Args, bev_on_device=True)))[5]
    dev = S.BevStacker()(rec, device=torch.device("cuda"))
    assert tuple(dev.shape) == (4, 9, 320, 320) and torch.equal(dev.cpu(), S.BevStacker()(rec)) and dev.any()


def test_train_bev_driver_with_bev_on_device(tmp_path):
    """train_bev_v2.py --deterministic on the GPU over a recorded synthetic route, two steps of batch 2: the same losses with and
    without --bev-on-device."""
    cfg = make_routes(str(tmp_path), routes=1, frames=24)
    base = run_driver(cfg, str(tmp_path), "--deterministic")
    deferred = run_driver(cfg, str(tmp_path), "--deterministic", "--bev-on-device")
    print(base, deferred)
    assert base == deferred
