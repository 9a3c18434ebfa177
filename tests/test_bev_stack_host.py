"""The loaders' deferred BEV stacks on the host (lav_amd/data/bev_stack.py): a deferred loader plus BevStacker returns the default
loader's sample for all five BEV-bearing loaders, bev_stack_numpy is warp_affine_linear's arithmetic with the pad / slice shift, the
launcher's tile rule, and train_bev_v2.py --bev-on-device on the CPU."""
import os

import numpy as np
import pytest
import torch

from lav_amd import ops
from lav_amd.data import bev_stack as S
from lav_amd.data import datasets, image
from tests.bev_stack_util import BEV_AT, LOADER_CASES, assert_same_sample, default_samples, draw, make_routes, run_driver

IDENT = np.array(image.IDENTITY_INVERSE_MAP)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    return make_routes(str(tmp_path_factory.mktemp("bev_stack_routes")))


def rotation(angle, center=(160, 280), scale=1.0):
    return image.inverse_map(image.rotation_matrix_2d(center, angle, scale))


def images(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ loaders
@pytest.mark.parametrize("name,picks", LOADER_CASES)
def test_deferred_loader_and_stacker_return_the_default_sample(routes, name, picks):
    """Same seeds: the record rendered by BevStacker on the CPU is the default loader's `bev`, every other element is identical, and
    both paths leave torch's and NumPy's generators in the same state (the same draws in the same order)."""
    want = default_samples(routes, name, picks)
    ds = datasets.LOADERS[name](routes)
    ds.bev_on_device = True
    planes = 9 if "temporal" in name else 5
    for p in picks:
        got, after = draw(ds, p)
        rec = got[BEV_AT[name]]
        assert isinstance(rec, S.BevRecord)
        assert rec.planes.dtype == np.uint8 and rec.planes.shape == (planes, 320, 320)
        assert rec.coef.dtype == np.float64 and rec.coef.shape == (planes, 12) and rec.shift.dtype == np.int32 and rec.shift.shape == (planes, 2)
        if "temporal" in name and ds.idx_map[p] < 2:       # missing history: zero planes at the end of the stack
            assert not rec.planes[9 - 2 * (2 - ds.idx_map[p]):].any() and rec.planes[:5].any()
        if "temporal" not in name:
            assert np.array_equal(rec.coef[:, 6:], np.tile(IDENT, (5, 1)))
        bev = S.BevStacker()(rec)
        assert isinstance(bev, torch.Tensor) and bev.dtype == torch.uint8 and not bev.is_cuda
        assert_same_sample(name, p, got, want[p][0], bev.numpy())
        assert after == want[p][1], f"{name} sample {p}: the deferred path consumed other random draws"


def test_get_data_loader_collates_records(routes):
    class Args:
        config_path, seed, num_workers, batch_size = routes, 2021, 0, 4
    torch.manual_seed(3)
    np.random.seed(3)
    want = next(iter(datasets.get_data_loader("temporal_bev", Args)))
    torch.manual_seed(3)
    np.random.seed(3)
    loader = datasets.get_data_loader("temporal_bev", Args, bev_on_device=True)
    assert loader.dataset.bev_on_device and not datasets.LOADERS["temporal_bev"].bev_on_device
    got = next(iter(loader))
    rec = got[0]
    assert isinstance(rec, S.BevRecord)
    assert (rec.planes.dtype, tuple(rec.planes.shape)) == (torch.uint8, (4, 9, 320, 320))
    assert (rec.coef.dtype, tuple(rec.coef.shape)) == (torch.float64, (4, 9, 12)) and (rec.shift.dtype, tuple(rec.shift.shape)) == (torch.int32, (4, 9, 2))
    assert torch.equal(S.BevStacker()(rec), want[0])
    assert all(torch.equal(g, w) for g, w in zip(got[1:], want[1:]))
    with pytest.raises(ValueError, match="no BEV map"):
        datasets.get_data_loader("seg", Args, bev_on_device=True)


def test_a_shift_beyond_the_margin_raises_in_the_deferred_loader(routes):
    ds = datasets.TemporalBEVDataset(routes)
    ds.bev_on_device = True
    txn = ds.txn_map[3]
    for loc, y_offset in (((33, 0), 0), ((0, 33), 0), ((-33.5, 0), 0), ((0, 30), 3), ((0, -2), -31)):
        with pytest.raises(ValueError, match=r"frame 3\b.*shift"):
            ds._bev_channels(txn, 3, [1, 2], loc=loc, y_offset=y_offset)
    rec = ds._bev_channels(txn, 3, [1, 2], loc=(32.9, -32.9), y_offset=0)          # int() cuts towards zero, as in the default path
    assert rec.shift.tolist() == [[32, -32], [32, -32]]
    ds.bev_on_device = False
    assert np.array_equal(S.bev_stack_numpy(*rec), ds._bev_channels(txn, 3, [1, 2], loc=(32.9, -32.9), y_offset=0))


# ------------------------------------------------------------------------------------------------------ specification
@pytest.mark.parametrize("hw", [(320, 320), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_warp_of_the_specification_is_warp_affine_linear(hw):
    h, w = hw
    img = images((4, h, w), seed=h)
    for angle in (0.0, 90.0, -90.0, 180.0, 1e-3, 7.3, -19.99, 33.3):
        M = image.rotation_matrix_2d((w / 2, 0.875 * h), angle)
        coef = np.tile(np.concatenate([image.inverse_map(M), IDENT]), (4, 1))
        got = S.bev_stack_numpy(img, coef, np.zeros((4, 2), np.int32), threshold=False)
        want = image.warp_affine_linear(img.transpose(1, 2, 0), M).transpose(2, 0, 1)
        assert np.array_equal(got, want), angle
        assert np.array_equal(S.bev_stack_numpy(img, coef, np.zeros((4, 2), np.int32)), (want > 0).astype(np.uint8))
    # an identity W1 / W2 is skipped: the fixed-point path passes it exactly
    assert np.array_equal(image.warp_inverse_linear(img[0], IDENT), img[0])


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, -1), (-1, 1), (32, -32), (-32, 32), (32, 32)])
def test_shift_rule_is_pad_and_slice(shift):
    sr, sc = shift
    img = images((3, 320, 320), seed=7)
    ident = np.tile(np.concatenate([IDENT, IDENT]), (3, 1))
    got = S.bev_stack_numpy(img, ident, np.tile(np.array(shift, np.int32), (3, 1)), threshold=False)
    m = datasets.MARGIN
    want = np.pad(img, [[0, 0], [m, m], [m, m]])[:, sr + m:sr + m + 320, sc + m:sc + m + 320]
    assert np.array_equal(got, want)
    # and between two rotations: the temporal stack's host expression
    hwc = img.transpose(1, 2, 0)
    bev = datasets.rotate_image(hwc, 11.0)
    bev = np.pad(bev, [[m, m], [m, m], [0, 0]])[sr + m:sr + m + 320, sc + m:sc + m + 320]
    want2 = datasets.rotate_image(bev, -17.5).transpose(2, 0, 1)
    coef = np.tile(np.concatenate([rotation(11.0), rotation(-17.5)]), (3, 1))
    assert np.array_equal(S.bev_stack_numpy(img, coef, np.tile(np.array(shift, np.int32), (3, 1)), threshold=False), want2)


def test_specification_takes_leading_dimensions_and_refuses_bad_records():
    img = images((2, 3, 20, 24), seed=1)
    coef = np.stack([np.concatenate([rotation(5.0 * k, (12, 10)), rotation(-3.0 * k, (12, 10))]) for k in range(6)]).reshape(2, 3, 12)
    shift = np.arange(12, dtype=np.int32).reshape(2, 3, 2) - 5
    out = S.bev_stack_numpy(img, coef, shift, threshold=False)
    assert out.shape == img.shape and out.dtype == np.uint8
    for b in range(2):
        for p in range(3):
            assert np.array_equal(S.bev_stack_numpy(img[b, p][None], coef[b, p][None], shift[b, p][None], threshold=False)[0], out[b, p])
    assert np.array_equal(S.bev_stack_numpy(torch.from_numpy(img), torch.from_numpy(coef), torch.from_numpy(shift), threshold=False), out)
    with pytest.raises(ValueError, match="need coef"):
        S.bev_stack_numpy(img, coef[:, :2], shift)
    bad = coef.copy()
    bad[0, 0, 4] = np.nan
    with pytest.raises(ValueError, match="finite"):
        S.bev_stack_numpy(img, bad, shift)
    bad[0, 0, 4] = 2.0 ** 31
    with pytest.raises(ValueError, match="2\\^30"):
        S.bev_stack_numpy(img, bad, shift)


# ----------------------------------------------------------------------------------------------------------- plumbing
def test_tile_rule_of_the_launcher():
    """The kernel's per-tile choice, evaluated on the host: (zero, staged in LDS, direct from global memory) tiles of one plane."""
    tiles = 5 * 10                                                     # 64 x 32 tiles of a 320 x 320 plane
    ident = np.concatenate([IDENT, IDENT])
    assert ops.bev_stack_tile_paths(ident, (0, 0), 320, 320) == (0, tiles, 0)
    assert ops.bev_stack_tile_paths(ident, (0, 0), 37, 53) == (0, 2, 0)
    for a1, a2 in ((7.3, -19.99), (90.0, 45.0), (45.0, 45.0), (0.0, 20.0), (-20.0, 0.0)):      # no rotation leaves the LDS budget
        zero, staged, direct = ops.bev_stack_tile_paths(np.concatenate([rotation(a1), rotation(a2)]), (5, -17), 320, 320)
        assert direct == 0 and staged > 0 and zero + staged == tiles, (a1, a2)
    shrink = np.concatenate([rotation(90.0, scale=1 / 3), rotation(45.0)])      # W1 reads 3 x 3 source pixels per pixel
    zero, staged, direct = ops.bev_stack_tile_paths(shrink, (0, 0), 320, 320)
    assert direct > 0 and zero + staged + direct == tiles
    far = ident.copy()
    far[4] = 1e6                                                       # W1 reads 10^6 pixels to the right of the image
    assert ops.bev_stack_tile_paths(far, (0, 0), 320, 320) == (tiles, 0, 0)
    assert ops.bev_stack_tile_paths(ident, (0, 320), 320, 320) == (tiles, 0, 0)


def test_ops_bev_stack_u8_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bev_stack_u8(torch.zeros((1, 8, 8), dtype=torch.uint8), np.concatenate([IDENT, IDENT])[None], np.zeros((1, 2), np.int32))


def test_train_bev_driver_with_bev_on_device_on_the_cpu(tmp_path):
    """train_bev_v2.py --device cpu over a recorded synthetic route, two steps: the same losses with and without --bev-on-device."""
    cfg = make_routes(str(tmp_path), routes=1, frames=24)            # 4 samples: two batches of 2
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    base = run_driver(cfg, str(tmp_path), "--device", "cpu", env=env)
    deferred = run_driver(cfg, str(tmp_path), "--device", "cpu", "--bev-on-device", env=env)
    assert base == deferred
