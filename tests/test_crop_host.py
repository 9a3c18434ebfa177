"""The float64 reference of the rotated-crop tests, checked on the host: tests/crop_util.crop_matrix_f64 (written from the formulas in
crop.hip's header) against planner_common.crop_feature_torch (affine_grid + grid_sample) run in float64 on identity maps, at every
geometry and pose tests/test_gpu_crop.py uses; the poses are what their names say; and the kernel each geometry reaches."""
import numpy as np
import pytest
import torch

from tests import crop_util as cu

GEOMS = list(cu.GEOMETRIES)


@pytest.mark.parametrize("geom", GEOMS, ids=cu.geom_id)
def test_crop_matrix_f64_matches_grid_sample_in_float64(geom):
    H, W, crop = geom
    worst = 0.0
    for ox, oy in cu.OFFSETS:
        locs, oris, kinds = cu.poses(H, W, crop, ox, oy)
        for sl in cu.chunks(len(kinds)):
            mine = cu.crop_matrix_f64(H, W, crop, locs[sl].numpy(), oris[sl].numpy(), cu.PPM, ox, oy)
            ref = cu.torch_crop_matrix(H, W, crop, locs[sl], oris[sl], cu.PPM, ox, oy, torch.float64).numpy()
            err = np.abs(mine - ref).max(axis=(1, 2))
            worst = max(worst, float(err.max()))
            for j, e in enumerate(err):
                i = sl.start + j
                assert e <= 1e-12, f"{geom} offset ({ox}, {oy}) pose {i} ({kinds[i]}, ori {float(oris[i]):.4f}): max |diff| {e:.3e}"
    print(f"{cu.geom_id(geom)}: max |crop_matrix_f64 - grid_sample float64| = {worst:.3e}")


@pytest.mark.parametrize("geom", GEOMS, ids=cu.geom_id)
def test_poses_are_what_their_names_say(geom):
    """`off_map` leaves no sample within one pixel of the map, `half_off` leaves part of the crop inside and part outside, every
    other pose has samples inside; no output pixel has more than four weights.  Where the pitch is exactly 1 the zero / whole-pixel
    / half-pixel shifts at ori = 0 and the `centred` poses at the four axis-aligned orientations sample the half-pixel lattice."""
    H, W, crop = geom
    for ox, oy in cu.OFFSETS:
        locs, oris, kinds = cu.poses(H, W, crop, ox, oy)
        assert sorted(set(kinds)) == sorted(cu.LOC_KINDS) and len(kinds) == len(cu.LOC_KINDS) * len(cu.ORIS)
        ix, iy = cu.crop_positions_f64(H, W, crop, locs.numpy(), oris.numpy(), cu.PPM, ox, oy)
        A = cu.crop_matrix_f64(H, W, crop, locs.numpy(), oris.numpy(), cu.PPM, ox, oy)
        mass = A.sum(axis=2)                                  # (n, crop^2): 1 inside the map, 0 outside, between on the rim
        for i, kind in enumerate(kinds):
            inside = (ix[i] > -1) & (ix[i] < W) & (iy[i] > -1) & (iy[i] < H)
            if kind == "off_map":
                assert not inside.any() and not A[i].any(), f"{geom} pose {i}: an off-map crop touches the map"
            elif crop == 2:           # (four samples only: nothing to say about where most of them are)
                pass
            elif kind == "half_off":
                assert (mass[i] == 0).any() and (mass[i] > 0.99).any(), f"{geom} pose {i}: not half off the map"
            else:
                assert (mass[i] > 0.99).any(), f"{geom} pose {i} ({kind}): no sample inside the map"
            on_lattice = kind == "centred" and i % len(cu.ORIS) < 4 or kind in ("zero", "whole_pixel", "half_pixel") and i % len(cu.ORIS) == 0
            if geom == (12, 12, 12) and on_lattice:
                twice = 2 * np.stack([ix[i], iy[i]])
                assert np.abs(twice - np.round(twice)).max() < 1e-5, f"pose {i} ({kind}): not on the half-pixel lattice"
        assert (np.count_nonzero(A, axis=2) <= 4).all()


def test_kernel_choice_of_every_geometry():
    """The float32 restatement of crop_fwd_staged_ok / crop_bwd_staged_ok gives the dispatch the GPU tests rely on: the general
    backward is reached only by the H > W geometry (4 candidates per axis), every staged box bound stays clear of the limit of 32,
    and square maps - whatever the crop size - never leave the staged backward."""
    for (H, W, crop), (fwd, bwd) in cu.GEOMETRIES.items():
        staged, span, box = cu.bwd_staged(H, W, crop)
        assert ("staged" if cu.fwd_staged_ok(H, W, crop) else "general") == fwd, (H, W, crop)
        assert ("staged" if staged else "general") == bwd, (H, W, crop, span, box)
        if staged:
            assert span == 3 and box <= 27.5, (H, W, crop, span, box)
    assert cu.bwd_staged(28, 20, 14)[1] == 4
    for H in (12, 24, 40, 56, 80, 160, 320):
        for crop in (2, 3, 13, 24, 33, 96, H):
            if crop <= H:
                staged, span, box = cu.bwd_staged(H, H, crop)
                assert staged and span <= 3, (H, crop, span, box)
