"""Writes a small synthetic route in the data collector's LMDB layout (the keys lav/utils/datasets reads: `len`, `town`,
and per frame t `id_`, `loc_`, `ori_`, `bbox_`, `type_`, `nxp_`, `cmd_`, `bra_`, `lidar_`, `lidar_sem_`, `map_{0..11}_`; with
cameras=N also `rgb_{0..N-1}_` (colour PNG) and `sem_{0..N-1}_` (grayscale PNG of CARLA class ids), what the 'seg' loader reads;
with tel also `tel_rgb_` / `tel_sem_`, which the 'bra' loader reads besides the three middle cameras).
No recorded data ships with the reference (Git-LFS pointers), so this is what the loader tests and a no-download smoke
run of the trainers read:

    python -m lav_amd.data.synthetic_route <data_dir> [--routes 2] [--frames 40]
    python train_bev_v2.py --config-path <yaml with data_dir: <data_dir>> ...
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import image, lmdb_ro


def camera_images(r, cameras: int, hw=(72, 64)):
    """{key stem: PNG bytes} of one frame's `cameras` images: an RGB picture and its class-id map, blocks of CARLA classes (road,
    lane marks, vehicles, pedestrians, ...) with the colour of each block a noisy function of its class."""
    H, W = hw
    out = {}
    classes = np.array([0, 1, 4, 6, 7, 8, 10, 12], np.uint8)
    palette = r.integers(0, 256, (len(classes), 3))
    for c in range(cameras):
        cells = r.integers(0, len(classes), (H // 8 + 1, W // 8 + 1))
        k = np.kron(cells, np.ones((8, 8), np.int64))[:H, :W]
        sem = classes[k]
        rgb = np.clip(palette[k] + r.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        out[f"rgb_{c}"] = image.imencode_png(rgb)
        out[f"sem_{c}"] = image.imencode_png(sem)
    return out


def tel_images(r, hw=(72, 64)):
    """{key stem: PNG bytes} of one frame's telephoto camera: `tel_rgb` and `tel_sem`, drawn like camera_images' views."""
    H, W = hw
    classes = np.array([0, 1, 4, 6, 7, 8, 10, 12, 18], np.uint8)
    palette = r.integers(0, 256, (len(classes), 3))
    cells = r.integers(0, len(classes), (H // 8 + 1, W // 8 + 1))
    k = np.kron(cells, np.ones((8, 8), np.int64))[:H, :W]
    rgb = np.clip(palette[k] + r.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    return {"tel_rgb": image.imencode_png(rgb), "tel_sem": image.imencode_png(classes[k])}


def make_route(path: str, seed: int = 0, frames: int = 40, points: int = 2500, town: str = "Town01", sem_channels: int = 4,
               cameras: int = 0, camera_hw=(72, 64), tel: bool = False, tel_hw=(72, 64)) -> None:
    """cameras > 0: also per-frame camera images of camera_hw (H, W) pixels; tel: also the telephoto camera's `tel_rgb_` /
    `tel_sem_` of tel_hw (what the 'bra' loader reads).  Each has its own random stream: the other records are the same as
    without them, and the camera images the same with or without tel."""
    r = np.random.default_rng(seed)
    rc = np.random.default_rng([seed, 7919])
    rt = np.random.default_rng([seed, 7927])
    items = {b"len": str(frames).encode(), b"town": town.encode()}
    f32 = lambda a: np.asarray(a, np.float32).tobytes()
    # actors: ego (id 100, vehicle) drives a gentle arc; vehicles / pedestrians around it, some leave early
    n_veh, n_ped = 5, 3
    ids = np.array([100] + [200 + 7 * i for i in range(n_veh)] + [900 + 3 * i for i in range(n_ped)], np.int32)
    typ = np.array([1] + [1] * n_veh + [0] * n_ped, np.uint8)
    start = np.concatenate([[[10.0, -4.0]], r.uniform(-22, 22, (n_veh, 2)) + [10, -4], r.uniform(-8, 8, (n_ped, 2)) + [10, -4]])
    speed = np.concatenate([[0.35], r.uniform(0.0, 0.5, n_veh), r.uniform(0.0, 0.08, n_ped)])
    head = np.concatenate([[20.0], r.uniform(-180, 180, n_veh + n_ped)])
    turn = np.concatenate([[0.6], r.uniform(-1, 1, n_veh + n_ped)])
    box = np.concatenate([[[2.4, 1.0]], r.uniform([1.8, 0.8], [2.6, 1.1], (n_veh, 2)), r.uniform([0.3, 0.3], [0.5, 0.5], (n_ped, 2))])
    leaves_at = {int(ids[2]): frames // 2, int(ids[-1]): frames // 3}          # present in early frames only
    pos = start.copy()
    yy, xx = np.mgrid[0:320, 0:320]
    for t in range(frames):
        ang = head + turn * t
        keep = np.array([t < leaves_at.get(int(a), frames + 1) for a in ids])
        items[f"id_{t:05d}".encode()] = ids[keep].tobytes()
        items[f"loc_{t:05d}".encode()] = f32(pos[keep])
        items[f"ori_{t:05d}".encode()] = f32(ang[keep])
        items[f"bbox_{t:05d}".encode()] = f32(box[keep])
        items[f"type_{t:05d}".encode()] = typ[keep].tobytes()
        items[f"nxp_{t:05d}".encode()] = f32(pos[0] + 18 * np.array([np.cos(np.deg2rad(ang[0])), np.sin(np.deg2rad(ang[0]))]))
        items[f"cmd_{t:05d}".encode()] = np.array([(t // 7) % 6], np.uint8).tobytes()
        items[f"bra_{t:05d}".encode()] = np.array([int(t % 11 == 0)], np.uint8).tobytes()
        # LiDAR: ground ring + a few boxes, in the sensor frame; painted scores in [0, 1]
        rad = r.uniform(2.5, 45, points)
        az = r.uniform(-np.pi, np.pi, points)
        xyz = np.stack([rad * np.cos(az), rad * np.sin(az), r.normal(-2.2, 0.15, points), r.uniform(0, 1, points)], 1)
        xyz[: points // 20, :3] = r.uniform([-2.3, -0.7, -1.45], [-0.1, 0.7, -1.05], (points // 20, 3))          # the ego's own body
        items[f"lidar_{t:05d}".encode()] = f32(xyz)
        sem = r.uniform(0, 1, (points, sem_channels)) * (r.uniform(0, 1, (points, 1)) > 0.5)
        items[f"lidar_sem_{t:05d}".encode()] = f32(sem)
        # BEV maps (ego at pixel (160, 280), 4 px / m): 0 road, 1 vehicles, 2 pedestrians, 9 / 10 lane markings, others empty
        maps = np.zeros((12, 320, 320), np.uint8)
        maps[0][:, 110:210] = 255
        maps[0][230:270, :] = 255
        maps[9][:, 158:162] = 255
        maps[10][248:252, ::8] = 255
        c, s = np.cos(np.deg2rad(ang[0])), np.sin(np.deg2rad(ang[0]))
        for k in np.nonzero(keep)[0]:
            d = pos[k] - pos[0]
            fwd, lat = d[0] * c + d[1] * s, -d[0] * s + d[1] * c
            px, py = 160 + 4 * lat, 280 - 4 * fwd
            hw = 4 * box[k]
            m = (np.abs(xx - px) <= max(hw[1], 1)) & (np.abs(yy - py) <= max(hw[0], 1))
            maps[1 if typ[k] == 1 else 2][m] = 255
        for ch in range(12):
            items[f"map_{ch}_{t:05d}".encode()] = image.imencode_png(maps[ch])
        for stem, png in camera_images(rc, cameras, camera_hw).items():
            items[f"{stem}_{t:05d}".encode()] = png
        if tel:
            for stem, png in tel_images(rt, tel_hw).items():
                items[f"{stem}_{t:05d}".encode()] = png
        pos = pos + speed[:, None] * np.stack([np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))], 1)
    lmdb_ro.write(path, items.items())


def make_dataset(data_dir: str, routes: int = 2, frames: int = 40, seed: int = 0, points: int = 2500, cameras: int = 0,
                 camera_hw=(72, 64), tel: bool = False, tel_hw=(72, 64)) -> None:
    os.makedirs(data_dir, exist_ok=True)
    towns = ["Town01", "Town03", "Town02", "Town06"]
    for i in range(routes):
        make_route(os.path.join(data_dir, f"route_{i:03d}"), seed=seed + i, frames=frames, points=points, town=towns[i % len(towns)],
                   cameras=cameras, camera_hw=camera_hw, tel=tel, tel_hw=tel_hw)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("data_dir")
    ap.add_argument("--routes", type=int, default=2)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--points", type=int, default=2500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cameras", type=int, default=0, help="also write rgb_i / sem_i camera images (train_seg.py's data)")
    ap.add_argument("--camera-hw", type=int, nargs=2, default=(72, 64), metavar=("H", "W"), help="camera image size")
    ap.add_argument("--tel", action="store_true", help="also write the telephoto camera's tel_rgb / tel_sem (train_bra_v2.py's data)")
    ap.add_argument("--tel-hw", type=int, nargs=2, default=(72, 64), metavar=("H", "W"), help="telephoto image size (before crop_tel_bottom)")
    a = ap.parse_args()
    make_dataset(a.data_dir, a.routes, a.frames, a.seed, a.points, a.cameras, tuple(a.camera_hw), a.tel, tuple(a.tel_hw))
    print(f"wrote {a.routes} route(s) of {a.frames} frames under {a.data_dir}")
