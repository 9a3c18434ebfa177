"""Offline point painting of recorded routes (lav/data_paint.py): the stage between `train_seg.py` and `train_full_v2.py`.

The trained ERFNet runs over every indexed frame's camera images, the frame's LiDAR sweep is painted with the class scores
`softmax[1:] * (1 - softmax[0])` of the pixels its points project to (float64 projection, lav/utils/point_painting.py), and
the (n, len(seg_channels)) float32 result is written into the route as `lidar_sem_%05d` - the key `LiDARPaintedDataset` and
`TemporalLiDARPaintedDataset` read.

Differences from the reference, all deliberate: no Ray actors, wandb or matplotlib (none is in this build) - one process owns
the GPU and paints `frames_per_batch` frames per launch sequence, `num_workers` DataLoader processes decode the PNGs; the
images travel to the GPU as uint8 and become float32 there (lav_image_u8_to_f32); a route is committed ONCE, after its last
frame (lmdb_ro.update rewrites the route's file; the reference's per-frame `txn.put` would rewrite it per frame); routes are
visited in sorted order (RouteFrames).  As in the reference the last num_plan frames of a route are not indexed and keep
whatever `lidar_sem_` they had.
"""
from __future__ import annotations

import time

import numpy as np
import torch
import yaml
from torch.utils.data import DataLoader, Dataset

from . import image, lmdb_ro
from .datasets import CameraProjection, RouteFrames, paint_from_cameras, read_array

RGB_H, RGB_W, RGB_FOV = 288, 256, 64          # data_paint.py:59-62


class PointPaintDataset(RouteFrames):
    """The painter's frames (lav/utils/datasets/point_paint_dataset.py): BasicDataset(config_path, close_txn=True)'s index - the
    per-route percentage_data coin, the all_towns filter, frames 0 .. len - num_plan - 1 of each route.  No environment stays
    open between two reads: a route is reopened per sample, so a read after `commit` sees the new file."""

    def __init__(self, config_path):
        super().__init__(config_path, close_txn=True)
        for env in {id(t._env): t._env for t in self.txn_map.values()}.values():
            env.close()
        self.txn_map = {}

    def _read(self, idx):
        env = lmdb_ro.open(self.nam_map[idx], readonly=True, lock=False, readahead=False, meminit=False)
        try:
            txn, index = env.begin(write=False), self.idx_map[idx]
            lidar = read_array(txn, "lidar", index).reshape(-1, 4)
            bgr = np.stack([image.imdecode(np.frombuffer(txn.get(f"rgb_{c}_{index:05d}".encode()), np.uint8), image.IMREAD_COLOR)
                            for c in range(len(self.camera_yaws))])
        finally:
            env.close()
        return lidar, bgr

    def __getitem__(self, idx):
        """(lidar (n, 4) float32, rgbs (ncam, 3, H, W) uint8 in RGB order), point_paint_dataset.py:13-32."""
        lidar, bgr = self._read(idx)
        return lidar, bgr[..., ::-1].transpose((0, 3, 1, 2))

    def raw(self, idx):
        """(lidar (n, 4) float32, images (ncam, H, W, 3) uint8 as decoded: BGR) - for the conversion on the device."""
        return self._read(idx)

    def commit(self, idx, lidar_painted):
        """One frame's scores into its route (point_paint_dataset.py:34-46).  Rewrites the route: paint_dataset commits a whole
        route at once instead."""
        lmdb_ro.update(self.nam_map[idx], [painted_item(self.idx_map[idx], lidar_painted)])


def painted_item(frame: int, lidar_painted):
    return f"lidar_sem_{frame:05d}".encode(), np.ascontiguousarray(lidar_painted).astype(np.float32).tobytes()


def host_paint(lidar, offsets, sem, cameras) -> np.ndarray:
    """The painting stage on the CPU, frame by frame, with the reference's statements (data_paint.py:75-77): what
    lav_paint_frames computes, for tests and comparisons.  lidar (total, 4), offsets (frames + 1,), sem (frames, ncam, 1+C, H, W)."""
    sem = np.asarray(sem)
    out = np.zeros((len(lidar), sem.shape[2] - 1), np.float32)
    for f in range(len(offsets) - 1):
        a, b = int(offsets[f]), int(offsets[f + 1])
        norm = sem[f][:, 1:] * (1 - sem[f][:, :1])
        out[a:b] = paint_from_cameras(lidar[a:b], norm, cameras)
    return out


class PointPainter:
    """data_paint.py's PointPainter for a list of frames.  `probs(images)` maps the frames' (frames * ncam, H, W, 3) uint8 BGR
    images (host array) to (frames * ncam, 1 + C, H, W) class probabilities; `paint(lidar, offsets, sem)` maps the concatenated
    clouds (host, (total, 4)), their int32 offsets and sem (frames, ncam, 1 + C, H, W) (whatever `probs` returned, reshaped) to the
    (total, C) float32 scores on the host.  Left at None they are the GPU stages: one upload of the uint8 images,
    lav_image_u8_to_f32, the ERFNet loaded from seg_model_dir in eval mode - run frame by frame, so that what is written does not
    depend on how many frames share a batch -, one lav_paint_frames launch, one download."""

    def __init__(self, config_path, device="cuda", probs=None, paint=None):
        with open(config_path, "r") as f:
            for key, value in yaml.safe_load(f).items():
                setattr(self, key, value)
        self.cameras = [CameraProjection(yaw, [0, 0, self.camera_z], [self.camera_x, 0, self.camera_z], RGB_H, RGB_W, RGB_FOV)
                        for yaw in self.camera_yaws]
        self.device = torch.device(device)
        self.seg_model = None
        self.seconds = dict(upload_convert=0.0, erfnet=0.0, paint_frames=0.0)
        self.timed = False                     # True: synchronise between the stages and add up their times (the probe)
        if probs is None or paint is None:
            if self.device.type != "cuda":
                raise RuntimeError(f"PointPainter: device {self.device} is refused: the eval-mode ERFNet and the painting kernel run "
                                   "on the GPU only - lav_amd has no CPU path")
            from .. import ops
            self._ops = ops
            self._cams = ops.make_cameras_f64(self.cameras)
        if probs is None:
            from ..rgb import RGBSegmentationModel
            self.seg_model = RGBSegmentationModel(self.seg_channels).to(self.device)
            self.seg_model.load_state_dict(torch.load(self.seg_model_dir, map_location=self.device))
            self.seg_model.eval()
        self._probs = probs if probs is not None else self._gpu_probs
        self._paint = paint if paint is not None else self._gpu_paint

    def _tick(self, name, t0):
        if self.timed:
            torch.cuda.synchronize(self.device)
            self.seconds[name] += time.perf_counter() - t0
        return time.perf_counter()

    def _gpu_probs(self, images):
        t0 = time.perf_counter()
        with torch.no_grad():
            x = self._ops.image_u8_to_f32(torch.from_numpy(images).to(self.device), reverse=True)
            t0 = self._tick("upload_convert", t0)
            # One ERFNet run per frame (its ncam images, the reference's batch): the convolutions' launch plans - and with them
            # the last bits of the maps - depend on the batch, so a run over the whole upload would make the written scores
            # depend on frames_per_batch (tools/data_paint_probe.py is the probe of that difference and of what the per-frame runs cost).
            ncam = len(self.cameras)
            sem = None
            for at in range(0, len(x), ncam):
                s_ = self.seg_model.probs(x[at:at + ncam])
                if sem is None:
                    sem = torch.empty((len(x),) + tuple(s_.shape[1:]), dtype=s_.dtype, device=s_.device)
                sem[at:at + ncam].copy_(s_)
            self._tick("erfnet", t0)
        return sem

    def _gpu_paint(self, lidar, offsets, sem):
        t0 = time.perf_counter()
        out = self._ops.paint_frames(torch.from_numpy(lidar).to(self.device), torch.from_numpy(offsets).to(self.device), sem, self._cams)
        out = out.cpu().numpy()
        self._tick("paint_frames", t0)
        return out

    def paint(self, lidars, images_u8):
        """lidars: per frame (n_f, 4) float32; images_u8: per frame (ncam, H, W, 3) uint8 BGR -> per frame (n_f, C) float32."""
        frames, ncam = len(lidars), len(self.cameras)
        if frames == 0:
            return []
        images = np.ascontiguousarray(np.stack(images_u8).reshape((frames * ncam,) + tuple(images_u8[0].shape[1:])))
        if images.dtype != np.uint8 or images.shape[1:3] != (RGB_H, RGB_W):
            raise ValueError(f"camera images of {images.dtype} {images.shape[1:]}: the painter's cameras are {RGB_H} x {RGB_W} uint8")
        sem = self._probs(images)
        sem = sem.reshape((frames, ncam) + tuple(sem.shape[1:]))
        offsets = np.zeros(frames + 1, np.int32)
        offsets[1:] = np.cumsum([len(l) for l in lidars])
        lidar = np.ascontiguousarray(np.concatenate([np.asarray(l, np.float32).reshape(-1, 4) for l in lidars]))
        painted = self._paint(lidar, offsets, sem)
        return [painted[offsets[f]:offsets[f + 1]] for f in range(frames)]


class _RawFrames(Dataset):
    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        t0 = time.perf_counter()
        lidar, bgr = self.dataset.raw(idx)
        return idx, lidar, bgr, time.perf_counter() - t0


def paint_dataset(config_path, device="cuda", frames_per_batch=16, num_workers=8, num_per_log=100, painter=None, log=print):
    """Paint every indexed frame of config_path's data_dir.  The index is walked in order (a route's frames are contiguous in
    it), PNGs are decoded by `num_workers` DataLoader processes, `frames_per_batch` frames are painted at a time, and a route's
    frames are buffered and committed with ONE lmdb_ro.update when its last frame has been painted.  Host memory therefore grows
    with the length of a route: its painted frames (16 bytes per point, 640 KB per 40 000-point sweep) are held until its
    commit, and once more as lmdb_ro.update's item list during it.  frames_per_batch batches the upload, the conversion, the
    painting launch and the download; the ERFNet runs frame by frame (PointPainter).  Prints frames/s every `num_per_log` frames.  Returns dict(frames, routes, seconds, decode, commit [, the painter's stage times])."""
    dataset = PointPaintDataset(config_path)
    painter = painter if painter is not None else PointPainter(config_path, device)
    loader = DataLoader(_RawFrames(dataset), batch_size=max(int(frames_per_batch), 1), shuffle=False, num_workers=num_workers,
                        collate_fn=list, drop_last=False)
    stats = dict(frames=0, routes=0, seconds=0.0, decode=0.0, commit=0.0)
    pending, route = [], None
    t_start = t_log = time.perf_counter()

    def flush():
        if pending:
            t0 = time.perf_counter()
            lmdb_ro.update(route, pending)
            stats["commit"] += time.perf_counter() - t0
            stats["routes"] += 1
            pending.clear()

    for batch in loader:
        painted = painter.paint([b[1] for b in batch], [b[2] for b in batch])
        for (idx, _, _, dt), scores in zip(batch, painted):
            if dataset.nam_map[idx] != route:
                flush()
                route = dataset.nam_map[idx]
            pending.append(painted_item(dataset.idx_map[idx], scores))
            stats["decode"] += dt
            stats["frames"] += 1
            if num_per_log and stats["frames"] % num_per_log == 0:
                now = time.perf_counter()
                log(f"data_paint: {stats['frames']} / {len(dataset)} frames, {num_per_log / (now - t_log):.1f} frames/s")
                t_log = now
    flush()
    stats["seconds"] = time.perf_counter() - t_start
    stats.update(getattr(painter, "seconds", {}))
    return stats


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Paint the LiDAR sweeps of config-path's recorded routes with the trained segmenter's class "
                                             "scores (lav/data_paint.py): writes lidar_sem_%%05d into every route's LMDB.")
    ap.add_argument("--config-path", default="config.yaml")
    ap.add_argument("--device", default="cuda", help="a GPU: cuda, cuda:1, ... (cpu is refused)")
    ap.add_argument("--num-per-log", type=int, default=100, help="print frames/s every this many frames")
    ap.add_argument("--num-workers", type=int, default=8,
                    help="processes that read and decode the frames' PNGs (NOT Ray actors as in the reference: one process owns the GPU)")
    ap.add_argument("--frames-per-batch", type=int, default=16, help="frames per upload, conversion, painting launch and download (the ERFNet runs one frame's cameras at a time, so "
                         "that the written scores do not depend on this number)")
    args = ap.parse_args(argv)
    if torch.device(args.device).type != "cuda":
        ap.error(f"--device {args.device} is refused: the eval-mode ERFNet and the painting kernel run on the GPU only - lav_amd has no CPU path")
    stats = paint_dataset(args.config_path, args.device, args.frames_per_batch, args.num_workers, args.num_per_log)
    print(f"data_paint: painted {stats['frames']} frames of {stats['routes']} routes in {stats['seconds']:.1f} s "
          f"({stats['frames'] / max(stats['seconds'], 1e-9):.1f} frames/s)")
    return stats
