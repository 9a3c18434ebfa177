"""Tensor-level wrappers over the C ABI (include/lav_amd.h).

torch is used here only as the owner of HBM buffers and of the HIP stream; every
function hands raw device pointers to liblav_amd.so and enqueues on torch's
current stream.  No function here has a torch/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import os as _os
import threading as _threading
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import Camera, Conv, Grid, PointNet, check

_workspaces: dict = {}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor in HBM (cuda/hip device), got {t.device}; lav_amd has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


_retired = []


def _workspace(key, nbytes: int, device) -> torch.Tensor:
    """Scratch buffer per (kind, device, stream): kernels enqueued on different streams may run concurrently
    (the frame graph forks the brake net and the ego branch onto side streams), so they never share scratch."""
    k = (key, device, torch.cuda.current_stream().cuda_stream)
    ws = _workspaces.get(k)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            # a captured HIP graph may have baked the old buffer's address into its kernel nodes: keep it alive (it stays
            # large enough for the launches that were captured with it) instead of returning it to the allocator
            _retired.append(ws)
        # zero-filled: kernels with arrival counters (lav_extract_peaks) expect zeros before their first launch
        ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=device)
        _workspaces[k] = ws
    return ws


def _drop_workspace(key, device):
    ws = _workspaces.pop((key, device, torch.cuda.current_stream().cuda_stream), None)
    if ws is not None:
        _retired.append(ws)   # (captured graphs may still hold its address)


# ------------------------------------------------------------------------------------------ pillar
def make_grid(min_x, max_x, min_y, max_y, ppm) -> Grid:
    nx = int((max_x - min_x) * ppm)
    ny = int((max_y - min_y) * ppm)
    return Grid(float(min_x), float(max_x), float(min_y), float(max_y), float(ppm), nx, ny)


def _pillar_cloud(points: torch.Tensor, num_points: Sequence[int]):
    """cloud(s) (B, Nmax, D) or (N, D) -> (B, Nmax, D) f32 contiguous in HBM, and the host array of row counts the ABI takes"""
    points = _f32c(points[None] if points.dim() == 2 else points, "points")
    if len(num_points) != points.shape[0]:
        raise RuntimeError("num_points must have one entry per cloud")
    return points, (C.c_int * points.shape[0])(*[int(n) for n in num_points])


def _pillar_index_buffers(points: torch.Tensor):
    """unique_coords, inverse and the two counts {pillars, kept rows} of a (B, Nmax, D) cloud, sized for the worst case"""
    total, dev = max(points.shape[0] * points.shape[1], 1), points.device
    return (torch.empty((total, 3), dtype=torch.int32, device=dev), torch.empty((total,), dtype=torch.int32, device=dev),
            torch.zeros((2,), dtype=torch.int32, device=dev))


def pillar_scatter(points: torch.Tensor, num_points: Sequence[int], grid: Grid, w1, b1, w2, b2,
                   want_indices: bool = False, amax: Optional["Amax"] = None):
    """points (B, Nmax, D) or (N, D) f32 in HBM -> canvas (B, C, ny, nx)
    [+ unique_coords (P,3) int32, inverse (N_kept,) int32 when want_indices].
    amax: an Amax that receives the canvas kernel's per-workgroup maxima (lav_pillar_scatter_amax) and is attached to the canvas
    (amax_of): the first BEV convolution then takes its fp16 scale from them instead of measuring the canvas with a launch."""
    lib = _lib.load()
    points, h_num = _pillar_cloud(points, num_points)
    B, nmax, D = points.shape
    Cc = w2.shape[1]
    net = PointNet(_ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), D + 5, Cc)
    dev = points.device
    canvas = torch.empty((B, Cc, grid.ny, grid.nx), dtype=torch.float32, device=dev)
    nbytes = lib.lav_pillar_workspace_bytes(B, nmax, C.byref(grid))
    # zero-filled once and kept per geometry: the head of a pillar workspace is state that every call leaves clean
    # (include/lav_amd.h, workspace contract)
    ws = _workspace(("pillar", B, grid.nx, grid.ny), nbytes, dev)
    uc, inv, cnt = _pillar_index_buffers(points) if want_indices else (None, None, None)
    parts = amax.reset().take(lib.lav_pillar_amax_count(B, C.byref(grid))) if amax is not None else None
    rc = lib.lav_pillar_scatter_amax(_ptr(points) if nmax > 0 else None, h_num, B, nmax, D, C.byref(grid), C.byref(net),
                                     _ptr(canvas), _ptr(uc), _ptr(inv), _ptr(cnt), _ptr(parts), _ptr(ws), ws.numel(), _stream())
    if amax is not None:
        tag_amax(canvas, amax)
    if rc != 0:
        # the workspace's zero-at-rest state (arrival counters, epoch words) may be half-updated: never reuse it (lav_amd.h, workspace
        # contract) - the next call zero-fills a fresh one
        _drop_workspace(("pillar", B, grid.nx, grid.ny), dev)
    check(rc, "lav_pillar_scatter")
    if want_indices:
        p, k = cnt.tolist()   # {pillars, kept rows}: the call's one device->host copy
        return canvas, uc[:p], inv[:k]
    return canvas


def pillar_decorate(points: torch.Tensor, num_points: Sequence[int], grid: Grid):
    """Training-side front end of PointPillarNet: points (B, Nmax, D) -> decorated (N_kept, D+5), unique_coords (P,3),
    inverse (N_kept,), kept_src (N_kept,) (int32, all in HBM).  One device->host copy (the two counts)."""
    lib = _lib.load()
    points, h_num = _pillar_cloud(points.detach(), num_points)
    B, nmax, D = points.shape
    uc, inv, cnt = _pillar_index_buffers(points)
    src = torch.empty_like(inv)
    dec = torch.empty((inv.shape[0], D + 5), dtype=torch.float32, device=points.device)
    nbytes = lib.lav_pillar_decorate_workspace_bytes(B, nmax, C.byref(grid))
    ws = _workspace("pillar_decorate", nbytes, points.device)
    check(lib.lav_pillar_decorate(_ptr(points) if nmax > 0 else None, h_num, B, nmax, D, C.byref(grid), _ptr(uc), _ptr(inv),
                                  _ptr(src), _ptr(dec), _ptr(cnt), _ptr(ws), ws.numel(), _stream()), "lav_pillar_decorate")
    p, k = cnt.tolist()
    return dec[:k], uc[:p], inv[:k], src[:k]


class _ScatterMax(torch.autograd.Function):
    """torch_scatter.scatter_max(src, index, dim=0) on liblav_amd, differentiable in src."""

    @staticmethod
    def forward(ctx, src, index, num_segments):
        lib = _lib.load()
        src = _f32c(src, "src")
        if index.dtype != torch.int32 or not index.is_cuda:
            raise RuntimeError("scatter_max: index must be an int32 tensor in HBM")
        n, ch = src.shape
        out = torch.empty((num_segments, ch), dtype=torch.float32, device=src.device)
        arg = torch.empty((num_segments, ch), dtype=torch.int32, device=src.device)
        check(lib.lav_scatter_max(_ptr(src), _ptr(index.contiguous()), n, ch, num_segments, _ptr(out), _ptr(arg), _stream()),
              "lav_scatter_max")
        ctx.save_for_backward(arg)
        ctx.n = n
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        (arg,) = ctx.saved_tensors
        lib = _lib.load()
        grad_out = _f32c(grad_out, "grad_out")
        num_segments, ch = grad_out.shape
        grad_src = torch.empty((ctx.n, ch), dtype=torch.float32, device=grad_out.device)
        check(lib.lav_scatter_max_backward(_ptr(grad_out), _ptr(arg), ctx.n, ch, num_segments, _ptr(grad_src), _stream()),
              "lav_scatter_max_backward")
        return grad_src, None, None


def scatter_max(src: torch.Tensor, index: torch.Tensor, num_segments: int):
    """(out (S, C), argmax (S, C) int32) - torch_scatter.scatter_max(src, index, dim=0) semantics."""
    return _ScatterMax.apply(src, index, int(num_segments))


# ------------------------------------------------------------------------------------------ paint
def make_cameras(mats) -> C.Array:
    """mats: sequence of (K 3x3, lidar_to_world 4x4, world_to_cam 4x4) float32 arrays."""
    arr = (Camera * len(mats))()
    for cam, (K, l2w, w2c) in zip(arr, mats):
        cam.K[:] = [float(v) for v in np.asarray(K, np.float32).reshape(-1)]
        cam.l2w[:] = [float(v) for v in np.asarray(l2w, np.float32).reshape(-1)]
        cam.w2c[:] = [float(v) for v in np.asarray(w2c, np.float32).reshape(-1)]
    return arr


def paint(lidar: torch.Tensor, sem: torch.Tensor, cams, want_uvz: bool = False):
    """lidar (N, Dl) f32, sem (ncam, 1+Cs, H, W) softmax maps -> fused (N, Dl+Cs) [+ uvz (ncam, N, 3) int32]."""
    lib = _lib.load()
    lidar = _f32c(lidar, "lidar")
    sem = _f32c(sem, "sem")
    n, dl = lidar.shape
    ncam, cs1, h, w = sem.shape
    fused = torch.empty((n, dl + cs1 - 1), dtype=torch.float32, device=lidar.device)
    uvz = torch.empty((ncam, n, 3), dtype=torch.int32, device=lidar.device) if want_uvz else None
    check(lib.lav_paint(_ptr(lidar), n, dl, _ptr(sem), ncam, cs1 - 1, h, w, cams, _ptr(fused), _ptr(uvz), _stream()),
          "lav_paint")
    return (fused, uvz) if want_uvz else fused


def make_cameras_f64(mats) -> C.Array:
    """mats: sequence of (K 3x3, lidar_to_world 4x4, world_to_cam 4x4) float64 arrays, or of objects with those three as
    attributes K, lidar_to_world, world_to_cam (lav_amd.data.datasets.CameraProjection) -> lav_camera_f64 records."""
    arr = (_lib.CameraF64 * len(mats))()
    for cam, m in zip(arr, mats):
        K, l2w, w2c = (m.K, m.lidar_to_world, m.world_to_cam) if hasattr(m, "world_to_cam") else m
        cam.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
        cam.l2w[:] = [float(v) for v in np.asarray(l2w, np.float64).reshape(16)]
        cam.w2c[:] = [float(v) for v in np.asarray(w2c, np.float64).reshape(16)]
    return arr


def paint_frames(lidar: torch.Tensor, offsets: torch.Tensor, sem: torch.Tensor, cams, want_uvz: bool = False):
    """The offline painter for a batch of frames in one launch (lav_paint_frames).  lidar (total, Dl) f32: the frames' clouds one
    after the other; offsets (frames + 1,) int32 in HBM, offsets[0] = 0, offsets[-1] = total; sem (frames, ncam, 1+Cs, H, W) class
    probabilities; cams: make_cameras_f64(...) of ncam cameras -> painted (total, Cs) [+ uvz (ncam, total, 3) int32]."""
    lib = _lib.load()
    lidar = _f32c(lidar, "lidar")
    sem = _f32c(sem, "sem")
    if not (offsets.is_cuda and offsets.dtype == torch.int32 and offsets.dim() == 1):
        raise RuntimeError(f"offsets: expected a 1-d int32 tensor in HBM, got {offsets.dtype} {tuple(offsets.shape)} on {offsets.device}")
    offsets = offsets.contiguous()
    total, dl = lidar.shape
    frames, ncam, cs1, h, w = sem.shape
    if offsets.numel() != frames + 1:
        raise RuntimeError(f"offsets: {offsets.numel()} entries for {frames} frames (frames + 1 expected)")
    if not 1 <= ncam <= _lib.MAX_CAM_F64:
        raise RuntimeError(f"paint_frames: ncam {ncam} outside [1,{_lib.MAX_CAM_F64}]")
    if len(cams) != ncam:
        raise RuntimeError(f"{len(cams)} camera records for {ncam} cameras' maps")
    painted = torch.empty((total, cs1 - 1), dtype=torch.float32, device=lidar.device)
    uvz = torch.empty((ncam, total, 3), dtype=torch.int32, device=lidar.device) if want_uvz else None
    check(lib.lav_paint_frames(_ptr(lidar), _ptr(offsets), frames, total, dl, _ptr(sem), ncam, cs1 - 1, h, w, cams, _ptr(painted),
                               _ptr(uvz), _stream()), "lav_paint_frames")
    return (painted, uvz) if want_uvz else painted


def image_u8_to_f32(img: torch.Tensor, reverse: bool = False) -> torch.Tensor:
    """img (n, H, W, 3 or 4) uint8 in HBM -> (n, 3, H, W) float32 of its first three channels, reversed with `reverse`
    (BGR / BGRA -> RGB).  Exact."""
    lib = _lib.load()
    if not img.is_cuda:
        raise RuntimeError(f"img: expected a tensor in HBM (cuda/hip device), got {img.device}; lav_amd has no CPU path")
    if img.dtype != torch.uint8 or img.dim() != 4:
        raise RuntimeError(f"img: expected (n, H, W, C) uint8, got {img.dtype} {tuple(img.shape)}")
    img = img.contiguous()
    n, h, w, c = img.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=img.device)
    check(lib.lav_image_u8_to_f32(_ptr(img), n, h, w, c, int(bool(reverse)), _ptr(out), _stream()), "lav_image_u8_to_f32")
    return out


def augment_u8(images: torch.Tensor, params: np.ndarray, seed: int) -> torch.Tensor:
    """The camera trainers' image augmentation in one launch (lav_augment_u8): images (n, H, W, 3) uint8 in HBM, params n records
    of lav_amd.data.augment.PARAMS_DTYPE (host; uploaded here, 128 bytes per image), seed the 64-bit Philox key -> the augmented
    (n, H, W, 3) uint8 images in a new tensor.  Bit-identical to lav_amd.data.augment.augment_numpy except for noise's rounding ties."""
    from .data.augment import check_params
    lib = _lib.load()
    if not images.is_cuda:
        raise RuntimeError(f"images: expected a tensor in HBM (cuda/hip device), got {images.device}; lav_amd.ops has no CPU path "
                           "(lav_amd.data.augment.Augmenter runs augment_numpy on CPU tensors)")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError(f"images: expected (n, H, W, 3) uint8, got {images.dtype} {tuple(images.shape)}")
    images = images.contiguous()
    n, h, w, _ = images.shape
    params = check_params(params, n)
    out = torch.empty_like(images)
    if n == 0 or h == 0 or w == 0:
        return out
    table = torch.from_numpy(params.view(np.uint8).reshape(n, -1)).to(images.device)
    check(lib.lav_augment_u8(_ptr(images), _ptr(out), n, h, w, _ptr(table), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "lav_augment_u8")
    return out


def bev_stack_u8(planes: torch.Tensor, coef, shift, threshold: bool = True) -> torch.Tensor:
    """The loaders' BEV stacks in one launch (lav_bev_stack_u8): planes (..., P, H, W) uint8 in HBM, coef (..., P, 12) float64 and shift
    (..., P, 2) int32 (arrays or tensors, host or device; uploaded here) -> W2(crop(W1(planes))) > 0 per plane, or the interpolated
    values with threshold=False, in a new uint8 tensor.  Bit-identical to lav_amd.data.bev_stack.bev_stack_numpy."""
    from .data.bev_stack import check_record
    lib = _lib.load()
    if not planes.is_cuda:
        raise RuntimeError(f"planes: expected a tensor in HBM (cuda/hip device), got {planes.device}; lav_amd.ops has no CPU path "
                           "(lav_amd.data.bev_stack.BevStacker runs bev_stack_numpy on CPU tensors)")
    if planes.dtype != torch.uint8 or planes.dim() < 3:
        raise RuntimeError(f"planes: expected (..., P, H, W) uint8, got {planes.dtype} {tuple(planes.shape)}")
    planes = planes.contiguous()
    coef, shift = check_record(planes.shape, coef, shift)
    out = torch.empty_like(planes)
    h, w = planes.shape[-2:]
    n = len(coef)
    if n == 0 or h == 0 or w == 0:
        return out
    coef_d, shift_d = torch.from_numpy(coef).to(planes.device), torch.from_numpy(shift).to(planes.device)
    check(lib.lav_bev_stack_u8(_ptr(planes), _ptr(coef_d), _ptr(shift_d), _ptr(out), n, h, w, int(bool(threshold)), _stream()), "lav_bev_stack_u8")
    return out


def bev_stack_tile_paths(coef, shift, h: int, w: int):
    """(zero, staged, direct): how many of a plane's 64 x 32 tiles lav_bev_stack_u8 leaves zero, renders from LDS and renders from
    global memory - the kernel's own rule, evaluated on the host (lav_bev_stack_tile_paths).  coef (12,), shift (2,)."""
    import ctypes
    coef = np.ascontiguousarray(np.asarray(coef, np.float64).reshape(12))
    shift = np.ascontiguousarray(np.asarray(shift, np.int32).reshape(2))
    counts = (ctypes.c_int * 3)()
    check(_lib.load().lav_bev_stack_tile_paths(coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), shift.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               int(h), int(w), counts), "lav_bev_stack_tile_paths")
    return tuple(counts)


_view_constants: dict = {}


def debug_view(rgb: torch.Tensor, tel_rgb: torch.Tensor, lidar: torch.Tensor, pred_bev: torch.Tensor, prims, text, *, grid,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The agent's debug frame on the device (lav_debug_view; zeroing, histogram and compose launches on the current stream): rgb
    (h, w, 3) and tel_rgb (h', w', 3) uint8 RGB, lidar (n, >= 2) float32, pred_bev (3, x bins, width) float32 already sigmoided, all
    in HBM; prims the records of lav_amd.agent.debug_view.primitives and text those of text_rows (host arrays, uploaded here);
    grid = (min_x, max_x, min_y, max_y, pixels_per_meter).  Returns the (H / 2, W / 2, 3) uint8 frame (`out` when given).
    Bit-identical to lav_amd.agent.debug_view.compose_numpy.  Wrong shapes or dtypes raise ValueError before anything is launched."""
    from .agent import debug_view as V
    for name, t, dtype, dim in (("rgb", rgb, torch.uint8, 3), ("tel_rgb", tel_rgb, torch.uint8, 3), ("lidar", lidar, torch.float32, 2),
                                ("pred_bev", pred_bev, torch.float32, 3)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"debug_view: {name} must be a tensor in HBM (cuda/hip device); lav_amd.ops has no CPU path "
                             "(lav_amd.agent.debug_view.compose_numpy is the CPU specification)")
        if t.dtype != dtype or t.dim() != dim:
            raise ValueError(f"debug_view: {name} must be {dim}-d {dtype}, got {t.dtype} {tuple(t.shape)}")
    if lidar.shape[1] < 2:
        raise ValueError(f"debug_view: lidar {tuple(lidar.shape)} has no x and y columns")
    lay = V.layout(rgb.shape, tel_rgb.shape, grid, pred_bev.shape)
    (x0, x1, nxb), (y0, y1, nyb) = V.grid_bins(grid)
    prims, text = V.check_primitives(prims), V.check_text(text)
    shape = (lay["frame_h"], lay["frame_w"], 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=rgb.device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"debug_view: out must be a contiguous uint8 tensor of shape {shape} in HBM")
    lib = _lib.load()
    dev = rgb.device
    rgb, tel_rgb, lidar, pred_bev = rgb.contiguous(), tel_rgb.contiguous(), lidar.contiguous(), pred_bev.contiguous()
    key = (dev, tuple(rgb.shape), tuple(tel_rgb.shape), tuple(grid), lay["w_bev"])
    const = _view_constants.get(key)
    if const is None:      # per geometry, once: font, grey table and the six resize tables
        if len(_view_constants) > 16:
            _view_constants.clear()
        const = _view_constants[key] = (torch.from_numpy(V.FONT.copy()).to(dev), torch.from_numpy(V.HIST_LUT.copy()).to(dev),
                                        torch.from_numpy(V.resize_tables(rgb.shape, tel_rgb.shape, lay)).to(dev))
    font, lut, tables = const
    # text and records in one upload: [4 x TEXT_LEN bytes][records]
    host = np.concatenate([text.reshape(-1), prims.view(np.uint8).reshape(-1)])
    up = torch.from_numpy(host).to(dev)
    counts = _workspace(("debug_view", nxb, nyb), nxb * nyb * 4, dev)
    check(lib.lav_debug_view(_ptr(rgb), rgb.shape[0], rgb.shape[1], _ptr(tel_rgb), tel_rgb.shape[0], tel_rgb.shape[1], _ptr(lidar),
                             lidar.shape[0], lidar.shape[1], _ptr(pred_bev), lay["w_bev"], up.data_ptr() + text.size, len(prims), up.data_ptr(),
                             text.shape[1], _ptr(font), _ptr(lut), _ptr(tables), x0, x1, nxb, y0, y1, nyb, lay["w_rgb"], lay["w_tel"],
                             _ptr(counts), _ptr(out), _stream()), "lav_debug_view")
    return out


_jpeg_tables: dict = {}


def jpeg_encode(frames: torch.Tensor, quality: int = 90, restart_mcus: Optional[int] = None, out: Optional[torch.Tensor] = None,
                lengths: Optional[torch.Tensor] = None):
    """Baseline JPEG scans of RGB frames on the device (lav_jpeg_encode; three launches on the current stream for the whole batch, no
    synchronisation): frames (n, h, w, 3) or (h, w, 3) uint8 in HBM, quality 1 .. 100, restart_mcus 1 .. 10 MCUs per restart interval
    (default lav_amd.agent.mjpeg.DEFAULT_RESTART_MCUS).  Returns (scans (n, capacity) uint8, lengths (n,) int32) in HBM - `out` and
    `lengths` when given; out may have more columns than capacity = lav_amd.agent.mjpeg.scan_capacity(h, w, restart_mcus).
    scans[i, :lengths[i]] is what stands between jpeg_header(h, w, quality, restart_mcus) and EOI; the bytes behind it are not
    written.  Byte-identical to lav_amd.agent.mjpeg.scan_numpy.  The workspace and the device tables are kept per (n, h, w, quality,
    restart_mcus, stream).  Wrong device, dtype, shape, quality, interval or a short `out` raise ValueError before anything is launched."""
    from .agent import mjpeg as J
    if restart_mcus is None:
        restart_mcus = J.DEFAULT_RESTART_MCUS
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise ValueError("jpeg_encode: frames must be a tensor in HBM (cuda/hip device); lav_amd.ops has no CPU path "
                         "(lav_amd.agent.mjpeg.jpeg_encode_numpy is the CPU specification)")
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError(f"jpeg_encode: frames must be (n, h, w, 3) or (h, w, 3) uint8, got {frames.dtype} {tuple(frames.shape)}")
    if isinstance(quality, bool) or isinstance(restart_mcus, bool):
        raise ValueError("jpeg_encode: quality and restart_mcus are integers")
    J._check(quality, restart_mcus)
    batch = frames if frames.dim() == 4 else frames[None]
    n, h, w = (int(v) for v in batch.shape[:3])
    if n < 1 or n > 4096:
        raise ValueError(f"jpeg_encode: {n} frames (1 .. 4096)")
    capacity = J.scan_capacity(h, w, restart_mcus)           # (refuses sides outside 1 .. 16384)
    if capacity > 0x7FFFFFFF:
        raise ValueError(f"jpeg_encode: a scan of up to {capacity} bytes has no int32 length")
    dev = frames.device
    if out is None:
        out = torch.empty((n, capacity), dtype=torch.uint8, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == n
              and out.shape[1] >= capacity and out.stride(1) == 1 and out.stride(0) >= capacity):
        raise ValueError(f"jpeg_encode: out must be uint8 ({n}, >= {capacity}) with contiguous rows in HBM, on the frames' device")
    if lengths is None:
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    elif not (isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.device == dev and lengths.dtype == torch.int32 and tuple(lengths.shape) == (n,)
              and lengths.is_contiguous()):
        raise ValueError(f"jpeg_encode: lengths must be a contiguous int32 tensor of shape ({n},) in HBM, on the frames' device")
    lib = _lib.load()
    batch = batch.contiguous()
    key = (dev, int(quality))
    tables = _jpeg_tables.get(key)
    if tables is None:
        if len(_jpeg_tables) > 16:
            _jpeg_tables.clear()
        tables = _jpeg_tables[key] = torch.from_numpy(J.device_tables(int(quality))).to(dev)
    nbytes = int(lib.lav_jpeg_workspace_bytes(n, h, w, int(restart_mcus)))
    ws = _workspace(("jpeg_encode", n, h, w, int(quality), int(restart_mcus)), nbytes, dev)
    check(lib.lav_jpeg_encode(_ptr(batch), n, h, w, 3 * w, _ptr(tables), int(restart_mcus), _ptr(out), int(out.stride(0)), _ptr(lengths), _ptr(ws), nbytes,
                              _stream()), "lav_jpeg_encode")
    return out, lengths


_log_view_font: dict = {}


def log_view(panels, prims, text, sources, *, size=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A trainer's log frame on the device (lav_log_view; zeroing, minimum / maximum and compose launches on the current stream):
    panels, prims and text the host tables of lav_amd.train.log_view (uploaded here in one copy), sources the tensors in HBM the
    panels name; size = (height, width) of the frame, by default the extent of the panels.  Returns the (height, width, 3) uint8 frame
    (`out` when given).  Bit-identical to lav_amd.train.log_view.log_view_numpy.  Wrong tables, shapes or dtypes raise ValueError
    before anything is launched."""
    from .train import log_view as V
    sources = list(sources)
    for i, t in enumerate(sources):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"log_view: source {i} must be a tensor in HBM (cuda/hip device); lav_amd.ops has no CPU path "
                             "(lav_amd.train.log_view.log_view_numpy is the CPU specification)")
    panels = V.check_panels(panels, sources)
    prims, text = V.check_prims(prims, len(panels)), V.check_text(text)
    shape = V.frame_size(panels, size) + (3,)
    dev = sources[0].device if sources else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"log_view: out must be a contiguous uint8 tensor of shape {shape} in HBM")
    lib = _lib.load()
    sources = [t.contiguous() for t in sources]           # (kept alive until the launches are enqueued; the stream orders their reuse)
    dpanels, palette = V.device_tables(panels, sources, [t.data_ptr() for t in sources])
    font = _log_view_font.get(dev)
    if font is None:
        font = _log_view_font[dev] = torch.from_numpy(V.FONT.copy()).to(dev)
    # one upload: [panels][primitives][origins][characters][palette], the first three 4-byte aligned by their sizes
    parts = [dpanels.view(np.uint8).reshape(-1), prims.view(np.uint8).reshape(-1), np.ascontiguousarray(text["origin"]).view(np.uint8).reshape(-1),
             np.ascontiguousarray(text["chars"]).reshape(-1), palette.reshape(-1)]
    offs = np.cumsum([0] + [p.size for p in parts])
    up = torch.from_numpy(np.concatenate(parts + [np.zeros(16, np.uint8)])).to(dev)
    at = lambda k: up.data_ptr() + int(offs[k])
    mm = _workspace("log_view", 128, dev)
    check(lib.lav_log_view(at(0), len(panels), at(1), len(prims), at(3), at(2), len(text), V.TEXT_LEN, _ptr(font), at(4), len(palette),
                           _ptr(mm), shape[0], shape[1], _ptr(out), _stream()), "lav_log_view")
    return out


def eval_acc_words(nbins: int = 256) -> int:
    """Length of lav_eval_frame's accumulator (lav_eval_acc_words; host only, no device needed)."""
    n = int(_lib.load().lav_eval_acc_words(int(nbins)))
    if n == 0:
        raise ValueError(f"eval_frame: {nbins} score bins (1 .. 1024)")
    return n


def eval_frame(acc: torch.Tensor, pred_bev: torch.Tensor, bev: torch.Tensor, mask: torch.Tensor, rows: torch.Tensor, locs: torch.Tensor,
               typs: torch.Tensor, n: int, ego_plan: torch.Tensor, ego_locs: torch.Tensor, cmd: int, other_cast, other_cmds, other_row, *,
               ppm: float, centre, radius_px: float, threshold: float = 0.5, min_score: float = 0.1, det_score: float = 0.2,
               nbins: int = 256) -> torch.Tensor:
    """The open-loop metrics of one frame, ADDED into `acc` (int64, ops.eval_acc_words(nbins) words, in HBM) by one launch on the current
    stream (lav_eval_frame); nothing comes back to the host.  pred_bev (3, H, W) float32 probabilities; bev (>= 3, H, W) uint8, the
    loaders' stack, of which the first three planes are the labels; mask (H, W) uint8; rows (2, D <= 32, 7) float32 of extract_peaks;
    locs (G <= 64, T + 1, 2) float32, typs (G,) int32 and n: the ground truth as the loaders return it; ego_plan (T, 2), ego_locs
    (T + 1, 2), cmd; other_cast (N, 6, T, 2), other_cmds (N, 6), other_row (N,) int32 - with N = 0 they may be None or empty tensors on
    any device (UniPlanner.infer_all returns CPU zeros then).  centre = the ego pixel (x, y).  Bit-identical to
    lav_amd.train.evaluate.eval_frame_numpy, which names the accumulator's slices (ACC).  Wrong shapes, dtypes or devices raise
    ValueError before anything is launched."""
    _eval_section("eval_frame", acc, eval_acc_words(nbins), "acc")
    need = _eval_tensor("eval_frame", "evaluate.eval_frame_numpy", acc, copy=True)
    pred_bev = need("pred_bev", pred_bev, torch.float32, (3, None, None))
    H, W = pred_bev.shape[1:]
    bev = need("bev", bev, torch.uint8, (None, H, W))
    if bev.shape[0] < 3:
        raise ValueError(f"eval_frame: bev {tuple(bev.shape)} has fewer than three label planes")
    mask = need("mask", mask, torch.uint8, (H, W))
    rows = need("rows", rows, torch.float32, (2, None, 7))
    D = rows.shape[1]
    if not 1 <= D <= 32:
        raise ValueError(f"eval_frame: {D} rows per class (1 .. 32)")
    locs = need("locs", locs, torch.float32, (None, None, 2))
    G, T = locs.shape[0], locs.shape[1] - 1
    if G > 64 or not 1 <= T <= 64:
        raise ValueError(f"eval_frame: locs {tuple(locs.shape)}: at most 64 actors, 1 .. 64 waypoints")
    typs = need("typs", typs, torch.int32, (G,))
    n, cmd = int(n), int(cmd)
    if not 0 <= n <= G:
        raise ValueError(f"eval_frame: n = {n} of {G} actors")
    if not 0 <= cmd < 6:
        raise ValueError(f"eval_frame: command {cmd} (0 .. 5)")
    ego_plan = need("ego_plan", ego_plan, torch.float32, (T, 2))
    ego_locs = need("ego_locs", ego_locs, torch.float32, (T + 1, 2))
    count = lambda t: 0 if t is None else (t.shape[0] if t.dim() else 1)
    N = count(other_cast)
    if count(other_row) != N or count(other_cmds) != N:
        raise ValueError(f"eval_frame: {count(other_row)} rows and {count(other_cmds)} command scores for {N} forecasts")
    if N > 0:
        other_cast = need("other_cast", other_cast, torch.float32, (N, 6, T, 2))
        other_cmds = need("other_cmds", other_cmds, torch.float32, (N, 6))
        other_row = need("other_row", other_row, torch.int32, (N,))
        if N > D or G == 0:
            raise ValueError(f"eval_frame: {N} forecasts from {D} rows and {G} actors")
    else:
        other_cast = other_cmds = other_row = None
    scalars = [float(ppm), float(centre[0]), float(centre[1]), float(radius_px), float(min_score), float(det_score)]
    if not all(np.isfinite(scalars)) or not np.isfinite(float(threshold)) or scalars[0] <= 0 or scalars[3] < 0:
        raise ValueError("eval_frame: scalars must be finite, pixels per metre positive, the radius not negative")
    check(_lib.load().lav_eval_frame(_ptr(pred_bev), _ptr(bev), _ptr(mask), H, W, float(threshold), _ptr(rows), D, _ptr(locs), _ptr(typs), G, n, T,
                                     _ptr(ego_plan), _ptr(ego_locs), cmd, _ptr(other_cast), _ptr(other_cmds), _ptr(other_row), N, *scalars,
                                     int(nbins), _ptr(acc), _stream()), "lav_eval_frame")
    return acc


EVAL_SEG_WORDS = 68            # lav_eval_seg's section: images, pixels, ignored, nonfinite, conf [8][8]


def _eval_tensor(op, spec, like, copy=False):
    """The evaluation kernels' check of one argument, need(name, t, dtype, shape) -> t: in HBM, on the device of the accumulator `like`, of
    the dtype and shape (None: any size), and contiguous - or, with `copy`, made so.  `spec` names the CPU specification under
    lav_amd.train.  The checks are most of what a launch costs with its wrapper (tools/eval_probe.py), hence a closure per call rather
    than eight arguments per tensor, the device read once, and a loop over the sizes rather than any() of a generator."""
    device = like.device

    def need(name, t, dtype, shape):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{op}: {name} must be a tensor in HBM (cuda/hip device); lav_amd.ops has no CPU path "
                             f"(lav_amd.train.{spec} is the CPU specification)")
        if t.device != device:
            raise ValueError(f"{op}: {name} is on {t.device}, the accumulator on {device}")
        got = t.shape
        ok = t.dtype == dtype and len(got) == len(shape)
        if ok:
            for want, size in zip(shape, got):
                if want is not None and want != size:
                    ok = False
                    break
        if not ok:
            raise ValueError(f"{op}: {name} must be {dtype} of shape {tuple('*' if s is None else s for s in shape)}, got {t.dtype} {tuple(got)}")
        if copy:
            return t.contiguous()
        if not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be contiguous (the kernel reads it where it is)")
        return t
    return need


def _eval_section(op, acc_section, words, name="the section"):
    if (not isinstance(acc_section, torch.Tensor) or not acc_section.is_cuda or acc_section.dtype != torch.int64
            or tuple(acc_section.shape) != (words,) or not acc_section.is_contiguous()):
        raise ValueError(f"{op}: {name} must be a contiguous int64 tensor (or slice of one) of {words} words in HBM")


def eval_seg(acc_section: torch.Tensor, logits: torch.Tensor, labels: torch.Tensor, scale: int = 1) -> torch.Tensor:
    """The confusion matrix of labels (n, h * scale, w * scale) uint8 against logits (n, k, h, w) float32, 2 <= k <= 8, scale in
    {1, 2, 4, 8}, ADDED into `acc_section` (int64, 68 words, in HBM) by one launch on the current stream (lav_eval_seg); nothing comes
    back to the host.  Label pixel (y, x) is judged by logit pixel (y // scale, x // scale): F.interpolate(logits, scale_factor=scale)
    followed by argmax (the first maximum), without the up-sampled logits.  Word for word lav_amd.train.evaluate_camera.eval_seg_numpy,
    which has the definitions.  Wrong shapes, dtypes or devices raise ValueError before anything is launched."""
    _eval_section("eval_seg", acc_section, EVAL_SEG_WORDS)
    need = _eval_tensor("eval_seg", "evaluate_camera.eval_seg_numpy", acc_section)
    logits = need("logits", logits, torch.float32, (None, None, None, None))
    n, k, h, w = logits.shape
    scale = int(scale)
    if scale not in (1, 2, 4, 8):
        raise ValueError(f"eval_seg: scale {scale} (1, 2, 4 or 8)")
    if not 2 <= k <= 8:
        raise ValueError(f"eval_seg: {k} classes (2 .. 8)")
    if n < 1 or h < 1 or w < 1 or h > 16384 or w > 16384 or n * h * w * scale * scale > 1 << 31:
        raise ValueError(f"eval_seg: logits {tuple(logits.shape)} at scale {scale}: at least one pixel, sides up to 16384, at most 2^31 label pixels")
    labels = need("labels", labels, torch.uint8, (n, h * scale, w * scale))
    check(_lib.load().lav_eval_seg(_ptr(logits), _ptr(labels), n, k, h, w, scale, _ptr(acc_section), _stream()), "lav_eval_seg")
    return acc_section


def eval_scores(acc_section: torch.Tensor, scores: torch.Tensor, flags: torch.Tensor, threshold: float, nbins: int) -> torch.Tensor:
    """scores (n,) float32 against flags (n,) uint8, ADDED into `acc_section` (int64, 6 + 2 nbins words, in HBM) by one launch on the
    current stream (lav_eval_scores): samples, nonfinite, at [flag != 0][float64(score) > threshold], hist [flag != 0][bin].  Word for
    word lav_amd.train.evaluate_camera.eval_scores_numpy.  Wrong shapes, dtypes or devices raise ValueError before anything is launched."""
    nbins = int(nbins)
    if not 1 <= nbins <= 1024:
        raise ValueError(f"eval_scores: {nbins} score bins (1 .. 1024)")
    _eval_section("eval_scores", acc_section, 6 + 2 * nbins)
    need = _eval_tensor("eval_scores", "evaluate_camera.eval_scores_numpy", acc_section)
    scores = need("scores", scores, torch.float32, (None,))
    n = scores.shape[0]
    if n < 1:
        raise ValueError("eval_scores: no scores")
    flags = need("flags", flags, torch.uint8, (n,))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("eval_scores: the threshold must be a number")
    check(_lib.load().lav_eval_scores(_ptr(scores), _ptr(flags), n, threshold, nbins, _ptr(acc_section), _stream()), "lav_eval_scores")
    return acc_section


def eval_plans_words(iters: int) -> int:
    """Length of lav_eval_plans' accumulator for `iters` plan iterations, 57 + 37 (iters + 1) (lav_eval_plans_words; host only, no
    device needed)."""
    n = int(_lib.load().lav_eval_plans_words(int(iters)))
    if n == 0:
        raise ValueError(f"eval_plans: {iters} plan iterations (1 .. 8)")
    return n


def eval_plans(acc: torch.Tensor, ego_plan: torch.Tensor, ego_cast: torch.Tensor, ego_cmds: torch.Tensor, ego_locs: torch.Tensor,
               cmds: torch.Tensor, bras: torch.Tensor, other_cast=None, other_cmds=None, other_locs=None) -> torch.Tensor:
    """The teacher's metrics over one loader batch, ADDED into `acc` (int64, ops.eval_plans_words(I) words, in HBM) by one launch on the
    current stream (lav_eval_plans); nothing comes back to the host.  ego_plan (B, I, 6, T, 2), ego_cast (B, 6, T, 2), ego_cmds (B, 6),
    ego_locs (B, T + 1, 2) float32; cmds (B,) int32; bras (B,) uint8; other_cast (K, 6, T, 2), other_cmds (K, 6), other_locs (K, T, 2)
    float32 - with K = 0 they may be None or empty tensors.  B >= 1, 1 <= T <= 64, 1 <= I <= 8.  Word for word
    lav_amd.train.evaluate_bev.eval_plans_numpy, which names the accumulator's slices (PlanLayout).  Wrong shapes, dtypes, devices or
    an accumulator of another length raise ValueError before anything is launched."""
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.dtype != torch.int64 or acc.dim() != 1 or not acc.is_contiguous():
        raise ValueError("eval_plans: acc must be a contiguous int64 tensor in HBM (lav_amd.train.evaluate_bev.eval_plans_numpy is the CPU specification)")
    need = _eval_tensor("eval_plans", "evaluate_bev.eval_plans_numpy", acc)
    if not isinstance(ego_plan, torch.Tensor) or ego_plan.dim() != 5:
        raise ValueError("eval_plans: ego_plan must be a float32 tensor of shape (B, I, 6, T, 2)")
    B, I, _, T, _ = ego_plan.shape
    if B < 1 or B > 1 << 20 or not 1 <= T <= 64 or not 1 <= I <= 8:
        raise ValueError(f"eval_plans: ego_plan {tuple(ego_plan.shape)}: at least one frame, 1 .. 8 iterations, 1 .. 64 waypoints")
    words = eval_plans_words(I)
    if acc.shape[0] != words:
        raise ValueError(f"eval_plans: acc has {acc.shape[0]} words, {I} plan iterations take {words}")
    ego_plan = need("ego_plan", ego_plan, torch.float32, (B, I, 6, T, 2))
    ego_cast = need("ego_cast", ego_cast, torch.float32, (B, 6, T, 2))
    ego_cmds = need("ego_cmds", ego_cmds, torch.float32, (B, 6))
    ego_locs = need("ego_locs", ego_locs, torch.float32, (B, T + 1, 2))
    cmds = need("cmds", cmds, torch.int32, (B,))
    bras = need("bras", bras, torch.uint8, (B,))
    count = lambda t: 0 if t is None else (t.shape[0] if t.dim() else 1)
    K = count(other_cast)
    if count(other_cmds) != K or count(other_locs) != K:
        raise ValueError(f"eval_plans: {count(other_cmds)} command scores and {count(other_locs)} targets for {K} forecasts")
    if K > 1 << 24:
        raise ValueError(f"eval_plans: {K} forecasts (at most 2^24)")
    if K > 0:
        other_cast = need("other_cast", other_cast, torch.float32, (K, 6, T, 2))
        other_cmds = need("other_cmds", other_cmds, torch.float32, (K, 6))
        other_locs = need("other_locs", other_locs, torch.float32, (K, T, 2))
    else:
        other_cast = other_cmds = other_locs = None
    check(_lib.load().lav_eval_plans(_ptr(ego_plan), _ptr(ego_cast), _ptr(ego_cmds), _ptr(ego_locs), _ptr(cmds), _ptr(bras), B, I, T,
                                     _ptr(other_cast), _ptr(other_cmds), _ptr(other_locs), K, _ptr(acc), _stream()), "lav_eval_plans")
    return acc


def eval_distill_words(iters: int) -> int:
    """Length of lav_eval_distill's accumulator for `iters` plan iterations, 114 + 38 (iters + 1) (lav_eval_distill_words; host only, no
    device needed)."""
    n = int(_lib.load().lav_eval_distill_words(int(iters)))
    if n == 0:
        raise ValueError(f"eval_distill: {iters} plan iterations (1 .. 8)")
    return n


def eval_distill(acc: torch.Tensor, s_ego_plan: torch.Tensor, s_ego_cast: torch.Tensor, s_ego_cmds: torch.Tensor, t_ego_plan: torch.Tensor,
                 t_ego_cast: torch.Tensor, t_ego_cmds: torch.Tensor, ego_locs: torch.Tensor, cmds: torch.Tensor, s_other_cast=None,
                 s_other_cmds=None, t_other_cast=None, t_other_cmds=None, other_locs=None) -> torch.Tensor:
    """The student (s_*) beside the teacher (t_*) over one group of frames, the paired counters ADDED into `acc` (int64,
    ops.eval_distill_words(I) words, in HBM) by one launch on the current stream (lav_eval_distill); nothing comes back to the host.  Per
    arm ego_plan (B, I, 6, T, 2), ego_cast (B, 6, T, 2), ego_cmds (B, 6), other_cast (K, 6, T, 2), other_cmds (K, 6) float32; ego_locs
    (B, T + 1, 2) float32; cmds (B,) int32; other_locs (K, T, 2) float32 - with K = 0 the five forecast tensors may be None or empty.
    B >= 1, 1 <= T <= 64, 1 <= I <= 8.  Word for word lav_amd.train.evaluate_distill.eval_distill_numpy, which names the accumulator's
    slices (PairLayout).  Wrong shapes, dtypes, devices or an accumulator of another length raise ValueError before anything is launched."""
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.dtype != torch.int64 or acc.dim() != 1 or not acc.is_contiguous():
        raise ValueError("eval_distill: acc must be a contiguous int64 tensor in HBM (lav_amd.train.evaluate_distill.eval_distill_numpy is the CPU specification)")
    need = _eval_tensor("eval_distill", "evaluate_distill.eval_distill_numpy", acc)
    if not isinstance(s_ego_plan, torch.Tensor) or s_ego_plan.dim() != 5:
        raise ValueError("eval_distill: s_ego_plan must be a float32 tensor of shape (B, I, 6, T, 2)")
    B, I, _, T, _ = s_ego_plan.shape
    if B < 1 or B > 1 << 20 or not 1 <= T <= 64 or not 1 <= I <= 8:
        raise ValueError(f"eval_distill: s_ego_plan {tuple(s_ego_plan.shape)}: at least one frame, 1 .. 8 iterations, 1 .. 64 waypoints")
    words = eval_distill_words(I)
    if acc.shape[0] != words:
        raise ValueError(f"eval_distill: acc has {acc.shape[0]} words, {I} plan iterations take {words}")
    s_ego_plan = need("s_ego_plan", s_ego_plan, torch.float32, (B, I, 6, T, 2))
    t_ego_plan = need("t_ego_plan", t_ego_plan, torch.float32, (B, I, 6, T, 2))
    s_ego_cast = need("s_ego_cast", s_ego_cast, torch.float32, (B, 6, T, 2))
    t_ego_cast = need("t_ego_cast", t_ego_cast, torch.float32, (B, 6, T, 2))
    s_ego_cmds = need("s_ego_cmds", s_ego_cmds, torch.float32, (B, 6))
    t_ego_cmds = need("t_ego_cmds", t_ego_cmds, torch.float32, (B, 6))
    ego_locs = need("ego_locs", ego_locs, torch.float32, (B, T + 1, 2))
    cmds = need("cmds", cmds, torch.int32, (B,))
    count = lambda t: 0 if t is None else (t.shape[0] if t.dim() else 1)
    others = dict(s_other_cast=s_other_cast, s_other_cmds=s_other_cmds, t_other_cast=t_other_cast, t_other_cmds=t_other_cmds, other_locs=other_locs)
    K = count(s_other_cast)
    if any(count(t) != K for t in others.values()):
        raise ValueError(f"eval_distill: {K} forecasts, but " + ", ".join(f"{count(t)} rows of {k}" for k, t in others.items()))
    if K > 1 << 24:
        raise ValueError(f"eval_distill: {K} forecasts (at most 2^24)")
    if K > 0:
        shapes = dict(s_other_cast=(K, 6, T, 2), s_other_cmds=(K, 6), t_other_cast=(K, 6, T, 2), t_other_cmds=(K, 6), other_locs=(K, T, 2))
        others = {k: need(k, t, torch.float32, shapes[k]) for k, t in others.items()}
    else:
        others = dict.fromkeys(others)
    check(_lib.load().lav_eval_distill(_ptr(s_ego_plan), _ptr(s_ego_cast), _ptr(s_ego_cmds), _ptr(t_ego_plan), _ptr(t_ego_cast), _ptr(t_ego_cmds),
                                       _ptr(ego_locs), _ptr(cmds), B, I, T, _ptr(others["s_other_cast"]), _ptr(others["s_other_cmds"]),
                                       _ptr(others["t_other_cast"]), _ptr(others["t_other_cmds"]), _ptr(others["other_locs"]), K, _ptr(acc),
                                       _stream()), "lav_eval_distill")
    return acc


def eval_drive_words(nbins: int = 64) -> int:
    """Length of lav_eval_drive's accumulator, 92 + 6 nbins (lav_eval_drive_words; host only, no device needed)."""
    n = int(_lib.load().lav_eval_drive_words(int(nbins)))
    if n == 0:
        raise ValueError(f"eval_drive: {nbins} histogram bins (1 .. 1024)")
    return n


def eval_drive(acc: torch.Tensor, ego_plan: torch.Tensor, ego_cast: torch.Tensor, cmd: int, bra: int, ego_locs: torch.Tensor, other_cast,
               other_cmds, locs: torch.Tensor, typs: torch.Tensor, n: int, *, rules, nbins: int = 64) -> torch.Tensor:
    """The open-loop metrics of the agent's brake and aim rules over one frame, ADDED into `acc` (int64, ops.eval_drive_words(nbins) words,
    in HBM) by one launch on the current stream (lav_eval_drive); nothing comes back to the host.  ego_plan, ego_cast (T, 2) float32 (the
    cast is the commanded mode, as UniPlanner.infer_all returns it), cmd 0 .. 5, bra 0 or 1 (the expert's brake label), ego_locs
    (T + 1, 2); other_cast (N <= 64, 6, T, 2), other_cmds (N, 6) - with N = 0 they may be None or empty tensors on any device
    (UniPlanner.infer_all returns CPU zeros then); locs (G <= 64, T + 1, 2) float32, typs (G,) int32 and n <= G: the ground truth as
    the loaders return it.  2 <= T <= 64.  `rules` has the agent's constants as attributes (lav_amd.train.evaluate_drive.DriveRules):
    brake_speed, cmd_thresh, dist_static, dist_moving, behind, ego_radius and aim_point, six indices below T.  Word for word
    lav_amd.train.evaluate_drive.eval_drive_numpy, which has the definitions and names the accumulator's slices (DriveLayout).  Wrong
    shapes, dtypes, devices or values raise ValueError before anything is launched."""
    _eval_section("eval_drive", acc, eval_drive_words(nbins), "acc")
    need = _eval_tensor("eval_drive", "evaluate_drive.eval_drive_numpy", acc, copy=True)
    ego_plan = need("ego_plan", ego_plan, torch.float32, (None, 2))
    T = ego_plan.shape[0]
    if not 2 <= T <= 64:
        raise ValueError(f"eval_drive: {T} waypoints (2 .. 64)")
    ego_cast = need("ego_cast", ego_cast, torch.float32, (T, 2))
    ego_locs = need("ego_locs", ego_locs, torch.float32, (T + 1, 2))
    locs = need("locs", locs, torch.float32, (None, T + 1, 2))
    G = locs.shape[0]
    typs = need("typs", typs, torch.int32, (G,))
    if isinstance(bra, torch.Tensor):
        bra = bra.item()
    n, cmd = int(n), int(cmd)
    if G > 64 or not 0 <= n <= G:
        raise ValueError(f"eval_drive: n = {n} of {G} tracks (at most 64)")
    if not 0 <= cmd < 6:
        raise ValueError(f"eval_drive: command {cmd} (0 .. 5)")
    if bra not in (0, 1):
        raise ValueError(f"eval_drive: brake label {bra!r} (0 or 1)")
    count = lambda t: 0 if t is None else (t.shape[0] if t.dim() else 1)
    N = count(other_cast)
    if count(other_cmds) != N or N > 64:
        raise ValueError(f"eval_drive: {count(other_cmds)} rows of command scores for {N} vehicles (at most 64)")
    if N > 0:
        other_cast = need("other_cast", other_cast, torch.float32, (N, 6, T, 2))
        other_cmds = need("other_cmds", other_cmds, torch.float32, (N, 6))
    else:
        other_cast = other_cmds = None
    aim_point = [int(a) for a in rules.aim_point]
    if len(aim_point) != 6 or min(aim_point) < 0 or max(aim_point) >= T:
        raise ValueError(f"eval_drive: aim_point {aim_point}: six waypoint indices below {T}")
    scalars = [float(rules.brake_speed), float(rules.cmd_thresh), float(rules.dist_static), float(rules.dist_moving), float(rules.behind),
               float(rules.ego_radius)]
    if not all(np.isfinite(scalars)) or max(abs(s) for s in scalars) > 1e6 or min(scalars[0], scalars[2], scalars[3], scalars[5]) < 0:
        raise ValueError("eval_drive: the rule parameters must be finite, at most 1e6, and speeds, limits and the radius not negative")
    check(_lib.load().lav_eval_drive(_ptr(ego_plan), _ptr(ego_cast), _ptr(ego_locs), T, cmd, int(bra), aim_point[cmd], _ptr(other_cast),
                                     _ptr(other_cmds), N, _ptr(locs) if G else None, _ptr(typs) if G else None, G, n, *scalars, int(nbins),
                                     _ptr(acc), _stream()), "lav_eval_drive")
    return acc


def eval_det_words(nbins: int = 256) -> int:
    """Length of lav_eval_det's accumulator, 135 + 16 nbins (lav_eval_det_words; host only, no device needed)."""
    n = int(_lib.load().lav_eval_det_words(int(nbins)))
    if n == 0:
        raise ValueError(f"eval_det: {nbins} score bins (1 .. 1024)")
    return n


@functools.lru_cache(maxsize=16)
def _eval_det_thresholds(ppm, iou_thresholds, range_edges_m, heading_edges_deg):
    """lav_amd.train.evaluate_det.thresholds as the three host arrays lav_eval_det reads, computed once per setting."""
    from .train.evaluate_det import thresholds
    L, range2, hcos = thresholds(ppm, iou_thresholds, range_edges_m, heading_edges_deg)
    return ((C.c_longlong * max(1, len(L)))(*[int(v) for v in L]), len(L), (C.c_double * max(1, len(range2)))(*[float(v) for v in range2]), len(range2),
            (C.c_double * max(1, len(hcos)))(*[float(v) for v in hcos]), len(hcos))


def eval_det(acc: torch.Tensor, rows: torch.Tensor, locs: torch.Tensor, typs: torch.Tensor, n: int, size_map: torch.Tensor, ori_map: torch.Tensor,
             *, ppm: float, centre, radius_px: float, iou_thresholds=(0.3, 0.5, 0.7), range_edges_m=(15, 30, 50),
             heading_edges_deg=(5, 10, 20, 45, 90, 135, 175), min_score: float = 0.1, det_score: float = 0.2, nbins: int = 256) -> torch.Tensor:
    """The rotated-box metrics of one frame's detections, ADDED into `acc` (int64, ops.eval_det_words(nbins) words, in HBM) by one launch
    on the current stream (lav_eval_det); nothing comes back to the host.  rows (2, D <= 32, 7) float32 = (score, x, y, w, h, cos, sin)
    of extract_peaks / LiDARModel.detect, read where they are; locs (G <= 64, T + 1, 2) float32, typs (G,) int32 and n: the ground truth
    as the loaders return it; size_map, ori_map (2, H, W) float32: the loaders' regression targets, from which the ground-truth boxes
    are read.  centre = the ego pixel (x, y).  At most 3 IoU thresholds in (0, 1], 3 ascending range edges (metres) and 7 ascending
    heading edges (degrees); they reach the kernel as lav_amd.train.evaluate_det.thresholds makes them.  Word for word
    lav_amd.train.evaluate_det.eval_det_numpy, which has the definitions and names the accumulator's slices (DetLayout).  Wrong shapes,
    dtypes, devices or values raise ValueError before anything is launched."""
    _eval_section("eval_det", acc, eval_det_words(nbins), "acc")
    need = _eval_tensor("eval_det", "evaluate_det.eval_det_numpy", acc, copy=True)
    rows = need("rows", rows, torch.float32, (2, None, 7))
    D = rows.shape[1]
    if not 1 <= D <= 32:
        raise ValueError(f"eval_det: {D} rows per class (1 .. 32)")
    locs = need("locs", locs, torch.float32, (None, None, 2))
    G, T = locs.shape[0], locs.shape[1] - 1
    if G > 64 or T < 0:
        raise ValueError(f"eval_det: locs {tuple(locs.shape)}: at most 64 actors, at least their position")
    typs = need("typs", typs, torch.int32, (G,))
    n = int(n)
    if not 0 <= n <= G:
        raise ValueError(f"eval_det: n = {n} of {G} actors")
    size_map = need("size_map", size_map, torch.float32, (2, None, None))
    H, W = size_map.shape[1:]
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"eval_det: maps of {H} x {W} pixels")
    ori_map = need("ori_map", ori_map, torch.float32, (2, H, W))
    scalars = [float(ppm), float(centre[0]), float(centre[1]), float(radius_px), float(min_score), float(det_score)]
    if not all(np.isfinite(scalars)) or not 0 < scalars[0] <= 1e6 or scalars[3] < 0 or scalars[4] < 0:
        raise ValueError("eval_det: scalars must be finite, pixels per metre positive, the radius and min_score not negative")
    L, nl, range2, nr, hcos, nh = _eval_det_thresholds(scalars[0], tuple(float(t) for t in iou_thresholds), tuple(float(e) for e in range_edges_m),
                                                       tuple(float(e) for e in heading_edges_deg))
    check(_lib.load().lav_eval_det(_ptr(rows), D, _ptr(locs) if G else None, _ptr(typs) if G else None, G, n, T, _ptr(size_map), _ptr(ori_map), H, W,
                                   *scalars, L, nl, range2, nr, hcos, nh, int(nbins), _ptr(acc), _stream()), "lav_eval_det")
    return acc


EVAL_RESAMPLE_MAX_ROWS = 1 << 20          # lav_eval_resample: idx = (u * R) >> 32 favours rows by at most R / 2^32
EVAL_RESAMPLE_MAX_BYTES = 4 << 30         # of the row table


def eval_resample_chunk() -> int:
    """How many of a replicate's draws lav_eval_resample holds in LDS at a time (lav_eval_resample_chunk; host only, no device needed)."""
    return int(_lib.load().lav_eval_resample_chunk())


def eval_resample(rows: torch.Tensor, B: int, seed: int) -> torch.Tensor:
    """Block-bootstrap replicates of a row table, one launch on the current stream (lav_eval_resample): rows (R, W) int64 in HBM, read
    where they are -> (B + 1, W) int64 in HBM.  out[0] = rows.sum(0), the identity replicate; out[b], b = 1 .. B, is the sum of R rows
    drawn with replacement, idx(b, j) = (u * R) >> 32 with u = word j & 3 of Philox4x32-10 at counter (j >> 2, b, 0x52534D50, 0) and key
    (seed low word, seed high word).  That map favours some rows by at most R / 2^32, below 2.5e-4 at the cap of 2^20 rows.  Word for
    word lav_amd.train.eval_common.eval_resample_numpy.  Wrong shapes, dtypes or devices raise ValueError before anything is launched."""
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise ValueError("eval_resample: rows must be a tensor in HBM (cuda/hip device); lav_amd.ops has no CPU path "
                         "(lav_amd.train.eval_common.eval_resample_numpy is the CPU specification)")
    if rows.dtype != torch.int64 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError(f"eval_resample: rows must be a contiguous int64 tensor of shape (R, W), got {rows.dtype} {tuple(rows.shape)}")
    R, W = rows.shape
    B = int(B)
    if not 1 <= R <= EVAL_RESAMPLE_MAX_ROWS or W < 1 or R * W * 8 > EVAL_RESAMPLE_MAX_BYTES:
        raise ValueError(f"eval_resample: a table of {R} x {W} words (1 .. 2^20 rows, at least one word, at most 4 GiB)")
    if not 0 <= B < (1 << 31) - 1:
        raise ValueError(f"eval_resample: {B} replicates")
    out = torch.empty((B + 1, W), dtype=torch.int64, device=rows.device)
    check(_lib.load().lav_eval_resample(_ptr(rows), R, W, B, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out), _stream()), "lav_eval_resample")
    return out


# ------------------------------------------------------------------------------------------ GRU decoders
def gru_cast(embd, w_ih, w_hh, b_ih, b_hh, mlp_w, mlp_b, T: int):
    """embd (B, E); stacked per-command GRU/MLP weights -> (B, num_cmds, T, 2)."""
    lib = _lib.load()
    embd = _f32c(embd, "embd")
    B, E = embd.shape
    ncmd, g3, _ = w_ih.shape
    H = g3 // 3
    out = torch.empty((B, ncmd, T, 2), dtype=torch.float32, device=embd.device)
    check(lib.lav_gru_cast(_ptr(embd), B, E, H, ncmd, T, _ptr(w_ih), _ptr(w_hh), _ptr(b_ih), _ptr(b_hh), _ptr(mlp_w),
                           _ptr(mlp_b), _ptr(out), None, 0, _stream()), "lav_gru_cast")
    return out


def embed_cast(feat, w_ih, w_hh, b_ih, b_hh, mlp_w, mlp_b, T: int, cmd_w=None, cmd_b=None, oris=None, locs=None, want_embd=True):
    """feat (B, E, h, w) (the embedder's last map) or (B, E) -> (embd (B,E) or None, cast (B,num_cmds,T,2), cmds (B,num_cmds) or
    None): spatial mean, the six cast GRUs, the command scores and the rotation / translation of the waypoints into the ego
    frame in ONE launch (lav_embed_cast)."""
    lib = _lib.load()
    feat = _f32c(feat, "feat")
    B, E = feat.shape[0], feat.shape[1]
    hw = feat.numel() // max(B * E, 1) if B else 1
    ncmd, g3, _ = w_ih.shape
    dev = feat.device
    out = torch.empty((B, ncmd, T, 2), dtype=torch.float32, device=dev)
    embd = torch.empty((B, E), dtype=torch.float32, device=dev) if want_embd else None
    cmds = torch.empty((B, ncmd), dtype=torch.float32, device=dev) if cmd_w is not None else None
    check(lib.lav_embed_cast(_ptr(feat), B, E, hw, _ptr(embd), g3 // 3, ncmd, T, _ptr(w_ih), _ptr(w_hh), _ptr(b_ih), _ptr(b_hh),
                             _ptr(mlp_w), _ptr(mlp_b), _ptr(None if cmd_w is None else _f32c(cmd_w, "cmd_w")),
                             _ptr(None if cmd_b is None else _f32c(cmd_b, "cmd_b")), _ptr(cmds),
                             _ptr(None if oris is None else _f32c(oris.reshape(-1), "oris")),
                             _ptr(None if locs is None else _f32c(locs.reshape(-1, 2), "locs")), _ptr(out), _stream()), "lav_embed_cast")
    return embd, out, cmds


def gru_plan(embd, nxp, cast_locs, w_ih, w_hh, b_ih, b_hh, mlp_w, mlp_b, iters: int, cmd: int, ppm: float,
             crop_size: float, impl: str = "auto"):
    """embd (B,H), nxp (B,2), cast_locs (B,num_cmds,T,2) -> (B, iters, num_cmds or 1, T, 2).
    impl "auto": the persistent one-launch kernel when it applies (a launch that could not complete returns NaN and
    raises gru_plan_status); "steps": one launch per GRU step, no co-residency requirement."""
    lib = _lib.load()
    embd = _f32c(embd, "embd")
    nxp = _f32c(nxp, "nxp")
    cast_locs = _f32c(cast_locs, "cast_locs")
    B, H = embd.shape
    _, ncmd, T, _ = cast_locs.shape
    nc = 1 if cmd >= 0 else ncmd
    out = torch.empty((B, iters, nc, T, 2), dtype=torch.float32, device=embd.device)
    nbytes = lib.lav_gru_plan_workspace_bytes(B, H, ncmd, T)
    ws = _workspace("plan", nbytes, embd.device)
    fn = {"auto": lib.lav_gru_plan, "steps": lib.lav_gru_plan_steps}[impl]
    check(fn(_ptr(embd), _ptr(nxp), _ptr(cast_locs), B, H, ncmd, T, iters, cmd, float(ppm),
             float(crop_size), _ptr(w_ih), _ptr(w_hh), _ptr(b_ih), _ptr(b_hh), _ptr(mlp_w), _ptr(mlp_b),
             _ptr(out), _ptr(ws), ws.numel(), _stream()), "lav_gru_plan")
    return out


class _GruSeq(torch.autograd.Function):
    """GRU recurrence over a sequence on lav_gru_seq_forward / lav_gru_seq_backward (one launch per step, MFMA recurrent
    GEMM fused with the gates).  Differentiable in x (the input-side pre-activations), h0, w_hh and b_hh; the weight
    gradients are two GEMMs over the tape (rocBLAS through torch)."""

    @staticmethod
    def forward(ctx, x, h0, w_hh, b_hh, T):
        lib = _lib.load()
        x, h0 = _f32c(x, "x"), _f32c(h0, "h0")
        w_hh, b_hh = _f32c(w_hh, "w_hh"), _f32c(b_hh, "b_hh")
        R, H = h0.shape
        per_step = x.dim() == 3
        if (per_step and tuple(x.shape) != (R, T, 3 * H)) or (not per_step and tuple(x.shape) != (R, 3 * H)):
            raise RuntimeError(f"gru_seq: x has shape {tuple(x.shape)}, expected ({R}, {T}, {3 * H}) or ({R}, {3 * H})")
        if tuple(w_hh.shape) != (3 * H, H) or b_hh.numel() != 3 * H:
            raise RuntimeError("gru_seq: w_hh must be (3H, H) and b_hh (3H,)")
        out = torch.empty((R, T, H), dtype=torch.float32, device=x.device)
        need_tape = any(ctx.needs_input_grad[:4])
        tape = torch.empty((R, T, 4, H), dtype=torch.float32, device=x.device) if need_tape else None
        train_work["gru_seq_forward_flops"] += 2 * R * H * 3 * H * T
        check(lib.lav_gru_seq_forward(_ptr(x), int(per_step), _ptr(h0), _ptr(w_hh), _ptr(b_hh), R, T, H, _ptr(out),
                                      _ptr(tape) if need_tape else None, _stream()), "lav_gru_seq_forward")
        if need_tape:
            ctx.save_for_backward(tape, out, h0, w_hh)
            ctx.per_step = per_step
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        tape, out, h0, w_hh = ctx.saved_tensors
        R, T, H = out.shape
        dout = _f32c(dout, "dout")
        dx = torch.empty((R, T, 3 * H), dtype=torch.float32, device=out.device)
        dgh = torch.empty((R, T, 3 * H), dtype=torch.float32, device=out.device)
        dh0 = torch.empty((R, H), dtype=torch.float32, device=out.device)
        if R == 0:
            return (dx if ctx.per_step else dx.sum(1)), dh0, torch.zeros_like(w_hh), w_hh.new_zeros(3 * H), None
        ws = _workspace("gru_seq_bwd", lib.lav_gru_seq_backward_workspace_bytes(R, H), out.device)
        w_hh_t = w_hh.t().contiguous()
        train_work["gru_seq_backward_flops"] += 2 * R * 3 * H * H * T
        check(lib.lav_gru_seq_backward(_ptr(dout), _ptr(tape), _ptr(out), _ptr(h0), _ptr(w_hh_t), R, T, H, _ptr(dx), _ptr(dgh),
                                       _ptr(dh0), _ptr(ws), ws.numel(), _stream()), "lav_gru_seq_backward")
        h_prev = torch.cat([h0[:, None], out[:, :-1]], dim=1)                       # (R, T, H): the state each step started from
        dw_hh = dgh.view(R * T, 3 * H).t() @ h_prev.reshape(R * T, H)
        db_hh = dgh.sum(dim=(0, 1))
        return (dx if ctx.per_step else dx.sum(1)), dh0, dw_hh, db_hh, None


def gru_seq(x, h0, w_hh, b_hh, T: int):
    """h_t = GRUCell(x_t, h_{t-1}) for t < T with the input side already projected: x (R,T,3H) or (R,3H) (the same input at
    every step) = W_ih u + b_ih in torch's gate order (r, z, n); h0 (R,H) -> (R,T,H).  Same arithmetic as nn.GRU."""
    return _GruSeq.apply(x, h0, w_hh, b_hh, int(T))


def _plan_workspace(device, stream):
    """(the plan workspace of `stream` on `device` or None when gru_plan has not run there, the stream)"""
    device, st = _device_and_stream(device, stream)
    return _workspaces.get(("plan", device, st.cuda_stream)), st


def gru_plan_status(B: int, H: int, num_cmds: int, cmd: int, device, stream=None) -> int:
    """Status word of the last gru_plan launch on `stream` (default: the current one) with these sizes: 0 = completed,
    1 = the persistent kernel gave up waiting for its peers and returned NaN.  Synchronises that stream."""
    ws, st = _plan_workspace(device, stream)
    if ws is None:
        return 0
    status = C.c_int(0)
    check(_lib.load().lav_gru_plan_status(_ptr(ws), ws.numel(), B, H, num_cmds, cmd, C.byref(status), st.cuda_stream), "lav_gru_plan_status")
    return int(status.value)


def gru_plan_diag(B: int, H: int, num_cmds: int, cmd: int, device, stream=None) -> dict:
    """The diagnosis words of the last persistent gru_plan launch on `stream` (include/lav_amd.h: lav_gru_plan_diag)."""
    ws, st = _plan_workspace(device, stream)
    names = ("status", "entered", "abort_wg_plus1", "abort_wave", "abort_epoch", "abort_spins", "missing_granule", "tag_seen",
             "abort_us", "completed", "aborted_launches", "launches")
    if ws is None:
        return dict.fromkeys(names, 0)
    words = (C.c_int * 16)()
    check(_lib.load().lav_gru_plan_diag(_ptr(ws), ws.numel(), B, H, num_cmds, cmd, words, st.cuda_stream), "lav_gru_plan_diag")
    return dict(zip(names, list(words)))


# ------------------------------------------------------------------------------------------ conv
_precision_stack = _threading.local()


def infer_precision() -> int:
    """lav_conv.precision of the eval-mode engines built from now on by this thread: the innermost `with precision(...)`, else
    LAV_INFER_PRECISION (f16x3 | bf16x6 | f32, default: the library's, i.e. LAV_CONV_PRECISION / bf16x6).  The frame pipelines and
    InferModel ask for LAV_CONV_F16X3 (round 6: every split-kernel layer on two fp16 pieces, the scale handed from layer to layer);
    an engine a trainer builds by calling a module directly keeps the default (its layers are re-packed on the device after every
    step, which the fp16 packing does not support)."""
    st = getattr(_precision_stack, "v", None)
    if st:
        return st[-1]
    return {"f16x3": _lib.CONV_F16X3, "bf16x6": _lib.CONV_BF16X6, "f32": _lib.CONV_F32, "fp32": _lib.CONV_F32}.get(
        _os.environ.get("LAV_INFER_PRECISION", ""), 0)


class precision:
    """with ops.precision(_lib.CONV_F16X3): ... - the eval engines used inside are the ones packed for that precision (engines are
    cached per precision on their modules: nothing is written onto a module that somebody else owns)."""

    def __init__(self, p: int):
        self.p = int(p)

    def __enter__(self):
        st = getattr(_precision_stack, "v", None)
        if st is None:
            st = _precision_stack.v = []
        st.append(self.p)
        return self

    def __exit__(self, *exc):
        _precision_stack.v.pop()
        return False


def frame_heads_at_peaks() -> bool:
    """LAV_HEADS_AT_PEAKS (default 1): the frame pipelines evaluate the box / orientation heads at the peak rows only
    (LiDARModel.detect, lav_heads_at_peaks); 0 restores the dense four-head maps gathered by lav_extract_peaks."""
    return _os.environ.get("LAV_HEADS_AT_PEAKS", "1") != "0"


def frame_precision() -> int:
    """What the inference pipelines run at: LAV_CONV_F16X3 unless LAV_CONV_PRECISION asks for the exact-fp32 kernels or
    LAV_INFER_PRECISION says bf16x6."""
    if _os.environ.get("LAV_CONV_PRECISION", "") in ("f32", "fp32"):
        return 0
    want = _os.environ.get("LAV_INFER_PRECISION", "f16x3")
    return _lib.CONV_F16X3 if want == "f16x3" else 0


class Amax:
    """Maxima of the finite |values| of a tensor, in parts, as the launches that wrote it left them (lav_conv2d_amax): the next
    LAV_CONV_F16X3 layer takes its power-of-two activation scale from them instead of measuring its input.  One fixed buffer;
    `take(n)` hands out the next n slots (the same addresses on every pass over the same layers: HIP graphs may hold them).
    `generation` counts the resets: a bound handed on with a tensor (tag_amax) names the generation it was written in."""
    CAPACITY = 20480

    def __init__(self, device, capacity: Optional[int] = None, zeroed: bool = True):
        self.CAPACITY = int(capacity) if capacity else Amax.CAPACITY
        self.buf = (torch.zeros if zeroed else torch.empty)(self.CAPACITY, dtype=torch.float32, device=device)
        self.count = 0
        self.generation = 0

    def reset(self):
        self.count = 0
        self.generation += 1      # (the launches that follow rewrite the parts: every bound handed on before is void)
        return self

    def take(self, n: int) -> torch.Tensor:
        if self.count + n > self.CAPACITY:
            raise RuntimeError(f"Amax: {self.count} + {n} parts exceed the buffer ({self.CAPACITY})")
        v = self.buf[self.count:self.count + n]
        self.count += n
        return v


def tag_amax(t, am):
    """Attach the Amax whose parts bound |t| to the tensor OBJECT t (the producer's side of amax_of), stamped with the tensor's
    version and the Amax's generation: an in-place change of t, or a later call that resets the Amax (the same layers on another
    input of the same shape), voids the bound.  am None: t is returned untagged.  The only writer of these two attributes, for the
    inference engines and the training layers (train.hipnn) alike: the training Amaxes are made fresh per launch and never reset(),
    their generation stays 0 and the stamp comes down to the version check; one Amax may describe several tensors (hipnn.carry)."""
    if am is None:
        return t
    t._lav_amax = am
    t._lav_amax_stamp = (id(am), t._version, am.generation)
    return t


def amax_of(t):
    """The Amax a producer attached to the tensor OBJECT it returned (engine-internal hand-off between modules: backbone -> heads /
    crops), while it still bounds the tensor; None for anything else - the consumer then measures its input (one launch more,
    the same result).  A bound, not a measurement: valid for the tensor and for whatever is a max-pool, a crop or a bilinear
    resampling of it."""
    am, stamp = getattr(t, "_lav_amax", None), getattr(t, "_lav_amax_stamp", None)
    if am is None or stamp is None:
        return None
    return am if stamp == (id(am), t._version, am.generation) else None


def amax_key(x):
    """Key of a module's Amax list for input x: its shape and the current stream.  Launches on different streams may run
    concurrently (the frame's ego and others graphs: crop batches of one shape on s_ego and s_cap), so they never share the
    buffers their layers leave maxima in - as the split-K workspaces (_workspace)."""
    return tuple(x.shape), torch.cuda.current_stream(x.device).cuda_stream


def bn_fold(mean, var, gamma, beta, eps):
    """Eval-mode BatchNorm as y = x * scale + shift: (scale, shift) in float64, on the device the statistics live on."""
    mean, var, gamma, beta = (t.detach().double() for t in (mean, var, gamma, beta))
    scale = gamma / torch.sqrt(var + eps)
    return scale, beta - mean * scale


class ConvLayer:
    """One fused convolution of the C ABI: packed weights + epilogue vectors resident in HBM.

    Built once from PyTorch-layout parameters (host-side repack in the library), then
    `__call__(x, out=None, residual=None)` enqueues lav_conv2d.
    """

    def __init__(self, weight: torch.Tensor, *, stride=1, padding=(0, 0), dilation=(1, 1), transposed=False,
                 output_padding=0, bias: Optional[torch.Tensor] = None, bn=None, bn_eps: float = 1e-5,
                 relu_pre=False, relu_post=False, sigmoid=False, in_c_total=None, in_c_offset=0, out_c_total=None, target_cus=0, pad_value=0.0,
                 out_c_offset=0, precision=0, device=None):
        lib = _lib.load()
        # the sources are kept by reference (tensors, or callables that assemble them): refresh() re-packs from their current values
        self._src = dict(weight=weight, bias=bias, bn=bn, bn_eps=float(bn_eps))
        self._map = None
        src_dev = None
        if callable(weight):
            weight = weight()
        if callable(bias):
            bias = bias()
        if callable(bn):
            bn = bn()
        src_dev = weight.device
        w = weight.detach().to("cpu", torch.float32).contiguous()
        if transposed:
            cin, cout, kh, kw = w.shape
        else:
            cout, cin, kh, kw = w.shape
        if isinstance(padding, int):
            padding = (padding, padding)
        if isinstance(dilation, int):
            dilation = (dilation, dilation)
        self.cin, self.cout = cin, cout
        self.in_c_total = in_c_total if in_c_total is not None else cin
        self.out_c_total = out_c_total if out_c_total is not None else cout
        self.desc = Conv(1, self.in_c_total, in_c_offset, cin, 0, 0, cout, kh, kw, int(stride), int(padding[0]),
                         int(padding[1]), int(dilation[0]), int(dilation[1]), int(bool(transposed)),
                         int(output_padding), self.out_c_total, out_c_offset, int(relu_pre), int(relu_post),
                         int(sigmoid), int(target_cus), float(pad_value), int(precision))
        probe = self._desc()
        nfl = lib.lav_conv_packed_weight_floats(C.byref(probe))
        if nfl == 0:
            raise RuntimeError("lav_conv_packed_weight_floats: " + lib.lav_last_error().decode())
        packed = torch.empty(nfl, dtype=torch.float32)
        check(lib.lav_conv_pack_weights(C.byref(probe), w.data_ptr(), packed.data_ptr()), "lav_conv_pack_weights")
        dev = device if device is not None else src_dev
        self.w = packed.to(dev)
        self.bias = None if bias is None else bias.detach().to(dev, torch.float32).contiguous()
        self._ws_bytes = {}
        self.scale = self.shift = None
        if bn is not None:  # eval-mode BatchNorm as y = x*scale + shift, folded in float64 on the host
            self.scale, self.shift = (v.to(torch.float32).to(dev) for v in bn_fold(*[t.detach().cpu() for t in bn], bn_eps))

    def _desc(self, B=1, h=64, w=64):
        """A copy of the descriptor for a (B, ., h, w) input (the default: a probe for the calls that only read the layer's geometry)."""
        d = Conv.from_buffer_copy(self.desc)
        d.batch, d.h, d.w = B, h, w
        return d

    def refresh(self):
        """Re-pack the weights and re-fold the epilogue vectors from the CURRENT values of the tensors this layer was built from
        (parameters that an optimiser step or load_state_dict changed in place).  With everything resident in HBM this is one
        gather launch (lav_conv_repack through the layer's index map) plus lav_bn_fold - no host round trip, bit-identical to
        building the layer anew; anything else falls back to the host packer."""
        lib = _lib.load()
        src = self._src
        get = lambda v: v() if callable(v) else v
        w, bias, bn = get(src["weight"]), get(src["bias"]), get(src["bn"])
        dev = self.w.device
        probe = self._desc()
        if dev.type == "cuda" and w.device == dev and self._map is not False:
            if self._map is None:
                n = lib.lav_conv_pack_map_ints(C.byref(probe))
                m = torch.empty(max(n, 1), dtype=torch.int32)
                if n == 0 or lib.lav_conv_pack_map(C.byref(probe), m.data_ptr()) != 0:
                    self._map = False
                else:
                    self._map = m.to(dev)
        if dev.type == "cuda" and w.device == dev and self._map is not False and self._map is not None:
            wd = w.detach().to(torch.float32).contiguous()
            if self.desc.precision == _lib.CONV_F16X3:   # (the fp16 pieces are scaled by the weights' largest magnitude: measured into 512 floats of scratch)
                sc = _workspace("conv_repack", 512 * 4, dev)
                check(lib.lav_conv_repack_scratch(C.byref(probe), _ptr(wd), _ptr(self._map), _ptr(self.w), _ptr(sc), 512, _stream()), "lav_conv_repack_scratch")
            else:
                check(lib.lav_conv_repack(C.byref(probe), _ptr(wd), _ptr(self._map), _ptr(self.w), _stream()), "lav_conv_repack")
        else:
            packed = torch.empty(self.w.numel(), dtype=torch.float32)
            wh = w.detach().to("cpu", torch.float32).contiguous()
            check(lib.lav_conv_pack_weights(C.byref(probe), wh.data_ptr(), packed.data_ptr()), "lav_conv_pack_weights")
            self.w.copy_(packed)
        if self.bias is not None:
            self.bias.copy_(bias.detach())
        if bn is not None:
            if dev.type == "cuda" and all(t.device == dev for t in bn):
                mean, var, gamma, beta = [t.detach().to(torch.float32).contiguous() for t in bn]
                check(lib.lav_bn_fold(_ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), src["bn_eps"], mean.numel(), _ptr(self.scale),
                                      _ptr(self.shift), _stream()), "lav_bn_fold")
            else:
                scale, shift = bn_fold(*[t.detach().cpu() for t in bn], src["bn_eps"])
                self.scale.copy_(scale.to(torch.float32))
                self.shift.copy_(shift.to(torch.float32))

    @classmethod
    def from_module(cls, conv, bn=None, bn_slice=None, **kw):
        """Build from nn.Conv2d / nn.ConvTranspose2d (+ optional nn.BatchNorm2d, optionally a channel slice of it)."""
        import torch.nn as nn
        tr = isinstance(conv, nn.ConvTranspose2d)
        if conv.stride[0] != conv.stride[1]:
            raise RuntimeError("anisotropic stride unsupported")
        bnt, eps = None, 1e-5
        if bn is not None:
            sl = bn_slice if bn_slice is not None else slice(None)
            bnt = tuple(t[sl] for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias))
            eps = bn.eps
        return cls(conv.weight, stride=conv.stride[0], padding=tuple(conv.padding), dilation=tuple(conv.dilation),
                   transposed=tr, output_padding=conv.output_padding[0] if tr else 0, bias=conv.bias, bn=bnt, bn_eps=eps,
                   device=kw.pop("device", conv.weight.device), **kw)

    def out_hw(self, h: int, w: int):
        oh, ow = C.c_int(), C.c_int()
        check(_lib.load().lav_conv_out_hw(C.byref(self._desc(1, h, w)), C.byref(oh), C.byref(ow)), "lav_conv_out_hw")
        return oh.value, ow.value

    def uses_amax(self, B: int, h: int, w: int) -> bool:
        """Whether this layer on a (B, ., h, w) input runs the fp16 three-product plan, i.e. has a use for its producers' maxima."""
        key = ("f16", B, h, w, _os.environ.get("LAV_CONV_SPLIT"))
        v = self._ws_bytes.get(key)
        if v is None:
            v = False
            if self.desc.precision == _lib.CONV_F16X3:
                info = (C.c_int * 9)()
                v = _lib.load().lav_conv_tile_info(C.byref(self._desc(B, h, w)), info) == 0 and info[0] == -1 and info[7] >= 200
            self._ws_bytes[key] = v
        return v

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 amax_in: Optional["Amax"] = None, amax_out: Optional["Amax"] = None):
        """amax_in: maxima that bound |x| (an Amax its producers filled); amax_out: an Amax this launch appends the maxima of |y| to."""
        x = _f32c(x, "x")
        B, ct, h, w = x.shape
        if ct != self.in_c_total:
            raise RuntimeError(f"conv input has {ct} channels, layer expects {self.in_c_total}")
        d = self._desc(B, h, w)
        oh, ow = self.out_hw(h, w)
        if out is None:
            out = torch.empty((B, self.out_c_total, oh, ow), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (B, self.out_c_total, oh, ow) or not out.is_contiguous():
            raise RuntimeError(f"conv output buffer {tuple(out.shape)} != {(B, self.out_c_total, oh, ow)}")
        if residual is not None:
            residual = _f32c(residual, "residual")
            if residual.shape != out.shape:
                raise RuntimeError("residual shape mismatch")
        lib = _lib.load()
        key = (B, h, w, _os.environ.get("LAV_CONV_SPLIT"))   # lav_conv2d re-reads the plan knobs per call: the cached size follows them
        nbytes = self._ws_bytes.get(key)
        if nbytes is None:
            nbytes = self._ws_bytes[key] = lib.lav_conv_workspace_bytes(C.byref(d))
        ws = _workspace("conv", nbytes, x.device) if nbytes else None
        a_in = amax_in.buf if amax_in is not None and amax_in.count > 0 else None
        a_out = None
        if amax_out is not None:
            ck = ("amax", B, h, w, _os.environ.get("LAV_CONV_SPLIT"))
            n_out = self._ws_bytes.get(ck)
            if n_out is None:
                n_out = self._ws_bytes[ck] = lib.lav_conv_amax_count(C.byref(d))
            if n_out < 1:
                raise RuntimeError("lav_conv_amax_count: " + lib.lav_last_error().decode())
            a_out = amax_out.take(n_out)
        check(lib.lav_conv2d_amax(C.byref(d), _ptr(x), _ptr(self.w), _ptr(self.bias), _ptr(self.scale), _ptr(self.shift),
                                  _ptr(residual), _ptr(out), _ptr(ws), ws.numel() if ws is not None else 0,
                                  _ptr(a_in), amax_in.count if a_in is not None else 0, _ptr(a_out), _stream()),
              "lav_conv2d" if amax_in is None and amax_out is None else "lav_conv2d_amax")   # (lav_conv2d is this call with no maxima)
        return out


class GroupedDeconv:
    """ConvTranspose2d layers with few output channels that share geometry and read disjoint channel groups of one
    input, as ONE lav_deconv_grouped launch (memory-bound vector kernel): the tails of the detection / segmentation heads
    (4 x 64 channels -> 1 + 2 + 2 + 4), or a single layer (groups = 1: ERFNet's output layer)."""

    def __init__(self, deconvs, sigmoid_from: int = -1, softmax: bool = False, device=None):
        ct0 = deconvs[0]
        for ct in deconvs:
            if (ct.kernel_size, ct.stride, ct.padding, ct.output_padding, ct.in_channels) != \
                    (ct0.kernel_size, ct0.stride, ct0.padding, ct0.output_padding, ct0.in_channels) or ct.dilation != (1, 1) or ct.groups != 1:
                raise RuntimeError("GroupedDeconv: layers must share kernel / stride / padding / input channels")
        k, s_ = ct0.kernel_size, ct0.stride
        if k[0] != k[1] or s_[0] != s_[1] or (k[0], s_[0]) not in ((3, 2), (2, 2)) or ct0.padding[0] != ct0.padding[1]:
            raise RuntimeError(f"GroupedDeconv: kernel {k} stride {s_} unsupported")
        dev = device if device is not None else ct0.weight.device
        self.k, self.s, self.pad, self.opad = k[0], s_[0], ct0.padding[0], ct0.output_padding[0]
        self.cin_g, self.groups = ct0.in_channels, len(deconvs)
        self.outs = [ct.out_channels for ct in deconvs]
        if max(self.outs) > 8 or self.groups > 8:
            raise RuntimeError("GroupedDeconv: at most 8 groups of at most 8 output channels")
        self._deconvs, self._dev = list(deconvs), dev
        self.w = self.bias = None
        self.refresh()
        self._outs_c = (C.c_int * self.groups)(*self.outs)
        self.sigmoid_from = -2 if softmax else int(sigmoid_from)     # -2: softmax over each group's channels, in the epilogue

    def refresh(self):
        """(Re-)read the layers' parameters: concatenated where they live, moved once."""
        w = torch.cat([ct.weight.detach().to(torch.float32).reshape(-1) for ct in self._deconvs]).to(self._dev)
        b = None
        if self._deconvs[0].bias is not None:
            b = torch.cat([ct.bias.detach().to(torch.float32) for ct in self._deconvs]).to(self._dev)
        if self.w is None:
            self.w, self.bias = w, b
        else:   # in place: captured graphs hold these addresses
            self.w.copy_(w)
            if b is not None:
                self.bias.copy_(b)

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None):
        x = _f32c(x, "x")
        B, c, h, w = x.shape
        if c != self.cin_g * self.groups:
            raise RuntimeError(f"GroupedDeconv input has {c} channels, expects {self.cin_g * self.groups}")
        oh = (h - 1) * self.s - 2 * self.pad + self.k + self.opad
        ow = (w - 1) * self.s - 2 * self.pad + self.k + self.opad
        if out is None:
            out = torch.empty((B, sum(self.outs), oh, ow), dtype=torch.float32, device=x.device)
        check(_lib.load().lav_deconv_grouped(B, c, h, w, self.groups, self._outs_c, self.k, self.s, self.pad, self.opad, _ptr(x),
                                             _ptr(self.w), _ptr(self.bias), self.sigmoid_from, _ptr(out), _stream()),
              "lav_deconv_grouped")
        return out


class PointwiseUpconv:
    """ConvTranspose2d with kernel == stride (no bias) -> ReLU -> eval BatchNorm into a channel slice of a wider map, as ONE
    lav_upconv_pointwise launch: exact fp32 matrix products, no pipeline to fill (round 6: the BEV backbone's 1x1 and 4x4 / stride-4
    up-convolutions, 21.5 + 31.1 us on the implicit-GEMM kernels).  Same call surface as the ConvLayer it stands in for:
    `__call__(x, out=, amax_in=, amax_out=)`, `out_hw`, `uses_amax` (never: it reads fp32), `refresh` (re-packs on the device)."""

    @staticmethod
    def takes(ct, device=None) -> bool:
        k, s = ct.kernel_size, ct.stride
        return (isinstance(ct, torch.nn.ConvTranspose2d) and k[0] == k[1] == s[0] == s[1] and k[0] in (1, 4) and ct.bias is None
                and ct.in_channels in (64, 128) and ct.out_channels % (128 if k[0] == 1 else 32) == 0 and ct.groups == 1
                and ct.dilation == (1, 1) and ct.padding[0] == ct.padding[1] < k[0] and ct.output_padding[0] == ct.output_padding[1]
                and (k[0] > 1 or (ct.padding[0] == 0 and ct.output_padding[0] == 0))
                and _os.environ.get("LAV_UPCONV_POINTWISE", "1") != "0")

    def __init__(self, ct, bn, *, relu_pre=True, out_c_total=None, out_c_offset=0, device=None):
        if not PointwiseUpconv.takes(ct):
            raise RuntimeError("PointwiseUpconv: ConvTranspose2d with kernel == stride in {1, 4}, 64 / 128 input channels, no bias")
        self.k, self.pad, self.opad = ct.kernel_size[0], ct.padding[0], ct.output_padding[0]
        self.cin, self.cout = ct.in_channels, ct.out_channels
        self.relu_pre = bool(relu_pre)
        self.out_c_total = int(out_c_total) if out_c_total else self.cout
        self.out_c_offset = int(out_c_offset)
        self._src = (ct.weight, bn)
        self.device = torch.device(device) if device is not None else ct.weight.device
        self.w = self.scale = self.shift = None
        self.refresh()

    def refresh(self):
        """Packed weights and folded BatchNorm from the CURRENT parameter values: a permutation and five small float64 launches on the
        device the parameters live on (lav_upconv_pointwise_pack is the host form of the same permutation)."""
        w, bn = self._src
        w = w.detach().to(torch.float32)
        if self.k == 1:   # [ci][co] -> [128-cout tile][32-cout tile j][ci][32]
            p = w.reshape(self.cin, self.cout // 128, 4, 32).permute(1, 2, 0, 3)
        else:             # [ci][co][ky][kx] -> [ky][32-cout tile][kx][ci][32]
            p = w.reshape(self.cin, self.cout // 32, 32, 4, 4).permute(3, 1, 4, 0, 2)
        p = p.contiguous().reshape(-1).to(self.device)
        scale, shift = bn_fold(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps)
        if self.w is None:
            self.w, self.scale, self.shift = p, scale.float().to(self.device).contiguous(), shift.float().to(self.device).contiguous()
        else:     # in place: HIP graphs hold these addresses
            self.w.copy_(p); self.scale.copy_(scale.float()); self.shift.copy_(shift.float())

    def out_hw(self, h: int, w: int):
        f = lambda v: (v - 1) * self.k - 2 * self.pad + self.k + self.opad
        return f(h), f(w)

    def uses_amax(self, B: int, h: int, w: int) -> bool:
        return False

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, amax_in=None, amax_out=None) -> torch.Tensor:
        lib = _lib.load()
        x = _f32c(x, "x")
        B, c, h, w = x.shape
        if c != self.cin:
            raise RuntimeError(f"PointwiseUpconv: input has {c} channels, layer expects {self.cin}")
        oh, ow = self.out_hw(h, w)
        if out is None:
            out = torch.empty((B, self.out_c_total, oh, ow), dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != (B, self.out_c_total, oh, ow) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise RuntimeError(f"PointwiseUpconv: out must be a contiguous float32 {(B, self.out_c_total, oh, ow)} tensor in HBM")
        a_out = None
        if amax_out is not None:
            a_out = amax_out.take(lib.lav_upconv_pointwise_parts(B, self.cin, self.cout, h, w, self.k, self.pad, self.opad))
        check(lib.lav_upconv_pointwise(B, self.cin, self.cout, h, w, self.k, self.pad, self.opad, _ptr(x), _ptr(self.w), _ptr(self.scale),
                                       _ptr(self.shift), int(self.relu_pre), self.out_c_total, self.out_c_offset, _ptr(out), _ptr(a_out), _stream()),
              "lav_upconv_pointwise")
        return out


class Conv1dPair:
    """conv(3,1) -> ReLU -> conv(1,3) (+ eval BatchNorm, + residual, ReLU) as ONE lav_conv1d_pair launch: half of ERFNet's
    non_bottleneck_1d block.  `supported(x)` tells whether the row-tile kernel takes this shape."""

    def __init__(self, conv_a, conv_b, bn=None, relu_post=True, device=None):
        lib = _lib.load()
        ch = conv_a.in_channels
        if not (conv_a.kernel_size == (3, 1) and conv_b.kernel_size == (1, 3) and conv_a.out_channels == ch == conv_b.in_channels ==
                conv_b.out_channels and conv_a.stride == (1, 1) and conv_b.stride == (1, 1)
                and conv_a.padding == (conv_a.dilation[0], 0) and conv_b.padding == (0, conv_b.dilation[1])):
            raise RuntimeError("Conv1dPair: expects conv(3,1) then conv(1,3), same channels, stride 1, 'same' padding")
        self.ch, self.da, self.db = ch, conv_a.dilation[0], conv_b.dilation[1]
        dev = device if device is not None else conv_a.weight.device
        nfl = lib.lav_conv1d_pair_packed_weight_floats(ch)
        packed = []
        for conv in (conv_a, conv_b):
            w = conv.weight.detach().to("cpu", torch.float32).reshape(ch, ch, 3).contiguous()
            out = torch.empty(nfl, dtype=torch.float32)
            check(lib.lav_conv1d_pair_pack_weights(ch, w.data_ptr(), out.data_ptr()), "lav_conv1d_pair_pack_weights")
            packed.append(out.to(dev))
        self.wa, self.wb = packed
        self.ba = conv_a.bias.detach().to(dev, torch.float32).contiguous()
        self.bb = conv_b.bias.detach().to(dev, torch.float32).contiguous()
        self.scale = self.shift = None
        if bn is not None:
            self.scale, self.shift = (v.float().to(dev) for v in bn_fold(bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps))
        self.relu_post = bool(relu_post)

    def supported(self, x: torch.Tensor) -> bool:
        w = x.shape[3]
        return (w in (32, 64, 128) and self.ch % 16 == 0 and (self.ch + 31) // 32 <= 128 // w and self.db <= 16
                and _lib.load().lav_conv1d_pair_lds_bytes(self.ch, w, self.db) <= 160 * 1024)

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _f32c(x, "x")
        B, ch, h, w = x.shape
        if ch != self.ch:
            raise RuntimeError(f"Conv1dPair: input has {ch} channels, layer expects {self.ch}")
        if residual is not None:
            residual = _f32c(residual, "residual")
            if residual.shape != x.shape:
                raise RuntimeError("residual shape mismatch")
        y = torch.empty_like(x)
        check(_lib.load().lav_conv1d_pair(B, ch, h, w, self.da, self.db, _ptr(x), _ptr(self.wa), _ptr(self.ba), _ptr(self.wb),
                                          _ptr(self.bb), _ptr(self.scale), _ptr(self.shift), _ptr(residual), int(self.relu_post),
                                          _ptr(y), _stream()), "lav_conv1d_pair")
        return y


class Conv1dPairChain:
    """A run of Conv1dPair layers over one map as ONE persistent launch (lav_conv1d_pair_chain): `pairs` in execution order,
    `residual[i]` True where pair i adds the input of pair i-1 (the non_bottleneck_1d block's input).  Output buffers are kept per
    (batch, h, w) - every pair writes its own, the last one is returned (a fresh tensor per call unless `reuse_out`)."""

    def __init__(self, pairs, residual):
        if len(pairs) != len(residual) or not pairs or residual[0]:
            raise RuntimeError("Conv1dPairChain: one residual flag per pair, the first pair without")
        if any(p.ch != pairs[0].ch or p.scale is None for p in pairs):
            raise RuntimeError("Conv1dPairChain: pairs of one channel count, each with its BatchNorm affine")
        self.pairs, self.residual = list(pairs), [int(bool(r)) for r in residual]
        self._bufs = {}
        # round 6: engines built for LAV_CONV_F16X3 (the inference pipelines' default) run on two fp16 pieces per operand
        # (lav_conv1d_pair_chain_f16); every other precision keeps the bf16x6 run
        self.f16 = infer_precision() == _lib.CONV_F16X3

    def supported(self, x: torch.Tensor) -> bool:
        lib = _lib.load()
        B, ch, h, w = x.shape
        p0 = self.pairs[0]
        lds = lib.lav_conv1d_pair_chain_lds_bytes(p0.ch, w, max(p.db for p in self.pairs))
        return (_os.environ.get("LAV_CONV_PRECISION", "bf16x6") not in ("f32", "fp32") and _os.environ.get("LAV_ERFNET_CHAIN", "1") != "0"
                and len(self.pairs) <= 16 and all(p.supported(x) for p in self.pairs)
                and B * h <= _cu_count(x.device) * (2 if (lds <= 76 * 1024 and not (ch >= 64 and (ch // 16) % 2 == 0)) else 1)
                and lds <= 152 * 1024)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        lib = _lib.load()
        x = _f32c(x, "x")
        B, ch, h, w = x.shape
        n = len(self.pairs)
        key = (B, h, w, x.device, _stream())
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = [torch.empty_like(x) for _ in range(n - 1)]
        out = bufs + [torch.empty_like(x)]
        # sized ONCE for the largest run the chip can hold (2 rows per CU): the buffer never grows, so the sticky time-out / launch
        # counters of already captured graphs stay the ones pair_chain_status() reads
        ws = _workspace("pair_chain", max(lib.lav_conv1d_pair_chain_workspace_bytes(B, h), lib.lav_conv1d_pair_chain_workspace_bytes(pair_chain_capacity(x.device), 1)), x.device)
        ia = lambda vals: (C.c_int * n)(*vals)
        pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        ps = self.pairs
        check((lib.lav_conv1d_pair_chain_f16 if self.f16 else lib.lav_conv1d_pair_chain)(B, ch, h, w, n, ia([p.da for p in ps]), ia([p.db for p in ps]), ia(self.residual),
                                        ia([int(p.relu_post) for p in ps]), _ptr(x), pa([p.wa for p in ps]), pa([p.ba for p in ps]),
                                        pa([p.wb for p in ps]), pa([p.bb for p in ps]), pa([p.scale for p in ps]), pa([p.shift for p in ps]),
                                        pa(out), _ptr(ws), ws.numel(), _stream()), "lav_conv1d_pair_chain")
        return out[-1]

    def timeouts(self, x_like: torch.Tensor) -> int:
        """Workgroups of pair-chain launches on the current stream that gave up waiting for a neighbour row (0 = all results valid)."""
        return pair_chain_status(x_like.device)[0]


def pair_chain_capacity(device) -> int:
    """Rows of progress counters in the pair-chain workspace: room for several runs' regions (pair_chain_region)."""
    return 4 * _cu_count(device)


class pair_chain_region:
    """`with ops.pair_chain_region(row_offset, clean_rows):` - the Conv1dPairChain launches enqueued inside keep their progress counters at
    that offset of the workspace and zero the first `clean_rows` counters first (0: cleaned by an earlier launch; lav_conv1d_pair_chain_region).
    ERFNet's runs use it to share one cleaning launch per forward pass."""

    def __init__(self, row_offset: int, clean_rows: int):
        self.args = (int(row_offset), int(clean_rows))

    def __enter__(self):
        check(_lib.load().lav_conv1d_pair_chain_region(*self.args), "lav_conv1d_pair_chain_region")
        return self

    def __exit__(self, *exc):
        check(_lib.load().lav_conv1d_pair_chain_region(0, -1), "lav_conv1d_pair_chain_region")
        return False


def _device_and_stream(device, stream):
    """`device` with its index filled in and `stream` (default: the current one): what the keys of _workspaces are made of"""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device, stream if stream is not None else torch.cuda.current_stream()


def pair_chain_status(device, stream=None):
    """(workgroups that gave up, launches) of lav_conv1d_pair_chain on `stream` (default: the current one) since its workspace
    was created.  Synchronises that stream."""
    device, st = _device_and_stream(device, stream)
    ws = _workspaces.get(("pair_chain", device, st.cuda_stream))
    if ws is None:
        return (0, 0)
    v = (C.c_int * 2)()
    check(_lib.load().lav_conv1d_pair_chain_status(_ptr(ws), v, st.cuda_stream), "lav_conv1d_pair_chain_status")
    return (int(v[0]), int(v[1]))


def bev_run_stages():
    """The backbone stages (s1, s2, s3) whose same-shape 3x3 layers run as one persistent launch (ConvRun): LAV_BEV_RUN=0 none,
    =1 all, =s1,s3 those; default: what the measurement kept (profiles/bev_run_ab.txt)."""
    v = _os.environ.get("LAV_BEV_RUN", BEV_RUN_DEFAULT).strip().lower()
    if v in ("0", "", "off", "none"):
        return frozenset()
    if v in ("1", "on", "all"):
        return frozenset(("s1", "s2", "s3"))
    return frozenset(s for s in v.split(",") if s in ("s1", "s2", "s3"))


BEV_RUN_DEFAULT = "s2,s3"


class ConvRun:
    """A run of ConvLayers of one geometry - conv3x3(stride 1, pad 1, no bias) -> ReLU -> BatchNorm affine, C -> C channels, packed for
    LAV_CONV_F16X3 - as ONE persistent launch (lav_conv3x3_run_f16).  Reads the layers' own packed weights and epilogue vectors (a
    ConvLayer.refresh re-packs in place: nothing to refresh here).  `takes(B, h, w)`: whether the launch serves that input; else the
    caller runs the layers one by one."""

    def __init__(self, layers):
        lib = _lib.load()
        layers = list(layers)
        l0 = layers[0]
        for l in layers:
            d = l.desc
            if not (d.precision == _lib.CONV_F16X3 and (d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil_h, d.dil_w) == (3, 3, 1, 1, 1, 1, 1)
                    and not d.transposed and l.cin == l.cout == l0.cin and l.in_c_total == l.cin and l.out_c_total == l.cout
                    and l.bias is None and l.scale is not None and d.relu_pre and not d.relu_post and not d.sigmoid and d.pad_value == 0.0):
                raise RuntimeError("ConvRun: layers must be identical conv3x3 / ReLU / BatchNorm layers packed for LAV_CONV_F16X3")
        self.layers, self.ch = layers, l0.cin
        self._woff = int(lib.lav_conv_f16_weights_offset(C.byref(l0._desc())))
        if self._woff < 0 or len(layers) > 8:
            raise RuntimeError("ConvRun: at most 8 layers with fp16 packed weights")
        n = len(layers)
        self._n = n

    def takes(self, B: int, h: int, w: int) -> bool:
        return B == 1 and _lib.load().lav_conv3x3_run_f16_workspace_bytes(self.ch, h, w, self._n) > 0

    def uses_amax(self, B: int, h: int, w: int) -> bool:
        return self.takes(B, h, w)

    _served_by = "lav_conv3x3_run_f16_workspace_bytes"   # (named by the error for an input that takes() refuses)

    def _amax_count(self, lib, ch: int, h: int, w: int) -> int:
        return lib.lav_conv3x3_run_f16_amax_count(ch, h, w)

    def _launch(self, lib, x, w_f16, scale, shift, out, a_in, n_in, a_out):
        ch, h, w = x.shape[1:]
        # one workspace per run, shape AND stream (the maps and the hand-off words are private to the launches of one stream)
        ws = _workspace(("conv_run", id(self), ch, h, w), lib.lav_conv3x3_run_f16_workspace_bytes(ch, h, w, self._n), x.device)
        check(lib.lav_conv3x3_run_f16(ch, h, w, self._n, _ptr(x), w_f16, scale, shift, _ptr(out), _ptr(a_in), n_in, _ptr(a_out), _ptr(ws), ws.numel(),
                                      _stream()), "lav_conv3x3_run_f16")

    def __call__(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, amax_in: Optional["Amax"] = None,
                 amax_out: Optional["Amax"] = None) -> torch.Tensor:
        lib = _lib.load()
        x = _f32c(x, "x")
        B, ch, h, w = x.shape
        if ch != self.ch or not self.takes(B, h, w):
            raise RuntimeError(f"{type(self).__name__}: input {tuple(x.shape)} is not served ({self._served_by})")
        if out is None:
            out = torch.empty_like(x)
        n = self._n
        if amax_in is not None and amax_in.count > 0:
            a_in, n_in = amax_in.buf, amax_in.count
        else:   # nobody left the input's maxima: measure it (one launch more)
            a_in = _workspace(("conv_run_amax", id(self)), 512 * 4, x.device).view(torch.float32)
            n_in = 512
            check(lib.lav_absmax_parts(_ptr(x), x.numel(), _ptr(a_in), _stream()), "lav_absmax_parts")
        a_out = amax_out.take(self._amax_count(lib, ch, h, w)) if amax_out is not None else None
        pa = lambda ts: (C.c_void_p * n)(*[t if isinstance(t, int) else t.data_ptr() for t in ts])
        self._launch(lib, x, pa([l.w.data_ptr() + 4 * self._woff for l in self.layers]), pa([l.scale for l in self.layers]),
                     pa([l.shift for l in self.layers]), out, a_in, n_in, a_out)
        return out


def bev_tile_enabled() -> bool:
    """LAV_BEV_TILE: a 64-channel stage that LAV_BEV_RUN leaves on its per-layer path runs its same-shape 3x3 layers as one launch
    on halo tiles (ConvTileRun); default: what the measurement kept (profiles/bev_tile_ab.txt)."""
    return _os.environ.get("LAV_BEV_TILE", BEV_TILE_DEFAULT).strip().lower() not in ("0", "", "off", "none")


BEV_TILE_DEFAULT = "1"


class ConvTileRun(ConvRun):
    """ConvRun's layers (at most 3, at 64 channels) as ONE launch without hand-off between workgroups (lav_conv3x3_tile_f16): every
    workgroup owns an output tile for all layers, stages the input tile with its halo once and keeps the intermediate maps in LDS.
    The same layer checks, the same calling convention; no workspace and nothing that can time out."""

    _served_by = "lav_conv3x3_tile_f16_lds_bytes"

    def takes(self, B: int, h: int, w: int) -> bool:
        return B == 1 and _lib.load().lav_conv3x3_tile_f16_lds_bytes(self.ch, h, w, self._n) > 0

    def _amax_count(self, lib, ch: int, h: int, w: int) -> int:
        return lib.lav_conv3x3_tile_f16_amax_count(ch, h, w, self._n)

    def _launch(self, lib, x, w_f16, scale, shift, out, a_in, n_in, a_out):
        ch, h, w = x.shape[1:]
        check(lib.lav_conv3x3_tile_f16(ch, h, w, self._n, _ptr(x), w_f16, scale, shift, _ptr(out), _ptr(a_in), n_in, _ptr(a_out), _stream()),
              "lav_conv3x3_tile_f16")


def bev_run_status(device, stream=None):
    """(workgroups that gave up, launches) of the lav_conv3x3_run_f16 launches on `stream` (default: the current one), summed over
    the runs' workspaces.  Synchronises that stream."""
    device, st = _device_and_stream(device, stream)
    tot = [0, 0]
    for (key, dev, s), ws in list(_workspaces.items()):
        if isinstance(key, tuple) and key and key[0] == "conv_run" and dev == device and s == st.cuda_stream:
            v = (C.c_int * 2)()
            check(_lib.load().lav_conv3x3_run_f16_status(_ptr(ws), v, st.cuda_stream), "lav_conv3x3_run_f16_status")
            tot[0] += int(v[0]); tot[1] += int(v[1])
    return tuple(tot)


_CU_COUNT = {}


def _cu_count(device) -> int:
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _CU_COUNT[idx]


# algorithmic work of the training-side kernels since the last reset (bench.py's training roofline reads it next to the
# library's HIP-event timers): bytes the crop gradient must move, flops of the recurrent GEMMs
train_work = {"crop_rotate_backward_bytes": 0, "crop_rotate_backward_calls": 0, "gru_seq_forward_flops": 0, "gru_seq_backward_flops": 0,
              "bn_train_fwd_bytes": 0, "bn_train_bwd_bytes": 0, "conv_wgrad_flops": 0}


def _crop_args(features, locs, oris, crop):
    """The tensors both crop entry points pass on, and their output: features (M,C,H,W), locs (n,2), oris (n,), out (n,C,crop,crop)."""
    features = _f32c(features, "features")
    locs, oris = _f32c(locs.detach().reshape(-1, 2), "locs"), _f32c(oris.detach().reshape(-1), "oris")
    out = torch.empty((locs.shape[0], features.shape[1], crop, crop), dtype=torch.float32, device=features.device)
    return features, locs, oris, out


class _CropRotateIndexed(torch.autograd.Function):
    """Rotated crops taken from per-sample feature maps by index, differentiable in the maps (training path)."""

    @staticmethod
    def forward(ctx, features, map_index, locs, oris, ppm, crop, ox, oy):
        lib = _lib.load()
        features, locs, oris, out = _crop_args(features, locs, oris, crop)
        if map_index.dtype != torch.int32 or not map_index.is_cuda:
            raise RuntimeError("crop_rotate_indexed: map_index must be an int32 tensor in HBM")
        M, Cc, H, W = features.shape
        n = locs.shape[0]
        check(lib.lav_crop_rotate_indexed(_ptr(features), M, _ptr(map_index), Cc, H, W, _ptr(locs), _ptr(oris), n, float(ppm), int(crop),
                                          float(ox), float(oy), _ptr(out), _stream()), "lav_crop_rotate_indexed")
        ctx.save_for_backward(map_index, locs, oris)
        ctx.geom = (M, Cc, H, W, float(ppm), int(crop), float(ox), float(oy))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        map_index, locs, oris = ctx.saved_tensors
        M, Cc, H, W, ppm, crop, ox, oy = ctx.geom
        grad_out = _f32c(grad_out, "grad_out")
        grad_feat = torch.empty((M, Cc, H, W), dtype=torch.float32, device=grad_out.device)
        train_work["crop_rotate_backward_bytes"] += 4 * (grad_out.numel() + grad_feat.numel())     # read every output gradient once, write the map gradient once
        train_work["crop_rotate_backward_calls"] += 1
        check(_lib.load().lav_crop_rotate_backward(_ptr(grad_out), M, _ptr(map_index), Cc, H, W, _ptr(locs), _ptr(oris), locs.shape[0], ppm,
                                                   crop, ox, oy, _ptr(grad_feat), _stream()), "lav_crop_rotate_backward")
        return grad_feat, None, None, None, None, None, None, None


def crop_rotate_indexed(features, map_index, locs, oris, pixels_per_meter, crop, offset_x, offset_y):
    """features (M,C,H,W); crop i = rotated crop of features[map_index[i]] at (locs[i], oris[i]) -> (n,C,crop,crop)."""
    return _CropRotateIndexed.apply(features, map_index, locs, oris, pixels_per_meter, crop, offset_x, offset_y)


def det_decode(rows: torch.Tensor, actors: torch.Tensor, n_out: torch.Tensor, *, cls: int, min_score: float, ego_xy, near_px: float,
               far_px: float, min_box: float, centre_xy, skip_px: float, ppm: float, report=None):
    """Peak rows (ncls, max_det, 7) of lav_extract_peaks -> the other vehicles' ego-frame (x, y) and headings in `actors`
    ([2*max_det] + [max_det] floats) and their number in `n_out` (int32[1]), all in HBM (lav_det_decode).
    report = (host_rows float32 like rows, host_n int32[1], host_seq int32[1]), three PINNED host tensors: the launch also writes rows
    and count there and then increments host_seq (lav_det_decode_report) - the host polls the word instead of copying."""
    rows = _f32c(rows, "rows")
    ncls, max_det, _ = rows.shape
    if actors.numel() < 3 * max_det or actors.dtype != torch.float32 or n_out.dtype != torch.int32:
        raise RuntimeError("det_decode: actors must hold 3*max_det float32, n_out one int32")
    host = [None, None, None]
    if report is not None:
        h_rows, h_n, h_seq = report
        if not (h_rows.is_pinned() and h_n.is_pinned() and h_seq.is_pinned() and h_rows.is_contiguous()) or h_rows.dtype != torch.float32 \
                or h_rows.numel() < rows.numel() or h_n.dtype != torch.int32 or h_seq.dtype != torch.int32:
            raise RuntimeError("det_decode: report = (pinned float32 rows, pinned int32[1] count, pinned int32[1] sequence word)")
        host = [h_rows.data_ptr(), h_n.data_ptr(), h_seq.data_ptr()]
    check(_lib.load().lav_det_decode_report(_ptr(rows), ncls, max_det, int(cls), float(min_score), float(ego_xy[0]), float(ego_xy[1]),
                                            float(near_px), float(far_px), float(min_box), float(centre_xy[0]), float(centre_xy[1]),
                                            float(skip_px), float(ppm), _ptr(actors), _ptr(n_out), *host, _stream()), "lav_det_decode")


class batch_limit:
    """`with ops.batch_limit(d_n):` - the conv / crop / cast launches enqueued inside skip the rows >= d_n[0], a count that
    lives in HBM and is read when the kernels run (lav_batch_limit)."""

    def __init__(self, d_rows: torch.Tensor):
        if d_rows.dtype != torch.int32 or not d_rows.is_cuda:
            raise RuntimeError("batch_limit: an int32 tensor in HBM")
        self.d_rows = d_rows

    def __enter__(self):
        check(_lib.load().lav_batch_limit(_ptr(self.d_rows)), "lav_batch_limit")
        return self

    def __exit__(self, *exc):
        check(_lib.load().lav_batch_limit(None), "lav_batch_limit")
        return False


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    """F.max_pool2d(x, 3, 2, 1) on liblav_amd (lav_maxpool3x3s2); honours batch_limit."""
    x = _f32c(x, "x")
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    check(_lib.load().lav_maxpool3x3s2(_ptr(x), B, Cc, H, W, _ptr(out), _stream()), "lav_maxpool3x3s2")
    return out


def channel_affine(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """x (B,C,H,W) * scale[c] + shift[c] in one launch (lav_channel_affine); H*W must be a multiple of 4."""
    x = _f32c(x, "x")
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    check(_lib.load().lav_channel_affine(_ptr(x), B, Cc, H * W, _ptr(_f32c(scale, "scale")), _ptr(_f32c(shift, "shift")), _ptr(out), _stream()),
          "lav_channel_affine")
    return out


def nonfinite_count(tensors, counter: torch.Tensor) -> None:
    """counter (2,) int32 in HBM: [0] += number of `tensors` (float32, contiguous, <= 8) holding a NaN / Inf, [1] += 1.
    One launch, no host sync (include/lav_amd.h: lav_nonfinite_count)."""
    ts = [_f32c(t, "tensor") for t in tensors]
    n = len(ts)
    if counter.dtype != torch.int32 or counter.numel() < 2 or not counter.is_cuda:
        raise RuntimeError("nonfinite_count: counter must be an int32 tensor of two elements in HBM")
    check(_lib.load().lav_nonfinite_count(n, (C.c_void_p * n)(*[t.data_ptr() for t in ts]), (C.c_long * n)(*[t.numel() for t in ts]),
                                          _ptr(counter), _stream()), "lav_nonfinite_count")


def _optim_args(op, table, ntensors, chunks, watch, nwatch, watch_chunks, words):
    """The checked arguments the two lav_optim_* calls share: uint8 tables in HBM long enough for their row counts, the workspace."""
    from .train import optim as O
    dev = words["global"].device
    sizes = [(table, ntensors * O.TENSOR_DTYPE.itemsize, "table"), (watch, nwatch * O.WATCH_DTYPE.itemsize, "watch"),
             (words["global"], O.GLOBAL_DTYPE.itemsize, "global")]
    if "state" in words:        # (a row per tensor of the table at the least; the rows' own indices are the caller's)
        sizes.append((words["state"], ntensors * O.STATE_DTYPE.itemsize, "state"))
    for t, nbytes, name in sizes:
        if t is None and nbytes == 0:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= nbytes
                and (t.numel() == 0 or t.data_ptr() % 8 == 0)):
            raise ValueError(f"{op}: {name} must be a contiguous, 8-byte aligned uint8 tensor of at least {nbytes} bytes in HBM, on one device")
    lib = _lib.load()
    nbytes = int(lib.lav_optim_workspace_bytes(int(chunks), int(watch_chunks)))
    if nbytes == 0:
        raise ValueError(f"{op}: {chunks} + {watch_chunks} chunks")
    return lib, _workspace(("optim",), nbytes, dev), nbytes


def optim_grad_stats(table, ntensors, chunks, watch, nwatch, watch_chunks, glob, max_norm=None) -> None:
    """The statistics half of optim_adam_step alone (lav_optim_grad_stats: two launches on the current stream): writes nonfinite, sumsq,
    clip, apply and watch_nonfinite of `glob`; the counters, the tensors and their words are not touched."""
    lib, ws, nbytes = _optim_args("optim_grad_stats", table, ntensors, chunks, watch, nwatch, watch_chunks, dict(**{"global": glob}))
    check(lib.lav_optim_grad_stats(_ptr(table), int(ntensors), int(chunks), _ptr(watch), int(nwatch), int(watch_chunks), _ptr(glob),
                                   float(max_norm or 0.0), _ptr(ws), nbytes, _stream()), "lav_optim_grad_stats")


def optim_adam_step(table, ntensors, chunks, watch, nwatch, watch_chunks, state, glob, max_norm=None) -> None:
    """One guarded Adam step over every tensor of a descriptor table (lav_optim_adam_step: three launches on the current stream, no
    synchronisation).  table / watch / state / glob: uint8 tensors in HBM holding rows of lav_amd.train.optim's TENSOR_DTYPE /
    WATCH_DTYPE / STATE_DTYPE / GLOBAL_DTYPE (include/lav_amd.h's structs); chunks / watch_chunks: what fill_chunks returned for them.
    The library trusts the rows: lav_amd.train.optim.FusedAdam builds them from live tensors.  Equal to fused_adam_numpy in every bit."""
    lib, ws, nbytes = _optim_args("optim_adam_step", table, ntensors, chunks, watch, nwatch, watch_chunks, dict(state=state, **{"global": glob}))
    check(lib.lav_optim_adam_step(_ptr(table), int(ntensors), int(chunks), _ptr(watch), int(nwatch), int(watch_chunks), _ptr(state), _ptr(glob),
                                  float(max_norm or 0.0), _ptr(ws), nbytes, _stream()), "lav_optim_adam_step")


def optim_adam_ema_step(table, ntensors, chunks, watch, nwatch, watch_chunks, state, glob, shadow, ema_decay, max_norm=None) -> None:
    """optim_adam_step whose update launch also moves a shadow of every tensor towards its new parameter (lav_optim_adam_ema_step: the
    same three launches).  shadow: a uint8 tensor in HBM holding `ntensors` device pointers (little-endian uint64), row-parallel to
    `table`, to dense float32 tensors of the rows' sizes; ema_decay: 0 < decay < 1.  Equal to fused_adam_numpy(..., ema_decay=) in every
    bit; p, m, v and the words get optim_adam_step's bits."""
    lib, ws, nbytes = _optim_args("optim_adam_ema_step", table, ntensors, chunks, watch, nwatch, watch_chunks, dict(state=state, **{"global": glob}))
    if not (isinstance(shadow, torch.Tensor) and shadow.is_cuda and shadow.device == glob.device and shadow.dtype == torch.uint8
            and shadow.is_contiguous() and shadow.numel() >= 8 * int(ntensors) and (shadow.numel() == 0 or shadow.data_ptr() % 8 == 0)):
        raise ValueError(f"optim_adam_ema_step: shadow must be a contiguous, 8-byte aligned uint8 tensor of at least {8 * int(ntensors)} bytes in HBM")
    check(lib.lav_optim_adam_ema_step(_ptr(table), int(ntensors), int(chunks), _ptr(watch), int(nwatch), int(watch_chunks), _ptr(state), _ptr(glob),
                                      float(max_norm or 0.0), _ptr(shadow), float(ema_decay), _ptr(ws), nbytes, _stream()), "lav_optim_adam_ema_step")


def optim_tensor_stats(table, ntensors, chunks, watch, nwatch, watch_chunks, state, rows_out, watch_out) -> None:
    """The per-tensor view of a step (lav_optim_tensor_stats: two launches on the current stream, no synchronisation) over the tables
    and state words an optim_adam_step ran on: rows_out / watch_out, uint8 tensors in HBM, receive one lav_amd.train.optim
    TENSOR_ROW_DTYPE row per tensor and one WATCH_ROW_DTYPE row per watched buffer.  Reads g, p, m, v and the words; stores into none
    of them.  Equal to tensor_stats_numpy in every integer, bin and maximum; the sums of squares within numel * 2^-53 relative."""
    from .train import optim as O
    dev = rows_out.device
    for t, nbytes, name in ((table, ntensors * O.TENSOR_DTYPE.itemsize, "table"), (watch, nwatch * O.WATCH_DTYPE.itemsize, "watch"),
                            (state, ntensors * O.STATE_DTYPE.itemsize, "state"), (rows_out, ntensors * O.TENSOR_ROW_DTYPE.itemsize, "rows_out"),
                            (watch_out, nwatch * O.WATCH_ROW_DTYPE.itemsize, "watch_out")):
        if t is None and nbytes == 0:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= nbytes
                and (t.numel() == 0 or t.data_ptr() % 8 == 0)):
            raise ValueError(f"optim_tensor_stats: {name} must be a contiguous, 8-byte aligned uint8 tensor of at least {nbytes} bytes in HBM, on one device")
    lib = _lib.load()
    nbytes = int(lib.lav_optim_tensor_stats_workspace_bytes(int(chunks), int(watch_chunks)))
    if nbytes == 0:
        raise ValueError(f"optim_tensor_stats: {chunks} + {watch_chunks} chunks")
    ws = _workspace(("optim_tensor_stats",), nbytes, dev)
    check(lib.lav_optim_tensor_stats(_ptr(table), int(ntensors), int(chunks), _ptr(watch), int(nwatch), int(watch_chunks), _ptr(state),
                                     _ptr(rows_out), _ptr(watch_out), _ptr(ws), nbytes, _stream()), "lav_optim_tensor_stats")


def optim_blame(table, ntensors, chunks, watch, nwatch, watch_chunks, glob, blame) -> None:
    """Who caused a skipped step (lav_optim_blame: one workgroup on the current stream, behind the optim_adam_step / optim_adam_ema_step
    with these tables whose per-chunk counts it reads in their workspace).  blame: a uint8 tensor in HBM holding one
    lav_amd.train.optim BLAME_DTYPE block, zeroed by the caller once.  When that step was applied nothing is written.  Equal to
    blame_numpy in every word."""
    from .train import optim as O
    lib, ws, nbytes = _optim_args("optim_blame", table, ntensors, chunks, watch, nwatch, watch_chunks, dict(**{"global": glob}))
    if not (isinstance(blame, torch.Tensor) and blame.is_cuda and blame.device == glob.device and blame.dtype == torch.uint8 and blame.is_contiguous()
            and blame.numel() >= O.BLAME_DTYPE.itemsize and blame.data_ptr() % 8 == 0):
        raise ValueError(f"optim_blame: blame must be a contiguous, 8-byte aligned uint8 tensor of at least {O.BLAME_DTYPE.itemsize} bytes in HBM")
    check(lib.lav_optim_blame(_ptr(table), int(ntensors), int(chunks), _ptr(watch), int(nwatch), int(watch_chunks), _ptr(glob), _ptr(blame),
                              _ptr(ws), nbytes, _stream()), "lav_optim_blame")


def copy_many(pairs, block=None) -> None:
    """[(dst, src), ...] device tensors of equal shape into their destinations in at most two launches: contiguous same-dtype
    16-byte-aligned pairs through lav_copy_many (16-byte words), strided / uint8 sources of up to four dimensions into contiguous
    float32 destinations through lav_stage_many (the conversion torch's copy_ would do, for all of them at once); anything else
    takes Tensor.copy_.
    block = (dst device tensor, src HOST tensor of the same <= 256 bytes, a multiple of 4): rides in the staging launch's kernel
    arguments (lav_stage_many_block) instead of an upload of its own; copied with Tensor.copy_ when there is no such launch."""
    srcs, dsts, sizes, stage, plain = [], [], [], [], []
    for dst, src in pairs:
        nb = dst.numel() * dst.element_size()
        both = src.is_cuda and dst.is_cuda and dst.is_contiguous() and src.shape == dst.shape and nb > 0
        if (both and src.is_contiguous() and src.dtype == dst.dtype and nb % 4 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0):
            srcs.append(src.data_ptr()); dsts.append(dst.data_ptr()); sizes.append(nb); plain.append((dst, src))
        elif both and dst.dtype == torch.float32 and src.dtype in (torch.float32, torch.uint8) and 1 <= src.dim() <= 4:
            stage.append((dst, src))
        else:
            dst.copy_(src, non_blocking=True)
    lib = _lib.load()
    if stage and plain and len(stage) + len(plain) <= 8 and all(d.dtype == torch.float32 for d, _ in plain):
        # (round 6) one launch instead of two: the few contiguous float32 pairs of a frame (LiDAR rows, next waypoint) ride with the
        # strided ones - every launch on the frame's critical chain costs ~4.5 us whatever it moves
        stage = [(d.reshape(-1), s_.reshape(-1)) for d, s_ in plain] + stage
        srcs = []
    for i in range(0, len(srcs), 8):
        n = len(srcs[i:i + 8])
        check(lib.lav_copy_many(n, (C.c_void_p * n)(*srcs[i:i + 8]), (C.c_void_p * n)(*dsts[i:i + 8]), (C.c_size_t * n)(*sizes[i:i + 8]), _stream()),
              "lav_copy_many")
    blk = (None, 0, None)
    if block is not None:
        bdst, bsrc = block
        nb = bsrc.numel() * bsrc.element_size()
        if (stage and not bsrc.is_cuda and bsrc.is_contiguous() and bdst.is_cuda and bdst.is_contiguous() and nb % 4 == 0 and 0 < nb <= 256
                and nb == bdst.numel() * bdst.element_size() and bdst.data_ptr() % 4 == 0):
            blk = (bsrc.data_ptr(), nb, bdst.data_ptr())
        else:
            bdst.copy_(bsrc, non_blocking=True)
    for i in range(0, len(stage), 8):
        part = stage[i:i + 8]
        n = len(part)
        dims, strides = [], []
        for dst, src in part:
            pad = 4 - src.dim()
            dims += [1] * pad + list(src.shape)
            strides += [0] * pad + list(src.stride())
        b = blk if i == 0 else (None, 0, None)
        check(lib.lav_stage_many_block(n, (C.c_void_p * n)(*[s_.data_ptr() for _, s_ in part]), (C.c_void_p * n)(*[d.data_ptr() for d, _ in part]),
                                       (C.c_int * (4 * n))(*dims), (C.c_long * (4 * n))(*strides),
                                       (C.c_int * n)(*[int(s_.dtype == torch.uint8) for _, s_ in part]), b[0], b[1], b[2], _stream()), "lav_stage_many")


def linear_act(x: torch.Tensor, weight: torch.Tensor, bias, sigmoid: bool = False) -> torch.Tensor:
    """act(x @ weight.T + bias) for small layers, x (B,K) in HBM, weight (O,K) (lav_linear_act)."""
    x = _f32c(x, "x")
    B, K = x.shape
    O = weight.shape[0]
    out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    check(_lib.load().lav_linear_act(_ptr(x), B, K, _ptr(_f32c(weight, "weight")), _ptr(None if bias is None else _f32c(bias, "bias")), O,
                                     int(bool(sigmoid)), _ptr(out), _stream()), "lav_linear_act")
    return out


def attn_pool(x: torch.Tensor, u: torch.Tensor, dots_bias: torch.Tensor, w_v: torch.Tensor, b_v: torch.Tensor, heads: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B,C,h,w) in HBM -> (B,C): single-query multi-head attention pooling with folded projections (lav_attn_pool).
    out: a (B,C) buffer whose rows are C apart (e.g. one half of a (1,2C) concatenation buffer at batch 1)."""
    x = _f32c(x, "x")
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, Cc) or out.dtype != torch.float32 or not out.is_cuda or (B > 1 and out.stride(0) != Cc) or out.stride(1) != 1:
        raise RuntimeError("attn_pool: out must be a (B, C) float32 buffer in HBM with rows C apart")
    check(_lib.load().lav_attn_pool(_ptr(x), B, Cc, H * W, int(heads), _ptr(_f32c(u, "u")), _ptr(_f32c(dots_bias, "dots_bias")),
                                    _ptr(_f32c(w_v, "w_v")), _ptr(_f32c(b_v, "b_v")), _ptr(out), _stream()), "lav_attn_pool")
    return out


def pool_affine(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, out: torch.Tensor, out_c_offset: int, relu: bool = True):
    """2x2 max pooling + per-channel affine (+ ReLU) of x (B,C,H,W) into channels [out_c_offset, +C) of out (B,Ct,H/2,W/2)."""
    x = _f32c(x, "x")
    B, Cc, H, W = x.shape
    if out.shape[0] != B or out.shape[2:] != (H // 2, W // 2) or not out.is_contiguous():
        raise RuntimeError("pool_affine: output buffer does not match")
    check(_lib.load().lav_pool_affine(_ptr(x), B, Cc, H, W, _ptr(_f32c(scale, "scale")), _ptr(_f32c(shift, "shift")), int(relu),
                                      _ptr(out), out.shape[1], int(out_c_offset), _stream()), "lav_pool_affine")
    return out


def erfnet_entry_takes(x: torch.Tensor) -> bool:
    """Whether lav_erfnet_entry serves x as it lies in memory: (B, 3, H, W) float32, contiguous, H and W multiples of 4."""
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == 3 and 1 <= x.shape[0] <= 65535
            and x.shape[2] >= 4 and x.shape[3] >= 4 and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0 and x.shape[2] <= 8 * 4 * 65535)


def erfnet_entry(x: torch.Tensor, w1, b1, pad_value: float, scale1, shift1, w2, b2, scale2, shift2, out: Optional[torch.Tensor] = None):
    """ERFNet's two entry DownsamplerBlocks on the raw input x (B,3,H,W) as one launch -> (B,64,H/4,W/4); the parameters as
    include/lav_amd.h describes them (lav_erfnet_entry)."""
    if not erfnet_entry_takes(x):
        raise RuntimeError(f"erfnet_entry: input {tuple(x.shape)} is not served (contiguous float32 (B,3,H,W) with H, W multiples of 4)")
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty((B, 64, H // 4, W // 4), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, 64, H // 4, W // 4) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise RuntimeError("erfnet_entry: output buffer does not match")
    vec = [("w1", w1, 13 * 27), ("b1", b1, 13), ("scale1", scale1, 16), ("shift1", shift1, 16), ("w2", w2, 48 * 144), ("b2", b2, 48),
           ("scale2", scale2, 64), ("shift2", shift2, 64)]
    ptrs = {}
    for name, t, n in vec:
        if t.numel() != n or t.device != x.device:
            raise RuntimeError(f"erfnet_entry: {name} must hold {n} floats on {x.device}")
        ptrs[name] = _ptr(_f32c(t, name))
    check(_lib.load().lav_erfnet_entry(_ptr(x), B, H, W, ptrs["w1"], ptrs["b1"], float(pad_value), ptrs["scale1"], ptrs["shift1"], ptrs["w2"],
                                       ptrs["b2"], ptrs["scale2"], ptrs["shift2"], _ptr(out), _stream()), "lav_erfnet_entry")
    return out


def crop_rotate(features: torch.Tensor, locs: torch.Tensor, oris: torch.Tensor, pixels_per_meter: float, crop: int,
                offset_x: float, offset_y: float) -> torch.Tensor:
    """features (1 or N, C, H, W), locs (N,2), oris (N,) in HBM -> (N, C, crop, crop)."""
    lib = _lib.load()
    features, locs, oris, out = _crop_args(features, locs, oris, crop)
    fb, Cc, H, W = features.shape
    n = locs.shape[0]
    if fb not in (1, n):
        raise RuntimeError("features batch must be 1 (shared map) or N")
    check(lib.lav_crop_rotate(_ptr(features), fb, Cc, H, W, _ptr(locs), _ptr(oris), n, float(pixels_per_meter), int(crop),
                              float(offset_x), float(offset_y), _ptr(out), _stream()), "lav_crop_rotate")
    return out


def merge_ticks(tick: torch.Tensor, prev: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """cat([tick, prev]) with ego-box points marked x = NaN; then prev <- tick, in place.  tick, prev (P,4)."""
    lib = _lib.load()
    tick, prev = _f32c(tick, "tick"), _f32c(prev, "prev")
    if tick.shape != prev.shape or tick.dim() != 2 or tick.shape[1] != 4:
        raise RuntimeError(f"merge_ticks: tick {tuple(tick.shape)} / prev {tuple(prev.shape)} must both be (P, 4)")
    P = tick.shape[0]
    if out is None:
        out = torch.empty((2 * P, 4), dtype=torch.float32, device=tick.device)
    check(lib.lav_merge_ticks(_ptr(tick), _ptr(prev), P, 4, _ptr(out), _stream()), "lav_merge_ticks")
    return out


def stack_sweeps(fused: torch.Tensor, ring: torch.Tensor, slot: torch.Tensor, sweeps: torch.Tensor, R: torch.Tensor,
                 t: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """History write + temporal stacking: fused (rows,8), ring (slots,rows,8), slot (1,) int64, sweeps (S,) int64,
    R (S,3,3), t (S,3) - all in HBM -> (S*rows, 8+S)."""
    lib = _lib.load()
    fused, ring, R, t = _f32c(fused, "fused"), _f32c(ring, "ring"), _f32c(R, "R"), _f32c(t.reshape(-1, 3), "t")
    S, rows, dim = sweeps.numel(), fused.shape[0], fused.shape[1]
    if ring.shape[1:] != fused.shape or slot.dtype != torch.long or sweeps.dtype != torch.long or R.shape != (S, 3, 3):
        raise RuntimeError("stack_sweeps: inconsistent arguments")
    if out is None:
        out = torch.empty((S * rows, dim + S), dtype=torch.float32, device=fused.device)
    check(lib.lav_stack_sweeps(_ptr(fused), _ptr(ring), _ptr(slot), _ptr(sweeps), _ptr(R), _ptr(t), S, rows, dim, _ptr(out),
                               _stream()), "lav_stack_sweeps")
    return out


def extract_peaks(heat: torch.Tensor, size: Optional[torch.Tensor] = None, ori: Optional[torch.Tensor] = None, ks: int = 7,
                  max_det: int = 15, apply_sigmoid: bool = False) -> torch.Tensor:
    """heat (ncls,H,W), size (cs,H,W), ori (co,H,W) -> (ncls, max_det, 3+cs+co) rows (score, x, y, size.., ori..).  size / ori None:
    no gathered columns (size_c = ori_c = 0) - the (score, x, y) rows HeadsAtPeaks takes."""
    lib = _lib.load()
    heat = _f32c(heat, "heat")
    size, ori = (None if size is None else _f32c(size, "size")), (None if ori is None else _f32c(ori, "ori"))
    ncls, H, W = heat.shape
    if any(m is not None and m.shape[1:] != (H, W) for m in (size, ori)):
        raise RuntimeError("extract_peaks: size / ori maps must match the heat map")
    cs, co = (0 if size is None else size.shape[0]), (0 if ori is None else ori.shape[0])
    out = torch.empty((ncls, max_det, 3 + cs + co), dtype=torch.float32, device=heat.device)
    nbytes = lib.lav_extract_peaks_workspace_bytes(ncls, H, W)
    ws = _workspace("peaks", nbytes, heat.device)
    check(lib.lav_extract_peaks(_ptr(heat), ncls, H, W, ks, max_det, int(apply_sigmoid), _ptr(size), cs, _ptr(ori), co, _ptr(out),
                                _ptr(ws), ws.numel(), _stream()), "lav_extract_peaks")
    return out


class HeadsAtPeaks:
    """Heads conv3x3(cin -> hidden <= 64) -> ReLU -> eval BatchNorm -> ConvTranspose2d(hidden -> outs <= 4, 3, 2, 1, 1) evaluated at
    peak rows only, as ONE lav_heads_at_peaks launch: `heads` is a list of (conv, bn, deconv) modules (1 .. 4 of them).  The first
    convolutions' weights are re-laid-out once, here, as [9 cin rounded up to 128][64] for the kernel's contiguous stream; refresh()
    re-reads every parameter into the same buffers (captured graphs hold their addresses).  __call__(feat (cin,H,W), rows
    (ncls,max_det,3)) -> (ncls, max_det, 3 + sum(outs))."""

    def __init__(self, heads, device=None):
        lib = _lib.load()
        self._heads = [tuple(h) for h in heads]
        conv0, _, ct0 = self._heads[0]
        if not 1 <= len(self._heads) <= 4:
            raise RuntimeError("HeadsAtPeaks: 1 .. 4 heads")
        for conv, bn, ct in self._heads:
            if (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, conv.in_channels) != ((3, 3), (1, 1), (1, 1), (1, 1), 1, conv0.in_channels) \
                    or conv.bias is not None or conv.padding_mode != "zeros":
                raise RuntimeError("HeadsAtPeaks: first layer must be Conv2d(cin, hidden, 3, 1, 1, bias=False)")
            if (ct.kernel_size, ct.stride, ct.padding, ct.output_padding, ct.dilation, ct.groups, ct.in_channels) != \
                    ((3, 3), (2, 2), (1, 1), (1, 1), (1, 1), 1, conv.out_channels) or bn.num_features != conv.out_channels:
                raise RuntimeError("HeadsAtPeaks: tail must be ConvTranspose2d(hidden, outs, 3, 2, 1, 1) behind a BatchNorm2d(hidden)")
        self._dev = device if device is not None else conv0.weight.device
        self.cin = conv0.in_channels
        self.hidden = [conv.out_channels for conv, _, _ in self._heads]
        self.outs = [ct.out_channels for _, _, ct in self._heads]
        n = [lib.lav_heads_at_peaks_packed_floats(self.cin, h) for h in self.hidden]
        if not all(n) or max(self.outs) > 4:
            raise RuntimeError("HeadsAtPeaks: hidden width <= 64 and at most 4 outputs per head")
        f = dict(dtype=torch.float32, device=self._dev)
        self.w1 = [torch.zeros((k // 64, 64), **f) for k in n]
        self.scale = [torch.empty((h,), **f) for h in self.hidden]
        self.shift = [torch.empty((h,), **f) for h in self.hidden]
        self.wt = [torch.empty((h, o, 3, 3), **f) for h, o in zip(self.hidden, self.outs)]
        self.bias = [None if ct.bias is None else torch.empty((o,), **f) for (_, _, ct), o in zip(self._heads, self.outs)]
        self.refresh()
        G = len(self._heads)
        arr = lambda ts: (C.c_void_p * G)(*[_ptr(t) for t in ts])
        self._args = (arr(self.w1), arr(self.scale), arr(self.shift), arr(self.wt), arr(self.bias), (C.c_int * G)(*self.hidden),
                      (C.c_int * G)(*self.outs))

    def refresh(self):
        """(Re-)read the modules' parameters, in place."""
        for g, (conv, bn, ct) in enumerate(self._heads):
            hid = self.hidden[g]
            w = conv.weight.detach().to(self._dev, torch.float32)                        # (hidden, cin, 3, 3) -> [ci * 9 + tap][hidden]
            self.w1[g][:9 * self.cin, :hid].copy_(w.permute(1, 2, 3, 0).reshape(9 * self.cin, hid))
            scale, shift = bn_fold(*[t.detach().cpu() for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias)], bn.eps)
            self.scale[g].copy_(scale.to(torch.float32))
            self.shift[g].copy_(shift.to(torch.float32))
            self.wt[g].copy_(ct.weight.detach())
            if self.bias[g] is not None:
                self.bias[g].copy_(ct.bias.detach())

    def __call__(self, feat: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        feat, rows = _f32c(feat, "feat"), _f32c(rows, "rows")
        if feat.dim() != 3 or feat.shape[0] != self.cin or rows.dim() != 3 or rows.shape[2] != 3:
            raise RuntimeError(f"heads_at_peaks: feature map (cin = {self.cin}, H, W) and rows (ncls, max_det, 3) expected")
        ncls, max_det = rows.shape[:2]
        shape = (ncls, max_det, 3 + sum(self.outs))
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=feat.device)
        elif tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != torch.float32:
            raise RuntimeError(f"heads_at_peaks: output buffer must be contiguous float32 {shape}")
        check(_lib.load().lav_heads_at_peaks(_ptr(feat), self.cin, feat.shape[1], feat.shape[2], _ptr(rows), ncls, max_det,
                                            len(self._heads), *self._args, _ptr(out), _stream()), "lav_heads_at_peaks")
        return out


def heads_at_peaks(layer: HeadsAtPeaks, feat: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """Function form of HeadsAtPeaks.__call__ (one lav_heads_at_peaks launch)."""
    return layer(feat, rows)
