"""lav_heads_at_peaks: the box / orientation heads at the peak rows only (LiDARModel.detect) against float64 of the module's own layers
(tests/heads_peaks_util.py; that reference is checked against the parity rule by tests/test_heads_peaks_host.py), against the dense
path it replaces, and the LAV_HEADS_AT_PEAKS knob of the frame.

Bars.  Every value: |error| <= 2e-6 * sum|a||b| of its hidden dot products, carried through the tail's weights (the bar
tests/test_gpu_conv_run.py applies).  Over all rows: the maximum error is not larger than that of the dense path at LAV_CONV_F16X3 (the
fused first convolution + the grouped transposed convolution, gathered at the same rows) against the same float64 values."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lav_amd import _lib, ops
from tests import heads_peaks_util as hp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_path(feat, heads, precision):
    """The maps of the path lav_heads_at_peaks replaces: ONE first convolution over the heads' concatenated weights at `precision`
    and ONE grouped transposed convolution (LiDARModel._head_engine's layers) -> list of (outs, 2H, 2W) float64 arrays."""
    w = torch.cat([h[0].weight.detach() for h in heads])
    bn = tuple(torch.cat([getattr(h[1], n).detach() for h in heads]) for n in ("running_mean", "running_var", "weight", "bias"))
    conv = ops.ConvLayer(w, padding=1, bn=bn, bn_eps=heads[0][1].eps, relu_pre=True, device=DEV, precision=precision)
    deconv = ops.GroupedDeconv([h[2] for h in heads], device=DEV)
    y = deconv(conv(feat[None].to(DEV)))[0].double().cpu().numpy()
    outs = np.cumsum([0] + [h[2].out_channels for h in heads])
    return [y[a:b] for a, b in zip(outs[:-1], outs[1:])]


@pytest.mark.parametrize("cin,H,W,hidden,outs", [(20, 5, 7, 8, (2, 2)), (384, 4, 6, 64, (1, 3)), (20, 5, 7, 64, (1, 3)), (384, 4, 6, 8, (2, 2))])
def test_kernel_against_float64(cin, H, W, hidden, outs):
    feat = torch.randn((cin, H, W), generator=torch.Generator().manual_seed(cin + hidden))
    heads = [hp.make_head(cin, hidden, o, 10 * g + o) for g, o in enumerate(outs)]
    rows, bad = hp.hand_rows(H, W)
    refs = [hp.dense_reference(feat, h) for h in heads]
    want = hp.gather(rows, [v.numpy() for v, _ in refs], H, W)
    bound = hp.gather(rows, [b.numpy() for _, b in refs], H, W)
    layer = ops.HeadsAtPeaks(heads, device=DEV)
    d_rows = torch.from_numpy(rows).to(DEV)
    out = layer(feat.to(DEV), d_rows)
    got = out.cpu().numpy()
    assert got.shape == (2, 15, 3 + sum(outs))
    assert np.array_equal(got[..., :3].view(np.uint32), rows.view(np.uint32)), "columns 0..2 are copied bit for bit (NaN included)"
    for c, d in bad:
        assert not got[c, d, 3:].any(), f"bad row {(c, d)} must come back as zeros"
    err = np.abs(got[..., 3:].astype(np.float64) - want)
    live = hp.live_mask(rows, H, W)
    ratio = (err[live] / bound[live]).max()
    dense = hp.gather(rows, dense_path(feat, heads, _lib.CONV_F16X3), H, W)
    e_new, e_dense = err.max(), np.abs(dense - want).max()
    print(f"cin {cin} {H}x{W} hidden {hidden} outs {outs}: error / bound max {ratio:.4f}; max error at peaks {e_new:.3e}, dense f16x3 {e_dense:.3e}")
    assert ratio <= 1.0, f"beyond 2e-6 sum|a||b|: worst error / bound {ratio:.3f}"
    assert e_new <= e_dense, f"less accurate than the dense path it replaces: {e_new:.3e} > {e_dense:.3e}"
    # two launches are bit-identical; the same rows in another order give the same values per row
    assert np.array_equal(layer(feat.to(DEV), d_rows).cpu().numpy().view(np.uint32), got.view(np.uint32))
    perm = np.random.default_rng(0).permutation(30)
    shuffled = rows.reshape(30, 3)[perm].reshape(2, 15, 3)
    again = layer(feat.to(DEV), torch.from_numpy(shuffled).to(DEV)).cpu().numpy()
    assert np.array_equal(again.reshape(30, -1).view(np.uint32), got.reshape(30, -1)[perm].view(np.uint32))


@pytest.fixture(scope="module")
def lidar_model():
    import bench
    _, _, (lm, _, _, _) = bench.build_pipeline(DEV, eager=True)
    return lm


def test_detect_against_the_dense_path_on_the_model(lidar_model):
    """LiDARModel.detect against heads() + extract_peaks(heat, size, ori) on a seeded (1, 384, 12, 20) feature map: positions equal,
    scores and pred_bev within the e2e test's atol = 1e-5, attributes within the bars of test_kernel_against_float64; with the dense
    kernels at exact fp32 (lav_conv.precision f32; and at the library default, three bf16 pieces) the attributes agree to the fp32 bar
    alone.  Prints whether the two-head engine's heat map equals the four-head engine's bit for bit."""
    lm = lidar_model
    feats = torch.randn((1, 384, 12, 20), generator=torch.Generator().manual_seed(7)).to(DEV)
    H, W = feats.shape[2:]
    heads = [(h.net[0], h.net[2], h.net[3]) for h in (lm.box_head, lm.ori_head)]
    cpu_heads = [tuple(copy.deepcopy(m).cpu() for m in h) for h in heads]
    refs = [hp.dense_reference(feats[0].cpu(), h) for h in cpu_heads]
    with torch.no_grad():
        for prec in (ops.frame_precision(), _lib.CONV_F32, 0):
            with ops.precision(prec):
                heat4, size, ori, bev4 = lm.heads(feats)
                dense = ops.extract_peaks(heat4[0], size[0], ori[0], apply_sigmoid=True).cpu().numpy()
                heat2, _ = lm.heads(feats, ("center_head", "seg_head"))
                rows, bev = lm.detect(feats)
                same = torch.equal(heat2, heat4)
            rows = rows.cpu().numpy()
            assert rows.shape == dense.shape == (2, 15, 7)
            np.testing.assert_array_equal(rows[..., 1:3], dense[..., 1:3], err_msg=f"precision {prec}: peak positions")
            d_score = np.abs(rows[..., 0] - dense[..., 0]).max()
            d_bev = (bev - bev4).abs().max().item()
            want = hp.gather(rows[..., :3], [v.numpy() for v, _ in refs], H, W)
            bound = hp.gather(rows[..., :3], [b.numpy() for _, b in refs], H, W)
            live = hp.live_mask(rows[..., :3], H, W)
            assert live.sum() >= 4
            e_new, e_dense = np.abs(rows[..., 3:] - want), np.abs(dense[..., 3:] - want)
            ratio = (e_new[live] / bound[live]).max()
            print(f"precision {prec}: two-head heat == four-head heat bit for bit: {same}; max |score diff| {d_score:.3e}, |pred_bev diff| {d_bev:.3e}; "
                  f"attributes: error / bound max {ratio:.4f}, max error at peaks {e_new.max():.3e}, dense {e_dense.max():.3e}, "
                  f"max |at peaks - dense| / bound {(np.abs(rows[..., 3:] - dense[..., 3:])[live] / bound[live]).max():.4f}")
            assert d_score <= 1e-5 and d_bev <= 1e-5
            assert ratio <= 1.0
            if prec == ops.frame_precision():
                assert e_new.max() <= e_dense.max()
            else:
                assert (np.abs(rows[..., 3:] - dense[..., 3:])[live] <= bound[live]).all()


WORKER = """
import sys, numpy as np, torch
sys.path.insert(0, {repo!r})
import bench
from lav_amd.frame import GraphedFramePipeline
dev = torch.device('cuda', 0)
_, _, models = bench.build_pipeline(dev, eager=True)
pipe = GraphedFramePipeline(*models, 1.5, 2.4, num_frame_stack=2, device=dev, points_per_tick=8192)
host, d = bench.synthetic_inputs(dev, n_points=8192)
out = {{}}
for i in range(5):
    loc, ori = bench.pose(i)
    o = pipe.step(d['ticks'][i % len(d['ticks'])], d['all_rgbs'], d['rgbs'], d['tel_rgbs'], loc, ori, d['nxp'], 3)
    torch.cuda.synchronize()
    if o is None: continue
    out[f'bra{{i}}'] = o['pred_bra'].cpu().numpy(); out[f'plan{{i}}'] = o['ego_plan_locs'].cpu().numpy()
    out[f'cast{{i}}'] = o['other_cast_locs'].cpu().numpy(); out[f'det{{i}}'] = pipe.hn_det.copy()
np.savez(sys.argv[1], **out)
"""


def test_knob_restores_the_dense_path_and_the_frame_stays(tmp_path):
    """LAV_HEADS_AT_PEAKS=0 against the default, each in a process of its own (the knob is read at import), four frames of the bench
    inputs at points_per_tick = 8192: same detection counts and pixel positions per class, pred_bra equal, attributes within
    atol = 1e-5 + the dense f16x3 path's error relative to the largest value, measured here on test_kernel_against_float64's
    (384, 4, 6) case and scaled to the attributes' size, plans and forecasts within the e2e test's tolerances."""
    feat = torch.randn((384, 4, 6), generator=torch.Generator().manual_seed(384 + 64))
    heads = [hp.make_head(384, 64, o, 10 * g + o) for g, o in enumerate((1, 3))]
    rows, _ = hp.hand_rows(4, 6)
    want = hp.gather(rows, [hp.dense_reference(feat, h)[0].numpy() for h in heads], 4, 6)
    rel_dense = np.abs(hp.gather(rows, dense_path(feat, heads, _lib.CONV_F16X3), 4, 6) - want).max() / np.abs(want).max()
    print(f"dense f16x3 path: max error / max |value| = {rel_dense:.3e}")
    worker = tmp_path / "frames.py"
    worker.write_text(WORKER.format(repo=REPO))
    got = {}
    base = {k: v for k, v in os.environ.items() if k != "LAV_HEADS_AT_PEAKS"}
    for name, env in (("at_peaks", {}), ("dense", {"LAV_HEADS_AT_PEAKS": "0"})):       # the default against the knob
        f = tmp_path / f"{name}.npz"
        r = subprocess.run([sys.executable, str(worker), str(f)], env={**base, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = dict(np.load(f))
    a, b = got["at_peaks"], got["dense"]
    assert a.keys() == b.keys() and len(a) == 16
    for i in range(1, 5):
        da, db = a[f"det{i}"], b[f"det{i}"]
        np.testing.assert_array_equal(da[..., 1:3], db[..., 1:3], err_msg=f"frame {i}: peak positions")
        np.testing.assert_array_equal(da[..., 0] > 0.2, db[..., 0] > 0.2, err_msg=f"frame {i}: detection counts")
        size = np.abs(db[..., 3:]).max()
        diff = np.abs(da[..., 3:] - db[..., 3:]).max()
        print(f"frame {i}: max |attribute diff| {diff:.3e} at |attributes| max {size:.3e}; max |score diff| {np.abs(da[..., 0] - db[..., 0]).max():.3e}")
        assert np.abs(da[..., 0] - db[..., 0]).max() <= 1e-5
        assert diff <= 1e-5 + rel_dense * size
        np.testing.assert_array_equal(a[f"bra{i}"], b[f"bra{i}"], err_msg=f"frame {i}: pred_bra")
        for k in (f"plan{i}", f"cast{i}"):
            assert a[k].shape == b[k].shape, k
            np.testing.assert_allclose(a[k], b[k], atol=2e-5, rtol=2e-6, err_msg=k)
