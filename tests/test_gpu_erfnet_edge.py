"""lav_erfnet_entry (csrc/erfnet_edge.hip): ERFNet's two entry DownsamplerBlocks as one launch, against float64 of the module's own
layers on the CPU and against the four launches it replaces (DownsamplerBlock.engine twice) on the same device input.

Bar (the rule tests/test_gpu_conv_tile.py uses for a fused run): max|fused - f64| <= 2 max|per-launch - f64| + 1.2e-7 max|f64| - twice the
distance of the path it replaces plus one rounding of the largest value.  On exactly representable data (small integers, BatchNorm
scales that are powers of two: tests/exact_util.py) fused, per-launch and float64 agree bit for bit."""
import copy
import functools

import numpy as np
import pytest
import torch

from lav_amd import synth
from tests import exact_util as xu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

GEOMS = [(1, 4, 4), (1, 8, 12), (3, 36, 68), (2, 64, 128), (3, 288, 256)]     # (B, H, W): one pixel; small; ragged 9 x 17; whole tiles; the frame
AFFINES = [None, (2.0 / 255.0, -1.0)]                                          # the second one's pad value (127.5) is not zero


@functools.lru_cache(maxsize=None)
def blocks():
    """The two entry blocks with seeded parameters (eval mode, float32, on the CPU)."""
    from lav_amd.erfnet import DownsamplerBlock
    g = torch.Generator().manual_seed(11)
    out = []
    for cin, cout in ((3, 16), (16, 64)):
        blk = DownsamplerBlock(cin, cout).eval()
        with torch.no_grad():
            for p in blk.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            blk.bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
            blk.bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
        out.append(blk)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exact_blocks():
    """Integer weights and biases, BatchNorm folding to scales 0.5 / 1 and integer shifts (eps = 0): every intermediate value is a
    multiple of 2^-4 far below 2^24 in every precision mode."""
    from lav_amd.erfnet import DownsamplerBlock
    out = []
    for cin, cout, wb in ((3, 16, 2), (16, 64, 1)):
        rng = xu.rng_of("erfnet_edge", cin, cout)
        blk = DownsamplerBlock(cin, cout).eval()
        blk.bn.eps = 0.0
        bn, _, _ = xu.pow2_bn(rng, cout)
        with torch.no_grad():
            blk.conv.weight.copy_(xu.integers(rng, tuple(blk.conv.weight.shape), wb))
            blk.conv.bias.copy_(xu.integers(rng, (cout - cin,), 3))
            for dst, src in zip((blk.bn.running_mean, blk.bn.running_var, blk.bn.weight, blk.bn.bias), bn):
                dst.copy_(src)
        out.append(blk)
    return tuple(out)


def f64(blks, x, affine):
    """DownsamplerBlock.forward twice on s x + t, in float64 on the CPU."""
    b1, b2 = (copy.deepcopy(b).double() for b in blks)
    x = x.double()
    if affine is not None:
        x = x * affine[0] + affine[1]
    with torch.no_grad():
        for b in (b1, b2):
            if b.bn.eps > 0:
                x = b(x)
            else:      # (torch refuses eps = 0: the same layers with the BatchNorm written out)
                scale = b.bn.weight / torch.sqrt(b.bn.running_var)
                x = torch.relu(xu.affine(torch.cat([b.conv(x), b.pool(x)], 1), scale, b.bn.bias - b.bn.running_mean * scale))
    return x


@functools.lru_cache(maxsize=None)
def stages(exact, affine):
    """(fused stage, per-launch path) of the blocks on the device."""
    from lav_amd import erfnet
    b1, b2 = exact_blocks() if exact else blocks()
    first, second = b1.engine(DEV, affine), b2.engine(DEV)
    return erfnet._entry_stage(b1, b2, DEV, affine, first, second), (lambda x: second(first(x)))


def raw_input(B, H, W, affine):
    g = torch.Generator().manual_seed(B * 1000003 + H * 1009 + W)
    if affine is None:
        return torch.randn((B, 3, H, W), generator=g)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float()


@functools.lru_cache(maxsize=None)
def case(B, H, W, affine):
    """(input, float64 reference): computed once per geometry and affine, never written to."""
    x = raw_input(B, H, W, affine)
    return x, f64(blocks(), x, affine)


@pytest.mark.parametrize("affine", AFFINES, ids=["plain", "affine"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_entry_against_float64_and_the_launches_it_replaces(geom, affine):
    from lav_amd import ops
    B, H, W = geom
    x, want = case(B, H, W, affine)
    fused, launches = stages(False, affine)
    xd = x.to(DEV)
    assert ops.erfnet_entry_takes(xd)
    with torch.no_grad():
        got, old = fused(xd).cpu().double(), launches(xd).cpu().double()
    assert got.shape == want.shape == (B, 64, H // 4, W // 4)
    e_new, e_old, top = float((got - want).abs().max()), float((old - want).abs().max()), float(want.abs().max())
    print(f"{geom} affine={affine}: fused {e_new:.3e}  per-launch {e_old:.3e}  max|f64| {top:.3e}  bar {2 * e_old + 1.2e-7 * top:.3e}")
    assert torch.isfinite(got).all()
    assert e_new <= 2 * e_old + 1.2e-7 * top


@pytest.mark.parametrize("geom", [(1, 4, 4), (3, 36, 68)], ids=lambda g: "x".join(map(str, g)))
def test_entry_is_deterministic_and_stays_inside_its_output(geom):
    """Two launches on one input are bit-equal; a canary value around the output buffer is untouched."""
    from lav_amd import ops
    B, H, W = geom
    affine = AFFINES[1]
    xd = case(B, H, W, affine)[0].to(DEV)
    fused, _ = stages(False, affine)
    n, guard, canary = B * 64 * (H // 4) * (W // 4), 4096, -12345.5
    buf = torch.full((n + 2 * guard,), canary, device=DEV)
    out = buf[guard:guard + n].view(B, 64, H // 4, W // 4)
    args = fused.args
    a = ops.erfnet_entry(xd, *args, out=out).clone()
    b = ops.erfnet_entry(xd, *args, out=out)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, fused(xd))
    assert bool((buf[:guard] == canary).all()) and bool((buf[guard + n:] == canary).all())
    assert args[2] == 127.5 and bool((a != canary).all())


@pytest.mark.parametrize("affine", [None, (0.5, -1.0)], ids=["plain", "affine"])      # (0.5, -1): exact folding, pad value 2
@pytest.mark.parametrize("geom", [(1, 4, 4), (3, 36, 68), (2, 64, 128)], ids=lambda g: "x".join(map(str, g)))
def test_entry_exact_data_bit_for_bit(geom, affine):
    """A wrong tap, pad value or channel window that a tolerance would hide: fused, per-launch and float64 agree bit for bit."""
    B, H, W = geom
    x = xu.integers(xu.rng_of("erfnet_edge_x", geom), (B, 3, H, W), 4).float()
    want = f64(exact_blocks(), x, affine)
    fused, launches = stages(True, affine)
    xd = x.to(DEV)
    with torch.no_grad():
        got, old = fused(xd), launches(xd)
    assert float(want.abs().max()) > 8 and float((want > 0).double().mean()) > 0.2      # (not a map of zeros)
    xu.assert_exact(old, want, f"per-launch {geom} {affine}")
    xu.assert_exact(got, want, f"fused {geom} {affine}")


def test_entry_falls_back_for_what_the_kernel_does_not_take():
    """A non-contiguous input takes the blocks' own launches (their bits); H % 4 != 0 is refused by them as it was before."""
    from lav_amd import ops
    affine = AFFINES[1]
    fused, launches = stages(False, affine)
    g = torch.Generator().manual_seed(5)
    nhwc = torch.randint(0, 256, (2, 24, 20, 3), generator=g).float().to(DEV).permute(0, 3, 1, 2)     # channels last
    assert not nhwc.is_contiguous() and not ops.erfnet_entry_takes(nhwc)
    with torch.no_grad():
        assert torch.equal(fused(nhwc), launches(nhwc.contiguous()))
    odd = torch.zeros((1, 3, 6, 8), device=DEV)               # block 1 leaves 3 rows: neither the module nor lav_pool_affine pools them
    assert not ops.erfnet_entry_takes(odd)
    with pytest.raises(RuntimeError, match="pool_affine"):
        launches(odd)
    with pytest.raises(RuntimeError, match="pool_affine"):
        fused(odd)
    with pytest.raises(RuntimeError, match="not served"):
        ops.erfnet_entry(odd, *[torch.zeros(1, device=DEV)] * 2, 0.0, *[torch.zeros(1, device=DEV)] * 6)


def _seg_and_input():
    from lav_amd.rgb import RGBSegmentationModel
    seg = RGBSegmentationModel([4, 6, 7, 10]); seg.load_state_dict(synth.seeded_state_dict(seg, prefix="seg.")); seg.eval().to(DEV)
    cams, _ = synth.rgb_frames()
    x = torch.tensor(np.stack([c[..., :3][..., ::-1] for c in cams], 0).copy()).permute(0, 3, 1, 2).float().contiguous().to(DEV)
    return seg, x


def test_knob_restores_the_old_stages_and_the_network_keeps_its_logits(monkeypatch):
    """LAV_ERFNET_ENTRY=0: the two blocks' own stages again.  RGBSegmentationModel on synth.rgb_frames() with the knob on against off:
    logits within 1e-5 max|logit| (the absolute term of test_camera_nets_vs_reference_golden); four persistent runs per pass either way."""
    from lav_amd import ops
    seg, x = _seg_and_input()
    net, key = seg.erfnet, ((2.0 / 255.0, -1.0), False)
    out, nstages = {}, {}
    for knob in ("0", "1"):
        monkeypatch.setenv("LAV_ERFNET_ENTRY", knob)
        net._drop()
        with torch.no_grad():
            t0, n0 = ops.pair_chain_status(DEV)
            out[knob] = seg(x).clone()
            t1, n1 = ops.pair_chain_status(DEV)
        assert (t1, n1) == (t0, n0 + 4), (knob, t0, n0, t1, n1)
        st = net._engine(x.device, *key)
        nstages[knob] = len(st)
        assert [bool(getattr(s, "fused_entry", False)) for s in st[:2]] == ([True, False] if knob == "1" else [False, False])
    assert nstages["0"] == nstages["1"] + 1
    top = float(out["0"].abs().max())
    diff = float((out["1"] - out["0"]).abs().max())
    print(f"logits: max|on - off| {diff:.3e}, max|logit| {top:.3e}, bar {1e-5 * top:.3e}")
    assert diff <= 1e-5 * top
