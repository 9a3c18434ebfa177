"""The reference tests/test_gpu_heads_at_peaks.py compares lav_heads_at_peaks with (tests/heads_peaks_util.py: the module's layers in
float64, dense, gathered at the rows) against the rule the kernel is built on, written out by hand on a 3 x 4 map: an output pixel
(x, y) of ConvTranspose2d(k 3, stride 2, padding 1, output_padding 1) depends on the hidden rows y / 2 through tap ky = 1 when y is
even, and on (y - 1) / 2 through ky = 2 and (y + 1) / 2 through ky = 0 when y is odd - the latter only if it exists (< H) - likewise in
x; a hidden pixel is ReLU -> BatchNorm of a 3 x 3 x cin window of the zero-padded feature map.  No GPU."""
import numpy as np
import torch

from tests import heads_peaks_util as hp


def parity_rule(feat, head, x, y):
    """The head's outputs at output pixel (x, y), float64, by the rule of the module docstring."""
    conv, bn, ct = head
    w1 = conv.weight.detach().double().numpy()                # (hidden, cin, 3, 3)
    wt = ct.weight.detach().double().numpy()                  # (hidden, outs, 3, 3)
    scale = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).numpy()
    shift = bn.bias.detach().double().numpy() - bn.running_mean.double().numpy() * scale
    f = feat.double().numpy()
    cin, H, W = f.shape
    pad = np.zeros((cin, H + 2, W + 2))
    pad[:, 1:-1, 1:-1] = f
    taps = lambda v, n: [(v // 2, 1)] if v % 2 == 0 else [(i, k) for i, k in (((v - 1) // 2, 2), ((v + 1) // 2, 0)) if i < n]
    out = ct.bias.detach().double().numpy().copy()
    for hy, ky in taps(y, H):
        for hx, kx in taps(x, W):
            hidden = np.maximum(np.einsum("ocyx,cyx->o", w1, pad[:, hy:hy + 3, hx:hx + 3]), 0) * scale + shift
            out += hidden @ wt[:, :, ky, kx]
    return out


def test_dense_reference_is_the_parity_rule_on_a_3x4_map():
    H, W, cin = 3, 4, 5
    feat = torch.randn((cin, H, W), generator=torch.Generator().manual_seed(1))
    for hidden, outs, seed in ((8, 2, 2), (3, 3, 3)):
        head = hp.make_head(cin, hidden, outs, seed)
        vals, bound = hp.dense_reference(feat, head)
        assert vals.shape == (outs, 2 * H, 2 * W) and bound.shape == vals.shape and (bound > 0).all()
        n_hidden = set()
        for y in range(2 * H):
            for x in range(2 * W):
                np.testing.assert_allclose(vals[:, y, x].numpy(), parity_rule(feat, head, x, y), rtol=0, atol=1e-13)
                n_hidden.add((1 + (y % 2 and (y + 1) // 2 < H)) * (1 + (x % 2 and (x + 1) // 2 < W)))
        assert n_hidden == {1, 2, 4}


def test_hand_rows_cover_the_cases_and_gather_zeroes_the_bad_rows():
    for H, W in ((3, 4), (5, 7), (4, 6)):
        rows, bad = hp.hand_rows(H, W)
        live = hp.live_mask(rows, H, W)
        assert rows.shape == (2, 15, 3) and not any(live[c, d] for c, d in bad) and live.sum() == 30 - len(bad)
        pts = [(int(r[1]), int(r[2])) for c in range(2) for r, ok in zip(rows[c], live[c]) if ok]
        assert {(x % 2, y % 2) for x, y in pts} == {(0, 0), (1, 0), (0, 1), (1, 1)}
        assert {(0, 0), (2 * W - 1, 0), (0, 2 * H - 1), (2 * W - 1, 2 * H - 1)} <= set(pts)
        assert len(pts) > len(set(pts))                                        # one pixel in two rows
        maps = [np.arange(2 * 2 * H * 2 * W, dtype=np.float64).reshape(2, 2 * H, 2 * W) + 1, -np.ones((1, 2 * H, 2 * W))]
        g = hp.gather(rows, maps, H, W)
        assert g.shape == (2, 15, 3)
        for c, d in bad:
            assert not g[c, d].any()
        assert g[0, 1, 0] == maps[0][0, 0, 2 * W - 1] and g[0, 2, 1] == maps[0][1, 2 * H - 1, 0] and g[0, 0, 2] == -1
