"""The per-tick glue kernels at ties, caps and thresholds (lav_extract_peaks, lav_det_decode, lav_nonfinite_count,
lav_maxpool3x3s2, lav_stack_sweeps, lav_merge_ticks; through the C ABI), bit for bit against the numpy references of
tests/frame_ref_util.py.  tests/test_frame_ref_host.py holds those references to the oracle, asserts the premise of every table
used here (ties present, candidate counts on the intended side of the 2048 bound, filler rows) and shows that each single-rule
mistake changes the expected rows.  The only tolerance is the existing 2.4e-7 on the headings (a double atan2 rounded to float32
against the device's: one float32 ulp below pi)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lav_amd import _lib, ops
from tests import frame_ref_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the shared case arrays are read-only)


def run_case(name):
    heat, size, ori, ks, max_det, sig, want, cand = U.peak_case(name)
    got = ops.extract_peaks(dev(heat), dev(size), dev(ori), ks=ks, max_det=max_det, apply_sigmoid=sig).cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=f"{name}: {cand} candidates per class")
    return got, want, cand


# ------------------------------------------------------------------------------------------------ peaks
@pytest.mark.parametrize("name", list(U.TIE_CASES))
def test_peaks_ties_and_caps(name):
    """Rows by descending score, ties by ascending pixel index, the gathered columns, and (-1e5, 0, 0, ..) exactly beyond the
    survivors: up to 8 planes, max_det 64, windows 1 to 15, maps smaller than a tile and than max_det, partial tiles both ways."""
    got, want, _ = run_case(name)
    fill = U.filler_rows(want)
    for c in range(got.shape[0]):
        n = got.shape[1] - fill[c]
        assert (got[c, n:, 0] == U.FILLER).all() and not got[c, n:, 1:].any()


@pytest.mark.parametrize("name", list(U.PATH_CASES))
def test_peaks_on_both_selection_paths(name):
    """The last workgroup keeps up to 2048 candidates of a class in registers and rescans the list in HBM beyond: plateau maps
    with exactly 2048, with more (partial tiles, and both classes of the frame's own 320 x 320 map at once) and the evaluator's
    max_det = 20 configuration."""
    kind, shape, _, want_cand, _ = U.PATH_CASES[name]
    _, _, cand = run_case(name)
    assert cand == [want_cand] * shape[0]
    assert (max(cand) > U.REG_CANDIDATES) == (kind == "scan")


@pytest.mark.parametrize("name", list(U.SIGMOID_CASES))
def test_peaks_on_saturated_logits(name):
    """apply_sigmoid on logits whose float32 sigmoid is exactly 0, 0.5 or 1: large exact plateaus across tile borders."""
    run_case(name)


def test_peaks_on_a_shared_workspace_and_in_graph_replays():
    """large -> small -> large maps on the cached workspace (the counters sit at the end of the larger buffer), then three
    replays of one captured launch with the heat map rewritten in place."""
    for name in ("p320", "t3", "t33x65", "p320", "t1", "p320d20"):
        run_case(name)
    heat, size, ori, ks, max_det, _, _, _ = U.peak_case("t64x96")
    alt = np.zeros_like(heat)                       # the second map: t33x65 inside an all-(-2) frame of the first one's shape
    alt[:] = -2
    alt[:, :33, :65] = U.peak_case("t33x65")[0]
    maps = (heat, alt, heat)
    d_heat, d_size, d_ori = dev(heat), dev(size), dev(ori)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.extract_peaks(d_heat, d_size, d_ori, ks=ks, max_det=max_det)          # the stream's workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rows = ops.extract_peaks(d_heat, d_size, d_ori, ks=ks, max_det=max_det)
    torch.cuda.synchronize()
    for m in maps:
        d_heat.copy_(dev(m))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(rows.cpu().numpy(), U.peaks_ref(m, size, ori, ks, max_det)[0])


def test_peaks_with_a_nan():
    """A +NaN is ignored inside every window; the NaN pixel itself survives and sorts by its bit pattern, first.  The other
    planes are the rows of the same call without it, and nothing is written behind `out`."""
    heat, clean, (y, x) = U.nan_map()
    ncls, H, W = heat.shape
    size, ori = U.gather_maps(H, W, 9)
    want, _ = U.peaks_ref(heat, size, ori, 7, 15)
    lib = _lib.load()
    ws = torch.zeros(lib.lav_extract_peaks_workspace_bytes(ncls, H, W), dtype=torch.uint8, device=DEV)
    d_size, d_ori = dev(size), dev(ori)
    res = []
    for m in (heat, clean):
        buf = torch.full((ncls * 15 * 7 + 1024,), 7.0, device=DEV)
        d = dev(m)
        rc = lib.lav_extract_peaks(d.data_ptr(), ncls, H, W, 7, 15, 0, d_size.data_ptr(), 2, d_ori.data_ptr(), 2, buf.data_ptr(), ws.data_ptr(),
                                   ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.lav_last_error().decode()
        b = buf.cpu().numpy()
        assert (b[ncls * 15 * 7:] == 7.0).all(), "written behind out"
        res.append(b[:ncls * 15 * 7].reshape(ncls, 15, 7))
    got, got_clean = res
    np.testing.assert_array_equal(got, want)
    assert got[1, 0, 0].view(np.uint32) == U.NAN_BITS and (got[1, 0, 1], got[1, 0, 2]) == (x, y)
    np.testing.assert_array_equal(got[[0, 2]], got_clean[[0, 2]])
    np.testing.assert_array_equal(got_clean, U.peaks_ref(clean, size, ori, 7, 15)[0])


# ------------------------------------------------------------------------------------------------ detection decode
def decode(rows, cls, consts):
    max_det = rows.shape[1]
    actors = torch.full((3 * max_det + 16,), 5.0, device=DEV)
    n_out = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    ops.det_decode(dev(rows), actors, n_out[1:2], cls=cls, **consts)
    a, n = actors.cpu().numpy(), n_out.cpu().numpy()
    assert (a[3 * max_det:] == 5.0).all() and n[0] == -7 and n[2] == -7, "written outside actors / n_out"
    want, want_n = U.det_decode_ref(rows, cls, **consts)
    assert n[1] == want_n
    np.testing.assert_array_equal(a[:2 * max_det], want[:2 * max_det])
    np.testing.assert_allclose(a[2 * max_det:3 * max_det], want[2 * max_det:], rtol=0, atol=2.4e-7)
    assert not a[2 * want_n:2 * max_det].any() and not a[2 * max_det + want_n:3 * max_det].any()
    return a, int(n[1])


@pytest.mark.parametrize("consts", [U.DECODE, U.DECODE_EXACT], ids=["frame_constants", "float32_thresholds"])
def test_det_decode_on_its_thresholds(consts):
    """One constructed row per filter, on and beside each strict inequality: a score of 0.2f passes `> 0.2` (and fails
    `> (double)0.2f`), distances of exactly near_px, far_px and skip_px are dropped, a box of exactly min_box and NaN sizes are
    kept, the filler and a NaN score are dropped, fractional coordinates truncate."""
    rows = U.decode_rows("threshold")
    a, n = decode(rows, 1, consts)
    if consts is U.DECODE:
        kept = [k for _, _, k in U.DECODE_THRESHOLD_ROWS]
        assert n == sum(kept)
        for j, (label, _, k) in enumerate(U.DECODE_THRESHOLD_ROWS):
            assert decode(np.repeat(rows[:, j:j + 1], 2, axis=1), 1, consts)[1] == (2 if k else 0), label


@pytest.mark.parametrize("kind,ncls,cls", [("all64", 2, 1), ("none64", 2, 1), ("threshold", 1, 0), ("all64", 1, 0), ("none64", 2, 0)])
def test_det_decode_at_the_full_wave_and_at_class_0(kind, ncls, cls):
    """max_det = 64: every lane owns a row and lane 63's prefix is (1 << 63) - 1; all rows kept (count 64), all dropped (0),
    and one plane with cls = 0."""
    rows = U.decode_rows(kind, ncls=ncls, cls=1 if (kind, ncls, cls) == ("none64", 2, 0) else cls)
    _, n = decode(rows, cls, U.DECODE)
    kept = sum(k for _, _, k in U.DECODE_THRESHOLD_ROWS)
    assert n == {"all64": 64, "none64": 64 if ncls == 2 and cls == 0 else 0, "threshold": kept}[kind]


# ------------------------------------------------------------------------------------------------ health counter
def _finite(n, seed):
    g = np.random.default_rng([seed, 8])
    v = (g.standard_normal(n) * 1e3).astype(np.float32)
    if n:
        v[g.integers(0, n)] = np.finfo(np.float32).max
        v[g.integers(0, n)] = -np.finfo(np.float32).max
        v[g.integers(0, n)] = np.float32(1e-45)                 # subnormal
        v[g.integers(0, n)] = -np.finfo(np.float32).tiny / 2
    return v


NONFINITE_LENGTHS = (0, 1, 255, 256, 257, 100001)


def test_nonfinite_count_per_length_and_position():
    counter = torch.tensor([40, 2], dtype=torch.int32, device=DEV)          # sticky: starts from a non-zero value
    bad_total, launches = 40, 2
    for n in NONFINITE_LENGTHS:
        v = _finite(n, n)
        variants = [(v, 0)]
        if n:
            for pos, val in ((n - 1, np.nan), (0, np.inf), (n // 2, -np.inf)):
                w = v.copy()
                w[pos] = val
                variants.append((w, 1))
        for w, bad in variants:
            ops.nonfinite_count([dev(w)], counter)
            bad_total, launches = bad_total + bad, launches + 1
            assert counter.cpu().tolist() == [bad_total, launches], f"length {n}"
    ops.nonfinite_count([], counter)                                        # n = 0 adds (0, 1)
    assert counter.cpu().tolist() == [bad_total, launches + 1]


def test_nonfinite_count_of_eight_tensors_in_one_launch():
    ts = [_finite(n, 100 + i) for i, n in enumerate((257, 1, 0, 100001, 256, 255, 3, 513))]
    ts[0][256] = np.nan
    ts[3][50000] = -np.inf
    ts[7][0] = np.inf
    counter = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    d = [dev(t) for t in ts]
    ops.nonfinite_count(d, counter)
    assert counter.cpu().tolist() == [5 + 3, 9 + 1]
    ops.nonfinite_count(d, counter)                                          # sticky across launches
    assert counter.cpu().tolist() == [5 + 6, 9 + 2]
    with pytest.raises(RuntimeError):
        ops.nonfinite_count(d + [d[1]], counter)                             # nine tensors: refused before any launch
    torch.cuda.synchronize()
    assert counter.cpu().tolist() == [5 + 6, 9 + 2]


# ------------------------------------------------------------------------------------------------ max pooling
def _pool_input(shape, seed):
    g = np.random.default_rng([seed, 9])
    x = g.standard_normal(shape).astype(np.float32)
    B, Cc, H, W = shape
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1), (H // 2, W // 2)]
    spots = list(dict.fromkeys(spots))                   # corners, edge middles and the centre coincide on thin maps
    vals = (np.nan, np.inf, -np.inf)
    for p in range(B * Cc):
        for k, (y, xx) in enumerate(spots):
            if len(spots) <= 3 or (k + p) % 2 == 0:
                x.reshape(B * Cc, H, W)[p, y, xx] = vals[(k + p) % 3]
    if H >= 5 and W >= 5:
        x.reshape(B * Cc, H, W)[0, H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] = -np.inf    # a whole window of -inf
    return x


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 7), (1, 2, 9, 1), (2, 1, 1, 1), (1, 3, 8, 6), (3, 2, 17, 33)])
def test_maxpool3x3s2_propagates_nan_and_infinities(shape):
    x = _pool_input(shape, 1)
    want = F.max_pool2d(torch.from_numpy(x), 3, 2, 1).numpy()               # the CPU kernel: the documented rule
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any() == (shape[2] * shape[3] > 1)
    np.testing.assert_array_equal(ops.maxpool3x3s2(dev(x)).cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(3, 2, 17, 33), (2, 3, 5, 7)])
def test_maxpool3x3s2_under_batch_limit(shape):
    x = _pool_input(shape, 2)
    B, Cc, H, W = shape
    want = F.max_pool2d(torch.from_numpy(x), 3, 2, 1).numpy()
    lib, d_x = _lib.load(), dev(x)
    for n in (0, 1, B):
        y = torch.full(want.shape, -77.0, device=DEV)
        with ops.batch_limit(torch.tensor([n], dtype=torch.int32, device=DEV)):
            rc = lib.lav_maxpool3x3s2(d_x.data_ptr(), B, Cc, H, W, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.lav_last_error().decode()
            torch.cuda.synchronize()
        got = y.cpu().numpy()
        np.testing.assert_array_equal(got[:n], want[:n])
        assert (got[n:] == -77.0).all(), f"rows beyond {n} were written"
    np.testing.assert_array_equal(ops.maxpool3x3s2(d_x).cpu().numpy(), want)       # the limit is off again


# ------------------------------------------------------------------------------------------------ lidar glue
@pytest.mark.parametrize("rows", [1, 256, 257, 3000])
def test_stack_sweeps_bit_for_bit(rows):
    """All eleven columns against products summed left to right with one float32 rounding each: a fused multiply-add anywhere
    in the rotation differs on these inputs (tests/test_frame_ref_host.py).  NaN x as lav_merge_ticks leaves them."""
    fused, ring, slot, sweeps, R, t = U.stack_inputs(rows, seed=rows, nan_rows=(0, rows // 2, rows - 1))
    want, ring_after = U.stack_sweeps_ref(fused, ring, slot, sweeps, R, t)
    d_ring = dev(ring)
    out = ops.stack_sweeps(dev(fused), d_ring, torch.tensor([slot], device=DEV), torch.tensor(sweeps, device=DEV), dev(R), dev(t))
    got = out.cpu().numpy()
    assert got.shape == (3 * rows, 11) and np.isnan(want[:, 0]).sum() >= 2
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(d_ring.cpu().numpy(), ring_after)


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_merge_ticks_rows_and_box_faces(rows):
    """Points exactly on each of the six faces of the ego box are kept, the points one float32 inside are marked x = NaN."""
    tick, prev = U.merge_inputs(rows, seed=rows)
    want, want_prev, inside = U.merge_ticks_ref(tick, prev)
    d_prev = dev(prev)
    guard = torch.full((2 * rows + 8, 4), 3.0, device=DEV)
    cur = ops.merge_ticks(dev(tick), d_prev, out=guard[:2 * rows]).cpu().numpy()
    assert inside.any() and not inside.all()
    np.testing.assert_array_equal(np.isnan(cur[:, 0]), inside)
    np.testing.assert_array_equal(cur, want)
    np.testing.assert_array_equal(d_prev.cpu().numpy(), want_prev)
    assert (guard[2 * rows:] == 3.0).all()


def test_merge_ticks_of_no_rows_is_a_no_op():
    lib = _lib.load()
    sentinel = torch.full((4, 4), 3.0, device=DEV)
    assert lib.lav_merge_ticks(sentinel.data_ptr(), sentinel.data_ptr(), 0, 4, sentinel.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert lib.lav_merge_ticks(None, None, 0, 4, None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (sentinel == 3.0).all()
    e = torch.zeros((0, 4), device=DEV)
    assert ops.merge_ticks(e, e.clone()).shape == (0, 4)
