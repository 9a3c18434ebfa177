"""lav_jpeg_encode (csrc/jpeg.hip, ops.jpeg_encode) on the GPU against the specification lav_amd.agent.mjpeg: every comparison is
exact.  The sizes and content cases are those of tests/test_mjpeg_host.py (tests/mjpeg_util.py says what each is the smallest shape
for); then a batch, reuse of the output and the workspace, refused arguments, the recorder on device frames and the agent with
debug_view_format: mjpeg (graphs and eager) and with the default config."""
import os

import numpy as np
import pytest
import torch
import yaml

from lav_amd import ops, synth
from lav_amd.agent import RoadOption
from lav_amd.agent import debug_view as V
from lav_amd.agent import mjpeg as M
from tests.mjpeg_util import CASES, SIZES, case_frame, lowpass_noise

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared case frames are read-only)


def encode(frame, quality, restart, **kw):
    scans, lengths = ops.jpeg_encode(dev(frame), quality, restart, **kw)
    assert scans.dtype == torch.uint8 and lengths.dtype == torch.int32 and scans.shape[0] == lengths.shape[0] == (1 if frame.ndim == 3 else len(frame))
    n = lengths.cpu().numpy()
    s = scans.cpu().numpy()
    return [s[i, :n[i]].tobytes() for i in range(len(n))]


@pytest.fixture(scope="module")
def want():
    """The specification's scan of every content case, made once."""
    return {name: M.scan_numpy(case_frame(name), q, r) for name, (q, r) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_specification_on_every_content_case(want, name):
    q, r = CASES[name]
    frame = case_frame(name)
    got, = encode(frame, q, r)
    assert len(got) == len(want[name]) <= M.scan_capacity(*frame.shape[:2], r)
    assert got == want[name]


@pytest.mark.parametrize("quality", [25, 100])
@pytest.mark.parametrize("h,w,restart", SIZES[:4])
def test_kernel_equals_specification_on_every_size(h, w, restart, quality):
    frame = lowpass_noise(h, w, seed=3) if quality == 25 else np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got, = encode(frame, quality, restart)
    assert got == M.scan_numpy(frame, quality, restart)


def test_a_batch_equals_single_calls():
    rng = np.random.default_rng(2)
    frames = np.stack([rng.integers(0, 256, (17, 33, 3), dtype=np.uint8), lowpass_noise(17, 33, seed=4), np.full((17, 33, 3), 77, np.uint8)])
    got = encode(frames, 90, 2)
    assert len(got) == 3 and len(set(map(len, got))) == 3
    for g, f in zip(got, frames):
        assert g == encode(f, 90, 2)[0] == M.scan_numpy(f, 90, 2)


def test_reused_output_and_workspace():
    rng = np.random.default_rng(3)
    noise, flat = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8), np.full((48, 48, 3), 130, np.uint8)
    cap = M.scan_capacity(48, 48, 4)
    out = torch.full((1, cap + 5), 0xAB, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros((1,), dtype=torch.int32, device="cuda")
    a = encode(noise, 100, 4, out=out, lengths=lengths)
    b = encode(noise, 100, 4, out=out, lengths=lengths)
    assert a == b == [M.scan_numpy(noise, 100, 4)]
    s, n = ops.jpeg_encode(dev(noise), 100, 4, out=out, lengths=lengths)
    assert s is out and n is lengths and bool((out[0, int(n[0]):] == 0xAB).all())          # nothing is written behind the scan
    # the flat frame after the noise frame, same shape and workspace: no interval keeps the length it had
    c = encode(flat, 100, 4, out=out, lengths=lengths)
    assert c == [M.scan_numpy(flat, 100, 4)] and len(c[0]) < len(a[0]) // 10
    ops._drop_workspace(("jpeg_encode", 1, 48, 48, 100, 4), torch.device("cuda", torch.cuda.current_device()))
    assert encode(flat, 100, 4) == c


def test_ops_jpeg_encode_refuses_wrong_arguments(monkeypatch):
    from lav_amd import _lib
    lib = _lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            if name == "lav_jpeg_encode":
                return lambda *a: calls.append(a) or lib.lav_jpeg_encode(*a)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Counting())
    frame = dev(np.zeros((16, 16, 3), np.uint8))
    cap = M.scan_capacity(16, 16, 10)
    bad = [dict(frames=frame.cpu()), dict(frames=frame.float()), dict(frames=dev(np.zeros((16, 16, 4), np.uint8))), dict(frames=frame[..., 0]),
           dict(frames=np.zeros((16, 16, 3), np.uint8)), dict(quality=0), dict(quality=101), dict(quality=50.0), dict(restart_mcus=0), dict(restart_mcus=-3),
           dict(restart_mcus=M.MAX_RESTART_MCUS + 1), dict(out=torch.empty((1, cap - 1), dtype=torch.uint8, device="cuda")),
           dict(out=torch.empty((2, cap), dtype=torch.uint8, device="cuda")), dict(out=torch.empty((1, cap), dtype=torch.uint8)),
           dict(out=torch.empty((1, cap), dtype=torch.int8, device="cuda")), dict(lengths=torch.empty((1,), dtype=torch.int64, device="cuda")),
           dict(lengths=torch.empty((2,), dtype=torch.int32, device="cuda"))]
    for change in bad:
        with pytest.raises(ValueError):
            ops.jpeg_encode(**{**dict(frames=frame, quality=90, restart_mcus=10), **change})
    assert not calls
    ops.jpeg_encode(frame)
    assert len(calls) == 1


# ---------------------------------------------------------------------------------------------- the recorder
def test_recorder_mjpeg_on_device_frames(tmp_path):
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (24, 40, 3), dtype=np.uint8) for _ in range(6)]
    rec = V.ViewRecorder(str(tmp_path / "v"), 4, format="mjpeg", quality=75, fps=5.0)
    for i, f in enumerate(frames):
        rec.append(dev(f), 10 + i)
        assert len(rec) == (i % 4) + 1 and len(rec.written) == (1 if i >= 4 else 0)
    assert rec.frames_jpeg() == [M.jpeg_encode_numpy(f, 75) for f in frames[4:]]
    assert rec.flush() == str(tmp_path / "v" / "view_000014.avi") and len(rec) == 0
    assert sorted(os.listdir(tmp_path / "v")) == ["view_000010.avi", "view_000014.avi"]
    for name, part in (("view_000010.avi", frames[:4]), ("view_000014.avi", frames[4:])):
        info, got = M.read_avi(str(tmp_path / "v" / name))
        assert got == [M.jpeg_encode_numpy(f, 75) for f in part]
        assert (info["microsec_per_frame"], info["total_frames"], info["width"], info["height"], info["closed"]) == (200000, len(part), 40, 24, True)
    # pinned memory does not grow with the capacity
    assert rec.stage[2].is_pinned() and tuple(rec.stage[2].shape) == (V.ViewRecorder.STAGES, M.scan_capacity(24, 40))


# ---------------------------------------------------------------------------------------------- the agent
def _agent(tmp_path, tag, **over):
    from lav_amd.lav_agent import LAVAgent
    cfg = dict(dict(synthetic_weights=True, points_per_tick=8192, precapture=False), **over)
    p = tmp_path / f"cfg_{tag}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    agent = LAVAgent(str(p))
    sc = synth.agent_scenario()
    agent.set_global_plan([({"lat": la, "lon": lo, "z": 0.0}, RoadOption(int(c))) for la, lo, c in zip(sc["lat"], sc["lon"], sc["cmds"])])
    return agent, sc


@pytest.mark.parametrize("hip_graphs", [True, False])
def test_agent_records_mjpeg_and_drives_the_same(tmp_path, hip_graphs):
    out_dir = tmp_path / "views"
    a, sc = _agent(tmp_path, "on", hip_graphs=hip_graphs, debug_view=True, debug_view_format="mjpeg", debug_view_flush=4, debug_view_every=1,
                   debug_view_quality=80, debug_view_dir=str(out_dir))
    b, _ = _agent(tmp_path, "off", hip_graphs=hip_graphs)
    clones = []
    real = a.visualize
    a.visualize = lambda *args: (lambda f: (clones.append(f.clone()), f)[1])(real(*args))
    ticks = 7                                      # tick 0 only stashes its sweep: six frames, one file of four and two left for destroy()
    for i in range(ticks):
        ca, cb = a.run_step(synth.agent_inputs(i, sc), i * 0.05), b.run_step(synth.agent_inputs(i, sc), i * 0.05)
        assert (ca.steer, ca.throttle, ca.brake) == (cb.steer, cb.throttle, cb.brake), i
        assert len(b.vizs) == 0 and len(clones) == i and len(a.vizs) == i % 4 and len(a.vizs.written) == i // 4
    assert sorted(os.listdir(out_dir)) == ["view_000002.avi"]
    a.destroy(); b.destroy()
    assert sorted(os.listdir(out_dir)) == ["view_000002.avi", "view_000006.avi"] and len(a.vizs) == 0
    want = [M.jpeg_encode_numpy(c.cpu().numpy(), 80) for c in clones]
    head = M.jpeg_header(160, 1146, 80, M.DEFAULT_RESTART_MCUS)
    for name, part in (("view_000002.avi", want[:4]), ("view_000006.avi", want[4:])):
        info, got = M.read_avi(str(out_dir / name))
        assert (info["microsec_per_frame"], info["total_frames"], info["width"], info["height"], info["closed"]) == (50000, len(part), 1146, 160, True)
        assert len(got) == len(part)
        for g, w in zip(got, part):
            assert g[:len(head)] == head and g[-2:] == M.EOI and g == w


def test_agent_with_the_default_config_never_encodes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = []
    real = ops.jpeg_encode
    monkeypatch.setattr(ops, "jpeg_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    a, sc = _agent(tmp_path, "default")
    assert (a.debug_view, a.debug_view_format, a.debug_view_quality) == (False, "npy", 90)
    for i in range(3):
        a.run_step(synth.agent_inputs(i, sc), i * 0.05)
    assert a.flush_data() is None
    a.destroy()
    c, sc = _agent(tmp_path, "npy", debug_view=True, debug_view_flush=2, debug_view_dir=str(tmp_path / "npy"))
    for i in range(3):
        c.run_step(synth.agent_inputs(i, sc), i * 0.05)
    c.destroy()
    assert not calls and sorted(os.listdir(tmp_path / "npy")) == ["view_000002.npy"]
    assert not [f for _, _, fs in os.walk(tmp_path) for f in fs if f.endswith(".avi")]
