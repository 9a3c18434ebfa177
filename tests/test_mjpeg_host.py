"""lav_amd.agent.mjpeg on the CPU: the JPEG stream's structure walked with struct code of this file, its decoding by an independent
decoder (Pillow), its quality and size against Pillow's own encoder at the same tables, the code paths the chosen inputs exercise,
the AVI container parsed by hand, the recorder on CPU tensors and the capacity bound against the library's.

Margins against Pillow's encoder (libjpeg-turbo), measured here on the CPU over the three inputs at qualities 50 and 90 (DESIGN
4.5c): the specification's PSNR was at worst 0.139 dB below Pillow's (the gradient at quality 90, at 48.8 dB; elsewhere within 0.03 dB)
and its scan at worst 0.152 % longer (the same input; elsewhere within 0.12 %, shorter on three of six).  The two encoders differ only
in the rounding of two integer DCTs, two colour conversions and the chroma mean.  The bars are twice the measured gaps, 0.28 dB and
0.31 %, inside the conditions of 0.5 dB and 5 % beyond which the specification would count as wrong."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from lav_amd import _lib
from lav_amd.agent import debug_view as V
from lav_amd.agent import mjpeg as M
from tests.mjpeg_util import CASES, QUALITIES, SIZES, case_frame, debug_frame, gradient, lowpass_noise, walk_markers

PSNR_MARGIN_DB, SIZE_MARGIN = 0.28, 0.0031


# ---------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("h,w,restart", SIZES)
def test_stream_structure(h, w, restart):
    frame = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    stream, st = M.jpeg_encode_numpy(frame, 90, restart, stats=True)
    segs, scan = walk_markers(stream)
    assert [m for m, _ in segs] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA, 0xD9]
    body = dict((m, p) for m, p in segs if m != 0xC4)
    assert body[0xE0][:5] == b"JFIF\0"
    precision, hh, ww, ncomp = struct.unpack(">BHHB", body[0xC0][:6])
    assert (precision, hh, ww, ncomp) == (8, h, w, 3)
    assert [tuple(body[0xC0][6 + 3 * i:9 + 3 * i]) for i in range(3)] == [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    assert len(body[0xDB]) == 130 and body[0xDB][0] == 0 and body[0xDB][65] == 1
    ql, qc = M.quant_tables(90)
    assert list(body[0xDB][1:65]) == list(ql[M.ZIGZAG]) and list(body[0xDB][66:]) == list(qc[M.ZIGZAG])
    assert sorted(p[0] for m, p in segs if m == 0xC4) == [0x00, 0x01, 0x10, 0x11]
    assert struct.unpack(">H", body[0xDD])[0] == restart
    assert body[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    # the scan: every 0xFF is stuffed or the expected restart marker
    n_int = -(-((h + 15) // 16) * ((w + 15) // 16) // restart)
    assert st["intervals"] == n_int == M.intervals(h, w, restart)
    seen, i = 0, 0
    while i < len(scan):
        if scan[i] == 0xFF:
            assert i + 1 < len(scan)
            if scan[i + 1] != 0:
                assert scan[i + 1] == 0xD0 + seen % 8, (i, scan[i + 1], seen)
                seen += 1
            i += 2
        else:
            i += 1
    assert seen == n_int - 1
    assert len(scan) <= M.scan_capacity(h, w, restart)
    assert scan == M.scan_numpy(frame, 90, restart) and stream == M.jpeg_header(h, w, 90, restart) + scan + M.EOI


def test_zigzag_and_tables():
    assert list(M.ZIGZAG[:10]) == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(M.ZIGZAG) == list(range(64)) and M.ZIGZAG[63] == 63
    ql, qc = M.quant_tables(50)
    assert list(ql) == list(M.LUMA_Q) and list(qc) == list(M.CHROMA_Q)
    assert set(M.quant_tables(100)[0]) == {1} and M.quant_tables(1)[0].max() == 255
    for table, n in ((M.DC_LUMA, 12), (M.DC_CHROMA, 12), (M.AC_LUMA, 162), (M.AC_CHROMA, 162)):
        assert sum(table[0]) == len(table[1]) == len(set(table[1])) == n
        codes = M._codes(table)
        used = [(int(c), int(l)) for c, l in codes if l]
        strings = sorted(format(c, f"0{l}b") for c, l in used)
        assert len(used) == n and not any(b.startswith(a) for a, b in zip(strings, strings[1:]))      # prefix-free
        assert "1" * 16 not in strings
    import math
    want = [[round(2 ** 14 * (math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8)] for u in range(8)]
    assert M.DCT_MATRIX.tolist() == want and M.DCT_MATRIX.dtype == np.int32
    t = M.device_tables(90)
    assert t.shape == (M.T_WORDS,) and t.dtype == np.int32 and list(t[M.T_DCT:M.T_DCT + 8]) == [5793] * 8
    for q in (0, 101, 50.0, None):
        with pytest.raises(ValueError):
            M.quant_tables(q)
    for r in (0, M.MAX_RESTART_MCUS + 1, -1):
        with pytest.raises(ValueError):
            M.jpeg_encode_numpy(np.zeros((16, 16, 3), np.uint8), 90, r)
    for bad in (np.zeros((16, 16, 4), np.uint8), np.zeros((16, 16, 3), np.float32), np.zeros((16, 16), np.uint8)):
        with pytest.raises(ValueError):
            M.jpeg_encode_numpy(bad)


# ---------------------------------------------------------------------------------------------- an independent decoder
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("h,w,restart", SIZES)
def test_pillow_decodes(h, w, restart, quality):
    Image = pytest.importorskip("PIL.Image")
    frame = debug_frame() if (h, w) == (160, 1146) else gradient(h, w)
    im = Image.open(io.BytesIO(M.jpeg_encode_numpy(frame, quality, restart)))
    im.load()
    assert im.size == (w, h) and im.mode == "RGB" and im.format == "JPEG"
    got = np.asarray(im).astype(np.float64)
    # a decoder that lost its place in the stream (a wrong code, a wrong restart) gives garbage, not a close image
    assert np.abs(got - frame).mean() < (12 if quality >= 50 else 20)


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def _pillow_encode(frame, quality, restart):
    """Pillow's encoder with this module's tables; Pillow's table order is found by a round trip, not assumed."""
    from PIL import Image
    ql, qc = M.quant_tables(quality)
    for order in (np.arange(64), M.ZIGZAG):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", qtables=[list(map(int, ql[order])), list(map(int, qc[order]))], subsampling="4:2:0", optimize=False,
                                    restart_marker_blocks=restart)
        dqt = b"".join(p for m, p in walk_markers(buf.getvalue())[0] if m == 0xDB)
        tables = {dqt[i]: list(dqt[i + 1:i + 65]) for i in range(0, len(dqt), 65)}
        if tables == {0: list(ql[M.ZIGZAG]), 1: list(qc[M.ZIGZAG])}:       # the file holds this module's tables, in the file's zigzag order
            back = Image.open(io.BytesIO(buf.getvalue())).quantization
            assert sorted(back[0]) == sorted(ql) and sorted(back[1]) == sorted(qc)
            return buf.getvalue()
    raise AssertionError("neither table order makes Pillow write this module's tables")


@pytest.mark.parametrize("quality", [50, 90])
@pytest.mark.parametrize("name", ["debug", "gradient", "lowpass"])
def test_quality_and_size_against_pillow(name, quality):
    Image = pytest.importorskip("PIL.Image")
    frame = {"debug": debug_frame, "gradient": lambda: gradient(96, 208), "lowpass": lambda: lowpass_noise(96, 208, seed=1)}[name]()
    mine = M.jpeg_encode_numpy(frame, quality, M.DEFAULT_RESTART_MCUS)
    ref = _pillow_encode(frame, quality, M.DEFAULT_RESTART_MCUS)
    dec = lambda s: np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))          # noqa: E731
    p_mine, p_ref = _psnr(dec(mine), frame), _psnr(dec(ref), frame)
    # the scans alone: the two headers differ (Pillow writes its DQT and DHT segments its own way)
    n_mine, n_ref = len(walk_markers(mine)[1]), len(walk_markers(ref)[1])
    print(f"{name} q{quality}: PSNR {p_mine:.3f} dB against Pillow's {p_ref:.3f} ({p_mine - p_ref:+.3f}), scan {n_mine} bytes against {n_ref} ({n_mine / n_ref - 1:+.4%})")
    assert p_mine >= p_ref - PSNR_MARGIN_DB
    assert n_mine <= n_ref * (1 + SIZE_MARGIN)


# ---------------------------------------------------------------------------------------------- code paths
def test_inputs_exercise_the_code_paths():
    st = {name: M.jpeg_encode_numpy(case_frame(name), q, r, stats=True)[1] for name, (q, r) in CASES.items()}
    assert st["noise"]["stuffed"] > 0
    assert st["dots"]["zrl"] > 0
    flat = st["flat"]
    assert flat["ac_symbols"] == 0 and flat["zrl"] == 0 and flat["eob"] == flat["blocks"] > 6 and flat["dc_nonzero_after_first"] == 0 and flat["intervals"] > 1
    assert st["mcus"]["dc_category"] == 11
    assert st["checker"]["ac_category"] == 10
    for s in st.values():
        assert s["dc_category"] <= 11 and s["ac_category"] <= 10


def test_capacity_is_a_bound_and_equals_the_library():
    lib = _lib.load()                      # loads on the CPU (tests/test_capi_host.py)
    for h, w, r in SIZES + [(1, 1, 1), (160, 1146, 3), (16384, 16, 10)]:
        assert M.scan_capacity(h, w, r) == lib.lav_jpeg_scan_capacity(h, w, r)
    for bad in ((0, 16, 10), (16, 16, 0), (16, 16, M.MAX_RESTART_MCUS + 1), (16385, 16, 1)):
        assert lib.lav_jpeg_scan_capacity(*bad) == 0 and lib.lav_jpeg_workspace_bytes(1, *bad) == 0
        with pytest.raises(ValueError):
            M.scan_capacity(*bad)
    assert lib.lav_jpeg_workspace_bytes(0, 16, 16, 1) == 0
    # no symbol takes more than 16 + 11 bits, the DC code no more than 11: the per-block figure the bound is built from
    longest_ac = max(int(l) for t in (M.AC_LUMA, M.AC_CHROMA) for _, l in M._codes(t))
    longest_dc = max(int(l) for t in (M.DC_LUMA, M.DC_CHROMA) for _, l in M._codes(t))
    assert M.MAX_BLOCK_BITS == longest_dc + 11 + 63 * (longest_ac + 10) == 1660
    # the noisiest stream of the cases stays far below it
    scan = M.scan_numpy(case_frame("noise"), *CASES["noise"])
    assert len(scan) <= M.scan_capacity(*case_frame("noise").shape[:2], CASES["noise"][1])


def test_encode_arguments_are_checked_on_the_host():
    """lav_jpeg_encode checks every argument before its first launch: with no device in sight a refused call must fail on its
    arguments (LAV_EINVAL / LAV_EWORKSPACE), not on the HIP runtime."""
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data % 256)
    cap = M.scan_capacity(16, 16, 10)
    good = [p, 1, 16, 16, 48, p, 10, p, cap, p, p, 1 << 15, None]
    for at, value in ((0, None), (1, 0), (2, 0), (3, 16385), (4, 47), (5, None), (6, 0), (6, 11), (7, None), (8, cap - 1), (9, None), (10, None), (10, p + 4)):
        args = list(good)
        args[at] = value
        assert lib.lav_jpeg_encode(*args) == -1, (at, value)
        assert b"lav_jpeg_encode" in lib.lav_last_error()
    args = list(good)
    args[11] = 64
    assert lib.lav_jpeg_encode(*args) == -3


# ---------------------------------------------------------------------------------------------- AVI
def _chunks(data, pos, end):
    while pos + 8 <= end:
        fourcc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        yield fourcc, pos, size
        pos += 8 + size + (size & 1)


def test_avi_container(tmp_path):
    rng = np.random.default_rng(0)
    frames = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (101, 40, 7, 250, 33)]       # odd lengths: padding
    path = tmp_path / "five.avi"
    avi = M.AviWriter(str(path), 160, 1146, fps=10.0)
    for f in frames:
        avi.add(f)
    # not closed yet: the frames are in the file and recoverable
    info, got = M.read_avi(str(path))
    assert got == frames and info["closed"] is False and (info["width"], info["height"]) == (1146, 160)
    avi.close()
    avi.close()
    data = path.read_bytes()
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = {(f, data[p + 8:p + 12] if f == b"LIST" else b""): (p, s) for f, p, s in _chunks(data, 12, len(data))}
    assert list(top) == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", b"")]
    hp, hs = top[(b"LIST", b"hdrl")]
    hdrl = {(f, data[p + 8:p + 12] if f == b"LIST" else b""): (p, s) for f, p, s in _chunks(data, hp + 12, hp + 8 + hs)}
    assert list(hdrl) == [(b"avih", b""), (b"LIST", b"strl")]
    ap, asz = hdrl[(b"avih", b"")]
    avih = struct.unpack_from("<14I", data, ap + 8)
    assert asz == 56 and (avih[0], avih[4], avih[6], avih[8], avih[9]) == (100000, 5, 1, 1146, 160) and avih[3] & 0x10
    sp, ss = hdrl[(b"LIST", b"strl")]
    strl = {f: (p, s) for f, p, s in _chunks(data, sp + 12, sp + 8 + ss)}
    assert list(strl) == [b"strh", b"strf"]
    shp = strl[b"strh"][0] + 8
    assert data[shp:shp + 4] == b"vids" and data[shp + 4:shp + 8] == b"MJPG" and strl[b"strh"][1] == 56
    scale, rate, _, length = struct.unpack_from("<4I", data, shp + 20)
    assert rate / scale == 10.0 and length == 5
    sfp = strl[b"strf"][0] + 8
    size, bw, bh, planes, bits, comp = struct.unpack_from("<IiiHH4s", data, sfp)
    assert (size, bw, bh, planes, bits, comp) == (40, 1146, 160, 1, 24, b"MJPG") and strl[b"strf"][1] == 40
    mp, ms = top[(b"LIST", b"movi")]
    ip, isz = top[(b"idx1", b"")]
    assert isz == 16 * 5 and mp + 8 + ms == ip
    for i, f in enumerate(frames):
        ckid, flags, off, n = struct.unpack_from("<4sIII", data, ip + 8 + 16 * i)
        at = mp + 8 + off                            # offsets count from the 'movi' fourcc
        assert ckid == b"00dc" and flags & 0x10 and n == len(f) and at % 2 == 0
        assert data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == n and data[at + 8:at + 8 + n] == f
    assert [f for f, _, _ in _chunks(data, mp + 12, mp + 8 + ms)] == [b"00dc"] * 5
    info, got = M.read_avi(str(path))
    assert got == frames and info["closed"] is True
    assert (info["microsec_per_frame"], info["total_frames"], info["width"], info["height"], info["handler"], info["compression"], info["bit_count"]) \
        == (100000, 5, 1146, 160, "MJPG", "MJPG", 24)
    with pytest.raises(ValueError):
        avi.add(b"x")
    # a file cut in the middle of a chunk keeps the whole chunks before the cut
    cut = tmp_path / "cut.avi"
    cut.write_bytes(data[:top[(b"LIST", b"movi")][0] + 12 + 8 + 102 + 8 + 20])
    assert M.read_avi(str(cut))[1] == frames[:1]
    with pytest.raises(ValueError):
        M.read_avi(__file__)


def test_command_line_splits_a_file(tmp_path):
    frame = gradient(32, 48)
    jpeg = M.jpeg_encode_numpy(frame)
    with M.AviWriter(str(tmp_path / "v.avi"), 32, 48, fps=20.0) as avi:
        avi.add(jpeg)
        avi.add(jpeg)
    assert M.main([str(tmp_path / "v.avi"), "--frames", str(tmp_path / "out")]) == 0
    assert sorted(os.listdir(tmp_path / "out")) == ["frame_000000.jpg", "frame_000001.jpg"]
    assert (tmp_path / "out" / "frame_000001.jpg").read_bytes() == jpeg
    r = subprocess.run([sys.executable, "-m", "lav_amd.agent.mjpeg", str(tmp_path / "v.avi")], stdout=subprocess.PIPE, text=True, check=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "microsec_per_frame: 50000" in r.stdout and "frames: 2" in r.stdout


# ---------------------------------------------------------------------------------------------- the recorder on CPU tensors
def test_recorder_mjpeg_on_cpu_tensors(tmp_path):
    import torch
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (24, 40, 3), dtype=np.uint8) for _ in range(6)]
    rec = V.ViewRecorder(str(tmp_path / "v"), 4, format="mjpeg", quality=75, fps=5.0)
    for i, f in enumerate(frames):
        rec.append(torch.from_numpy(f), 10 + i)
        assert len(rec) == (i % 4) + 1 and len(rec.written) == (1 if i >= 4 else 0)
    assert [os.path.basename(p) for p in rec.written] == ["view_000010.avi"]
    assert rec.frames_jpeg() == [M.jpeg_encode_numpy(f, 75) for f in frames[4:]]
    assert rec.flush() == str(tmp_path / "v" / "view_000014.avi") and len(rec) == 0 and rec.flush() is None
    assert sorted(os.listdir(tmp_path / "v")) == ["view_000010.avi", "view_000014.avi"]
    for name, part in (("view_000010.avi", frames[:4]), ("view_000014.avi", frames[4:])):
        info, got = M.read_avi(str(tmp_path / "v" / name))
        assert got == [M.jpeg_encode_numpy(f, 75) for f in part]
        assert (info["microsec_per_frame"], info["total_frames"], info["width"], info["height"], info["closed"]) == (200000, len(part), 40, 24, True)
    with pytest.raises(RuntimeError):
        rec.frames()


def test_recorder_formats(tmp_path):
    with pytest.raises(ValueError):
        V.ViewRecorder(str(tmp_path), 4, format="mp4")
    with pytest.raises(ValueError):
        V.ViewRecorder(str(tmp_path), 4, format="mjpeg", quality=0)
    rec = V.ViewRecorder(str(tmp_path), 0, format="mjpeg")
    assert len(rec) == 0 and rec.flush() is None and os.listdir(tmp_path) == []
    assert V.ViewRecorder().format == "npy"


def test_recorder_npy_file_is_np_save_of_the_frames(tmp_path):
    """The npy format writes what it wrote before: np.save of the ring's frames.  (Its ring is pinned memory, which needs a device;
    the ring is set by hand here, as append() would leave it.)"""
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (3, 6, 10, 3), dtype=np.uint8)

    class Landed:
        def synchronize(self):
            pass

    import torch
    rec = V.ViewRecorder(str(tmp_path / "n"), 4, format="npy")
    rec.ring, rec.event, rec.count, rec.first_frame = torch.from_numpy(np.concatenate([frames, frames[:1]])), Landed(), 3, 7
    path = rec.flush()
    assert path == str(tmp_path / "n" / "view_000007.npy") and rec.written == [path] and len(rec) == 0
    buf = io.BytesIO()
    np.save(buf, frames)
    assert open(path, "rb").read() == buf.getvalue()
    with pytest.raises(RuntimeError):
        rec.frames_jpeg()
