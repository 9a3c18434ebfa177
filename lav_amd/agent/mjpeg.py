"""Motion-JPEG in an AVI container for the agent's debug view: the stream format, its NumPy specification and the container.

The reference ends a drive with wandb.Video(..., fps=20, format='mp4') (team_code_v2/lav_agent_fast.py:160-167, 355-358); this project
writes one self-contained JPEG per frame into an AVI file instead.  jpeg_encode_numpy is the specification; lav_jpeg_encode
(csrc/jpeg.hip, ops.jpeg_encode) produces the same entropy-coded scan on the device, byte for byte (tests/test_gpu_mjpeg.py).
Written from ITU-T T.81 and the AVI (RIFF) definition; no float is used anywhere on the encode path.

The JPEG stream
  SOI, APP0 (JFIF 1.01, no density, no thumbnail), one DQT with both tables, SOF0, four DHT, DRI, SOS, the scan, EOI.
  Baseline sequential DCT, 8 bit, three components Y, Cb, Cr with sampling 2x2, 1x1, 1x1: an MCU is 16 x 16 pixels and holds six
  8 x 8 blocks in the order Y00 Y01 Y10 Y11 Cb Cr.  A frame whose height or width is no multiple of 16 is padded by repeating its
  last row and column ON THE RGB IMAGE; SOF0 carries the true size.
  Colour: full-range BT.601 in 16-bit fixed point,
      Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
      Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16          (all three lie in 0 .. 255 without clamping)
  Chroma: (a + b + c + d + 2) >> 2 of the 2 x 2 block's four Cb (Cr) values.  Level shift: minus 128.
  Forward DCT: the 8 x 8 matrix DCT_MATRIX[u][x] = round(2^14 * C(u) / 2 * cos((2 x + 1) u pi / 16)), C(0) = 1 / sqrt 2 (the integers
  of COS16, written out below), applied to
  the rows and then to the columns in int32:
      t[y][u] = (sum_x DCT_MATRIX[u][x] * s[y][x] + 2^9) >> 10                 (4 fraction bits are kept; |t| < 2^13)
      S[v][u] = (sum_y DCT_MATRIX[v][y] * t[y][u] + 2^14) >> 15                (|sum| < 2^30; S is 8 times the coefficient)
  with >> the arithmetic shift (floor).  The coefficient keeps 3 fraction bits up to the division, so that it is rounded once.  The integers of DCT_MATRIX are part of the format: the kernel reads them from the table
  device_tables() builds, it computes no cosine.
  Quantisation: sign(S) * ((|S| + 4 Q) / (8 Q)), i.e. rounded division, half away from zero.  Q: the two tables of T.81 Annex K.1 and
  K.2 scaled by the IJG rule (quality < 50: 5000 / quality, else 200 - 2 quality; (base * scale + 50) / 100 cut to 1 .. 255), for
  quality 1 .. 100, written in DQT in zigzag order.
  Huffman: the four typical tables of Annex K.3, written in DHT; no optimisation pass.
  Restart: DRI carries restart_mcus (1 .. MAX_RESTART_MCUS, default DEFAULT_RESTART_MCUS); interval k (all but the last) is followed
  by RST(k mod 8), the DC predictors are zero at the start of an interval, the last byte of an interval is filled with 1-bits and
  every 0xFF of the entropy-coded data is followed by a stuffed 0x00.

The container
  RIFF 'AVI ': LIST hdrl (avih; LIST strl (strh vids / MJPG; strf BITMAPINFOHEADER, 24 bit, biCompression 'MJPG')), LIST movi of
  word-aligned '00dc' chunks, idx1.  The sizes and the frame counts are patched by close(); a file that was never closed still holds
  every frame that add() returned from, and read_avi recovers them by walking the '00dc' chunks.  No OpenDML: the caller keeps a file
  below 2 GB (the recorder writes at most debug_view_flush frames into one).

    python -m lav_amd.agent.mjpeg FILE.avi --frames DIR       # prints the header fields, writes DIR/frame_%06d.jpg
"""
from __future__ import annotations

import os
import struct

import numpy as np

DEFAULT_RESTART_MCUS = 10       # 60 blocks: one 64-lane wave codes an interval, one lane a block
MAX_RESTART_MCUS = 10           # more would not fit a wave; the kernel and the specification share the limit
DCT_BITS, PASS1_BITS, OUT_BITS = 14, 4, 3
# the most bits a block can take: its DC code (at most 11 bits, chroma category 11) and 11 magnitude bits, and per AC coefficient the
# longest code (16) and 10 magnitude bits - a ZRL (11 bits for 16 zeros) or an EOB (4 bits for at least one) costs less per coefficient
MAX_BLOCK_BITS = 11 + 11 + 63 * (16 + 10)
BLOCKS_PER_MCU = 6

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  np.int32)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32, np.int32)


def _zigzag() -> np.ndarray:
    """ZIGZAG[k]: the natural (row * 8 + column) index of the k-th coefficient in zigzag order."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, np.int32)


ZIGZAG = _zigzag()


def _rng(a, b):
    return list(range(a, b + 1))


# Annex K.3: (number of codes of each length 1 .. 16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _rng(0, 11))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _rng(0, 11))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a] + _rng(0x16, 0x1a) + _rng(0x25, 0x2a)
           + _rng(0x34, 0x3a) + _rng(0x43, 0x4a) + _rng(0x53, 0x5a) + _rng(0x63, 0x6a) + _rng(0x73, 0x7a) + _rng(0x83, 0x8a) + _rng(0x92, 0x9a)
           + _rng(0xa2, 0xaa) + _rng(0xb2, 0xba) + _rng(0xc2, 0xca) + _rng(0xd2, 0xda) + _rng(0xe1, 0xea) + _rng(0xf1, 0xfa))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a]
             + _rng(0x26, 0x2a) + _rng(0x35, 0x3a) + _rng(0x43, 0x4a) + _rng(0x53, 0x5a) + _rng(0x63, 0x6a) + _rng(0x73, 0x7a) + _rng(0x82, 0x8a)
             + _rng(0x92, 0x9a) + _rng(0xa2, 0xaa) + _rng(0xb2, 0xba) + _rng(0xc2, 0xca) + _rng(0xd2, 0xda) + _rng(0xe2, 0xea) + _rng(0xf2, 0xfa))
HUFFMAN = ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))       # (Tc << 4 | Th, table) in DHT order


def _codes(table) -> np.ndarray:
    """(256, 2) int32: code and length of every symbol (length 0: the symbol has no code), by T.81 Annex C."""
    bits, vals = table
    assert sum(bits) == len(vals)
    out = np.zeros((256, 2), np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


COS16 = (8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598, 0)      # round(2^13 cos(k pi / 16)), k = 0 .. 8


def _dct_matrix() -> np.ndarray:
    """DCT_MATRIX[u][x] = round(2^14 C(u) / 2 cos((2 x + 1) u pi / 16)) from the nine integers of COS16: the angle folded into the
    first quadrant; row 0 is 2^13 / sqrt 2 = COS16[4]."""
    out = np.zeros((8, 8), np.int32)
    for u in range(8):
        for x in range(8):
            a = (2 * x + 1) * u % 32
            a = 32 - a if a > 16 else a
            out[u, x] = COS16[4] if u == 0 else (-COS16[16 - a] if a > 8 else COS16[a])
    return out


DCT_MATRIX = _dct_matrix()

# device_tables(): offsets in int32 words
T_QUANT, T_DCT, T_ZIGZAG, T_DC, T_AC, T_WORDS = 0, 128, 192, 256, 288, 800


def _check(quality, restart_mcus):
    if not (isinstance(quality, (int, np.integer)) and 1 <= quality <= 100):
        raise ValueError(f"mjpeg: quality {quality!r} is not an integer in 1 .. 100")
    if not (isinstance(restart_mcus, (int, np.integer)) and 1 <= restart_mcus <= MAX_RESTART_MCUS):
        raise ValueError(f"mjpeg: restart_mcus {restart_mcus!r} is not an integer in 1 .. {MAX_RESTART_MCUS}")


def _check_size(h, w):
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError(f"mjpeg: frame size {h} x {w} outside 1 .. 16384")


def quant_tables(quality: int) -> tuple:
    """(luma, chroma): (64,) int32 in natural (row-major) order, the Annex K tables scaled by the IJG quality rule."""
    _check(quality, 1)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int32) for base in (LUMA_Q, CHROMA_Q))


def device_tables(quality: int) -> np.ndarray:
    """The (T_WORDS,) int32 table lav_jpeg_encode reads: [0, 128) the two quantisation tables in natural order, [128, 192)
    DCT_MATRIX, [192, 256) ZIGZAG, [256, 272) and [272, 288) code | length << 16 of the luma and chroma DC categories, [288, 544)
    and [544, 800) the same of the luma and chroma AC symbols run << 4 | size."""
    ql, qc = quant_tables(quality)
    out = np.zeros(T_WORDS, np.int32)
    out[0:64], out[64:128], out[T_DCT:T_DCT + 64], out[T_ZIGZAG:T_ZIGZAG + 64] = ql, qc, DCT_MATRIX.reshape(-1), ZIGZAG
    pack = lambda t: _codes(t)[:, 0] | _codes(t)[:, 1] << 16      # noqa: E731
    out[T_DC:T_DC + 16], out[T_DC + 16:T_DC + 32] = pack(DC_LUMA)[:16], pack(DC_CHROMA)[:16]
    out[T_AC:T_AC + 256], out[T_AC + 256:T_AC + 512] = pack(AC_LUMA), pack(AC_CHROMA)
    return out


def mcu_grid(h: int, w: int) -> tuple:
    return (h + 15) // 16, (w + 15) // 16


def intervals(h: int, w: int, restart_mcus: int) -> int:
    my, mx = mcu_grid(h, w)
    return (my * mx + restart_mcus - 1) // restart_mcus


def interval_capacity(mcus: int) -> int:
    """The most bytes the entropy-coded data of an interval of `mcus` MCUs can take, every byte stuffed."""
    return 2 * ((mcus * BLOCKS_PER_MCU * MAX_BLOCK_BITS + 7) // 8)


def scan_capacity(h: int, w: int, restart_mcus: int = DEFAULT_RESTART_MCUS) -> int:
    """A bound on the bytes of one frame's scan, RST markers included: every block MAX_BLOCK_BITS long, every byte stuffed."""
    _check(90, restart_mcus)
    _check_size(h, w)
    my, mx = mcu_grid(h, w)
    n = intervals(h, w, restart_mcus)
    last = my * mx - (n - 1) * restart_mcus
    return (n - 1) * (interval_capacity(restart_mcus) + 2) + interval_capacity(last)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(h: int, w: int, quality: int = 90, restart_mcus: int = DEFAULT_RESTART_MCUS) -> bytes:
    """SOI up to and including SOS: what precedes the scan."""
    _check(quality, restart_mcus)
    _check_size(h, w)
    ql, qc = quant_tables(quality)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0)),
           _segment(0xDB, b"\x00" + bytes(ql[ZIGZAG].astype(np.uint8)) + b"\x01" + bytes(qc[ZIGZAG].astype(np.uint8))),
           _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))]
    for ident, (bits, vals) in HUFFMAN:
        out.append(_segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", restart_mcus)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


EOI = b"\xff\xd9"


def coefficients_numpy(frame, quality: int = 90) -> np.ndarray:
    """(MCUs, 6, 64) int16: the quantised coefficients of every block in zigzag order, MCUs in raster order - what the first launch
    of lav_jpeg_encode leaves in its workspace."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"mjpeg: frame must be (h, w, 3) uint8, got {frame.dtype} {frame.shape}")
    h, w = frame.shape[:2]
    _check_size(h, w)
    ql, qc = quant_tables(quality)
    my, mx = mcu_grid(h, w)
    rgb = np.pad(frame, ((0, my * 16 - h), (0, mx * 16 - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2      # noqa: E731
    # blocks: (my, mx, 6, 8, 8)
    yb = (y - 128).reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, 4, 8, 8)
    cbb, crb = ((half(c) - 128).reshape(my, 8, mx, 8).transpose(0, 2, 1, 3)[:, :, None] for c in (cb, cr))
    s = np.concatenate([yb, cbb, crb], axis=2)
    m = DCT_MATRIX.astype(np.int64)
    t = (np.einsum("ux,...yx->...yu", m, s) + (1 << (DCT_BITS - PASS1_BITS - 1))) >> (DCT_BITS - PASS1_BITS)
    S = (np.einsum("vy,...yu->...vu", m, t) + (1 << (DCT_BITS + PASS1_BITS - OUT_BITS - 1))) >> (DCT_BITS + PASS1_BITS - OUT_BITS)
    q = np.stack([ql] * 4 + [qc] * 2).reshape(6, 8, 8).astype(np.int64)
    S = np.sign(S) * ((np.abs(S) + (q << (OUT_BITS - 1))) // (q << OUT_BITS))
    return S.reshape(my * mx, 6, 64)[:, :, ZIGZAG].astype(np.int16)


STATS = ("stuffed", "zrl", "eob", "ac_symbols", "dc_category", "ac_category", "dc_nonzero_after_first", "intervals", "blocks")


def scan_numpy(frame, quality: int = 90, restart_mcus: int = DEFAULT_RESTART_MCUS, stats: bool = False):
    """The entropy-coded scan of the frame (RST markers included, no header, no EOI): what lav_jpeg_encode writes.  With stats, also
    a dict of what the stream exercised (STATS): stuffed bytes, ZRL and EOB symbols, other AC symbols, the largest DC and AC magnitude
    categories, the DC differences other than zero that are not the first of their component in an interval, intervals, blocks."""
    _check(quality, restart_mcus)
    coef = coefficients_numpy(frame, quality).astype(np.int64)
    dc = (_codes(DC_LUMA).tolist(), _codes(DC_CHROMA).tolist())        # Python integers: the bit string is one big int
    ac = (_codes(AC_LUMA).tolist(), _codes(AC_CHROMA).tolist())
    st = dict.fromkeys(STATS, 0)
    out = []
    nmcu = len(coef)
    n_int = (nmcu + restart_mcus - 1) // restart_mcus
    for k in range(n_int):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for mcu in range(k * restart_mcus, min((k + 1) * restart_mcus, nmcu)):
            for blk in range(6):
                comp = max(blk - 3, 0)
                z = coef[mcu, blk]
                diff = int(z[0]) - pred[comp]
                if diff and (mcu > k * restart_mcus or (comp == 0 and blk > 0)):
                    st["dc_nonzero_after_first"] += 1
                pred[comp] = int(z[0])
                size = abs(diff).bit_length()
                st["dc_category"] = max(st["dc_category"], size)
                code, length = dc[comp > 0][size]
                acc, nbits = (acc << length | code) << size | ((diff if diff >= 0 else diff + (1 << size) - 1) & ((1 << size) - 1)), nbits + length + size
                last = 0
                for pos in np.flatnonzero(z[1:]) + 1:
                    run = int(pos) - last - 1
                    while run > 15:
                        code, length = ac[comp > 0][0xF0]
                        acc, nbits = acc << length | code, nbits + length
                        st["zrl"] += 1
                        run -= 16
                    v = int(z[pos])
                    size = abs(v).bit_length()
                    st["ac_category"] = max(st["ac_category"], size)
                    st["ac_symbols"] += 1
                    code, length = ac[comp > 0][run << 4 | size]
                    acc, nbits = (acc << length | code) << size | ((v if v >= 0 else v + (1 << size) - 1) & ((1 << size) - 1)), nbits + length + size
                    last = int(pos)
                if last < 63:
                    code, length = ac[comp > 0][0x00]
                    acc, nbits = acc << length | code, nbits + length
                    st["eob"] += 1
                st["blocks"] += 1
        pad = -nbits % 8
        data = (acc << pad | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big")
        st["stuffed"] += data.count(b"\xff")
        out.append(data.replace(b"\xff", b"\xff\x00"))
        if k + 1 < n_int:
            out.append(bytes([0xFF, 0xD0 + k % 8]))
    st["intervals"] = n_int
    scan = b"".join(out)
    return (scan, st) if stats else scan


def jpeg_encode_numpy(frame, quality: int = 90, restart_mcus: int = DEFAULT_RESTART_MCUS, stats: bool = False):
    """The specification: the whole JPEG stream of an (h, w, 3) uint8 RGB frame - jpeg_header(...) + scan_numpy(...) + EOI."""
    frame = np.asarray(frame)
    got = scan_numpy(frame, quality, restart_mcus, stats)
    head = jpeg_header(frame.shape[0], frame.shape[1], quality, restart_mcus)
    return (head + got[0] + EOI, got[1]) if stats else head + got + EOI


# ---------------------------------------------------------------------------------------------- AVI
_HEADER_BYTES = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 12      # RIFF, LIST hdrl, avih, LIST strl, strh, strf, LIST movi: 224


class AviWriter:
    """One MJPG video stream.  add() appends a '00dc' chunk and flushes it to the file; close() writes idx1 and patches the sizes."""

    def __init__(self, path: str, h: int, w: int, fps: float = 20.0):
        if not (fps > 0 and h >= 1 and w >= 1):
            raise ValueError(f"AviWriter: {h} x {w} at {fps} frames per second")
        self.path, self.h, self.w, self.fps = path, int(h), int(w), float(fps)
        self.index = []            # (offset from the 'movi' fourcc, length)
        self.largest = 0
        self.f = open(path, "wb")
        self.f.write(self._header(0, 0))
        self.f.flush()

    def _header(self, movi_bytes: int, riff_bytes: int) -> bytes:
        n = len(self.index)
        usec = int(round(1e6 / self.fps))
        rate, scale = int(round(self.fps * 1000)), 1000
        avih = struct.pack("<14I", usec, int(self.largest * self.fps), 0, 0x10, n, 0, 1, self.largest, self.w, self.h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, self.largest, 0xFFFFFFFF, 0, 0, 0, self.w, self.h)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.w, self.h, 1, 24, b"MJPG", self.w * self.h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"
        assert len(head) == _HEADER_BYTES
        return head

    def add(self, jpeg: bytes):
        if self.f is None:
            raise ValueError("AviWriter: the file is closed")
        jpeg = bytes(jpeg)
        if self.f.tell() + len(jpeg) + 16 * (len(self.index) + 2) + 16 > 0x7FFFFFFF:
            raise ValueError("AviWriter: the file would pass 2 GB (no OpenDML)")
        self.index.append((self.f.tell() - (_HEADER_BYTES - 4), len(jpeg)))
        self.largest = max(self.largest, len(jpeg))
        self.f.write(b"00dc" + struct.pack("<I", len(jpeg)) + jpeg + b"\0" * (len(jpeg) & 1))
        self.f.flush()

    def close(self):
        if self.f is None:
            return
        movi_bytes = self.f.tell() - (_HEADER_BYTES - 4)
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self.index)
        self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        riff_bytes = self.f.tell() - 8
        self.f.seek(0)
        self.f.write(self._header(movi_bytes, riff_bytes))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_avi(path: str) -> tuple:
    """(info, frames): the header fields (microsec_per_frame, total_frames, width, height, handler, compression, bit_count, scale,
    rate, closed) and the bytes of every '00dc' chunk, walked from the start of movi - the index is not needed, so a file that was
    never closed (sizes still zero, no idx1) yields the frames it holds; a chunk cut short by the end of the file is dropped."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < _HEADER_BYTES or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not an AVI file")
    pos, info, movi = 12, {}, None
    while pos + 8 <= len(data) and movi is None:
        fourcc, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        if fourcc == b"LIST":
            kind = data[pos + 8:pos + 12]
            if kind == b"movi":
                movi = (pos + 12, size)
            pos += 12                       # descend into hdrl / strl
            continue
        body = data[pos + 8:pos + 8 + size]
        if fourcc == b"avih":
            v = struct.unpack_from("<14I", body)
            info.update(microsec_per_frame=v[0], total_frames=v[4], streams=v[6], width=v[8], height=v[9])
        elif fourcc == b"strh":
            info.update(type=body[0:4].decode("latin1"), handler=body[4:8].decode("latin1"), scale=struct.unpack_from("<I", body, 20)[0],
                        rate=struct.unpack_from("<I", body, 24)[0], length=struct.unpack_from("<I", body, 32)[0])
        elif fourcc == b"strf":
            info.update(compression=body[16:20].decode("latin1"), bit_count=struct.unpack_from("<H", body, 14)[0])
        pos += 8 + size + (size & 1)
    if movi is None:
        raise ValueError(f"{path}: no movi list")
    start, size = movi
    info["closed"] = size != 0
    end = start + size - 4 if size else len(data)
    frames, pos = [], start
    while pos + 8 <= end and data[pos:pos + 4] == b"00dc":
        n = struct.unpack_from("<I", data, pos + 4)[0]
        if pos + 8 + n > len(data):
            break
        frames.append(data[pos + 8:pos + 8 + n])
        pos += 8 + n + (n & 1)
    return info, frames


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m lav_amd.agent.mjpeg", description="Print an MJPEG/AVI file's header and split it into JPEG files.")
    ap.add_argument("file")
    ap.add_argument("--frames", metavar="DIR", help="write DIR/frame_%%06d.jpg")
    args = ap.parse_args(argv)
    info, frames = read_avi(args.file)
    for k, v in info.items():
        print(f"{k}: {v}")
    print(f"frames: {len(frames)}  bytes: {sum(map(len, frames))}")
    if args.frames:
        os.makedirs(args.frames, exist_ok=True)
        for i, fr in enumerate(frames):
            with open(os.path.join(args.frames, f"frame_{i:06d}.jpg"), "wb") as f:
                f.write(fr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
