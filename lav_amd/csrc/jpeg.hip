// Baseline JPEG scans of RGB frames that live in HBM (ABI 41): the device half of the agent's MJPEG recording.  The specification is
// lav_amd.agent.mjpeg.scan_numpy and the two agree in every byte (tests/test_gpu_mjpeg.py); the stream format - colour conversion,
// the integer DCT, quantisation, the Annex K tables, restart intervals - is stated there, and every constant of it (quantisers, the
// DCT matrix, the zigzag order, the Huffman codes) arrives in the table lav_amd.agent.mjpeg.device_tables builds.  All integer.
//
// One C call, three launches for a batch of frames, and every dependency between workgroups is a launch boundary:
//   k_jpeg_coef    one workgroup per 16 x 16 MCU, one thread per pixel: the pixel (edge pixels repeated past the frame) to Y, Cb, Cr in
//                  LDS, the 2 x 2 chroma means, both DCT passes from LDS, quantisation; leaves [MCU][6][64] int16 in zigzag order.
//   k_jpeg_entropy one wave per restart interval, one lane per 8 x 8 block.  A lane takes the DC of the block before it straight from
//                  the coefficients, so nothing runs along the interval; it writes its block's bit string into its own LDS row (whole
//                  codes shifted into a 64-bit accumulator, a 32-bit word stored whenever one is full).  A wave scan of the bit
//                  counts places every block; the lanes OR their rows, shifted, into the interval's image in LDS; the last byte is
//                  filled with 1-bits; then the bytes go to the interval's worst-case slot of the workspace 64 at a time, each at its
//                  index plus the number of 0xFF before it (a ballot per 64 bytes and a running count), a 0x00 behind every 0xFF.
//   k_jpeg_compact one workgroup per interval: it sums the lengths of the intervals before it (and their markers), copies its slot
//                  to that offset of the frame's scan, appends RST(k mod 8) or, as the last one, writes the frame's length.
#include "common.hpp"

namespace {
using namespace lav;
constexpr int MAX_RESTART = 10;                      // lav_amd.agent.mjpeg.MAX_RESTART_MCUS: 60 blocks, one wave
constexpr int BLOCK_BITS = 11 + 11 + 63 * 26;        // MAX_BLOCK_BITS
constexpr int ROW_WORDS = (BLOCK_BITS + 31) / 32 + 1;      // 53: a lane's row (odd: the lanes' rows start on different banks)
constexpr int IMAGE_WORDS = (MAX_RESTART * 6 * BLOCK_BITS + 31) / 32 + 2;
constexpr int T_DCT = 128, T_ZIGZAG = 192, T_DC = 256, T_AC = 288;
constexpr int LIMIT = 16384;

__host__ __device__ inline long long interval_capacity(int mcus) { return 2 * (((long long)mcus * 6 * BLOCK_BITS + 7) / 8); }

struct Shape {
    int n, h, w, row_stride, mx, mcus, restart, intervals;
    long long slot;                                  // bytes of an interval's slot in the workspace
};

__global__ __launch_bounds__(256) void k_jpeg_coef(const unsigned char *__restrict__ frames, const int *__restrict__ tables, Shape s,
                                                   short *__restrict__ coef) {
    __shared__ int s_dct[64], s_zz[64], s_q[128];
    __shared__ short s_pix[6][64];                   // level-shifted samples of the six blocks
    __shared__ short s_c[2][16][16];                 // full-resolution Cb, Cr
    __shared__ int s_t[6][64];                       // after the row pass: [block][y][u]
    const int tid = threadIdx.x, mcu = blockIdx.x, frame = blockIdx.y;
    if (tid < 64) { s_dct[tid] = tables[T_DCT + tid]; s_zz[tid] = tables[T_ZIGZAG + tid] & 63; }
    if (tid < 128) s_q[tid] = max(tables[tid], 1);
    const int py = tid >> 4, px = tid & 15;
    const int y = min((mcu / s.mx) * 16 + py, s.h - 1), x = min((mcu % s.mx) * 16 + px, s.w - 1);
    const unsigned char *p = frames + ((size_t)frame * s.h + y) * s.row_stride + (size_t)x * 3;
    const int r = p[0], g = p[1], b = p[2];
    s_pix[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = (short)(((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128);
    s_c[0][py][px] = (short)((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16);
    s_c[1][py][px] = (short)((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16);
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 6, cy = (tid & 63) >> 3, cx = tid & 7;
        s_pix[4 + c][tid & 63] = (short)(((s_c[c][2 * cy][2 * cx] + s_c[c][2 * cy][2 * cx + 1] + s_c[c][2 * cy + 1][2 * cx] + s_c[c][2 * cy + 1][2 * cx + 1] + 2) >> 2) - 128);
    }
    __syncthreads();
    for (int i = tid; i < 384; i += 256) {           // t[b][y][u] = sum_x D[u][x] s[b][y][x]
        const int blk = i >> 6, yy = (i & 63) >> 3, u = i & 7;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += s_dct[u * 8 + k] * s_pix[blk][yy * 8 + k];
        s_t[blk][yy * 8 + u] = (acc + (1 << 9)) >> 10;
    }
    __syncthreads();
    short *out = coef + ((size_t)frame * s.mcus + mcu) * 384;
    for (int i = tid; i < 384; i += 256) {           // zigzag position k of block b: S[v][u] = sum_y D[v][y] t[b][y][u]
        const int blk = i >> 6, nat = s_zz[i & 63], v = nat >> 3, u = nat & 7;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += s_dct[v * 8 + k] * s_t[blk][k * 8 + u];
        const int S = (acc + (1 << 14)) >> 15, q = s_q[(blk >= 4 ? 64 : 0) + nat];      // 8 times the coefficient: rounded once, below
        const int mag = ((S < 0 ? -S : S) + 4 * q) / (8 * q);
        out[i] = (short)(S < 0 ? -mag : mag);
    }
}

// a lane's bit string: codes enter `acc` at its low end, `held` (< 32) bits wait there; a full word is stored most significant bit first
struct Bits {
    unsigned long long acc;
    int held, words;
    unsigned *row;
    __device__ __forceinline__ void put(unsigned code, int len) {      // len <= 27
        acc = acc << len | code;
        held += len;
        if (held >= 32) {
            held -= 32;
            if (words < ROW_WORDS) row[words] = (unsigned)(acc >> held);
            ++words;
        }
    }
    __device__ __forceinline__ void finish() {
        if (words < ROW_WORDS) row[words] = held ? (unsigned)(acc << (32 - held)) : 0u;    // the rest, left-aligned, zeros below
    }
};

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }          // 0 for 0
__device__ __forceinline__ unsigned magnitude(int v, int size) { return (unsigned)(v < 0 ? v + (1 << size) - 1 : v) & ((1u << size) - 1u); }

__global__ __launch_bounds__(64) void k_jpeg_entropy(const short *__restrict__ coef, const int *__restrict__ tables, Shape s,
                                                     unsigned char *__restrict__ slots, int *__restrict__ lengths) {
    __shared__ unsigned s_rows[64 * ROW_WORDS];
    __shared__ unsigned s_image[IMAGE_WORDS];
    __shared__ unsigned s_dc[32], s_ac[512];
    const int lane = threadIdx.x, k = blockIdx.x, frame = blockIdx.y;
    for (int i = lane; i < 512; i += 64) s_ac[i] = (unsigned)tables[T_AC + i];
    if (lane < 32) s_dc[lane] = (unsigned)tables[T_DC + lane];
    const int first = k * s.restart, mcus = min(s.restart, s.mcus - first), nblocks = mcus * 6;
    __syncthreads();

    int nbits = 0;
    if (lane < nblocks) {
        const int m = lane / 6, blk = lane - m * 6, chroma = blk >= 4;
        const short *base = coef + ((size_t)frame * s.mcus + first + m) * 384;
        const short *z = base + blk * 64;
        // the DC before this block's, of the same component: the block before it in the MCU, or the MCU before; 0 at the interval's start
        int pred = 0;
        if (blk >= 1 && blk <= 3) pred = base[(blk - 1) * 64];
        else if (m > 0) pred = base[-384 + (blk == 0 ? 3 : blk) * 64];
        alignas(16) short v[64];
        const int4 *z4 = reinterpret_cast<const int4 *>(z);                // 128 bytes, 128-byte aligned
#pragma unroll
        for (int i = 0; i < 8; ++i) reinterpret_cast<int4 *>(v)[i] = z4[i];
        Bits bits{0ull, 0, 0, s_rows + lane * ROW_WORDS};
        const int diff = v[0] - pred, dsize = min(category(diff), 11);
        const unsigned dcode = s_dc[chroma * 16 + dsize];
        bits.put((dcode & 0xFFFFu) << dsize | magnitude(diff, dsize), (int)(dcode >> 16) + dsize);
        const unsigned *ac = s_ac + chroma * 256;
        int run = 0;
#pragma unroll
        for (int i = 1; i < 64; ++i) {
            const int c = v[i];
            if (c == 0) { ++run; continue; }
            while (run > 15) { bits.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16)); run -= 16; }
            const int size = min(category(c), 10);
            const unsigned code = ac[run << 4 | size];
            bits.put((code & 0xFFFFu) << size | magnitude(c, size), (int)(code >> 16) + size);
            run = 0;
        }
        if (run > 0) bits.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
        bits.finish();
        nbits = min(bits.words * 32 + bits.held, BLOCK_BITS);            // (a table that broke the bound cuts the block, nothing strays)
    }
    // inclusive scan of the bit counts over the wave
    int incl = nbits;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int total = __shfl(incl, 63, 64), offset = incl - nbits;
    const int nbytes = (total + 7) >> 3, nwords = (total + 31) >> 5;
    for (int i = lane; i <= nwords && i < IMAGE_WORDS; i += 64) s_image[i] = 0u;
    __syncthreads();
    if (lane < nblocks) {
        const unsigned *row = s_rows + lane * ROW_WORDS;
        const int sh = offset & 31, w0 = offset >> 5, nw = (nbits + 31) >> 5;
        for (int i = 0; i < nw; ++i) {
            const unsigned word = row[i];
            if (w0 + i + 1 < IMAGE_WORDS) {
                atomicOr(&s_image[w0 + i], word >> sh);
                if (sh) atomicOr(&s_image[w0 + i + 1], word << (32 - sh));
            }
        }
    }
    if (lane == 0 && (total & 7)) {                                       // 1-bits up to the byte's end
        const int pad = 8 - (total & 7);
        atomicOr(&s_image[total >> 5], ((1u << pad) - 1u) << (32 - (total & 31) - pad));
    }
    __syncthreads();
    unsigned char *slot = slots + ((size_t)frame * s.intervals + k) * s.slot;
    const long long cap = interval_capacity(mcus);
    int stuffed = 0;
    for (int b0 = 0; b0 < nbytes; b0 += 64) {
        const int b = b0 + lane;
        const unsigned byte = b < nbytes ? (s_image[b >> 2] >> (24 - 8 * (b & 3))) & 255u : 0u;
        const unsigned long long ff = __ballot(byte == 255u);
        const int pos = b + stuffed + __popcll(ff & ((1ull << lane) - 1ull));
        if (b < nbytes && pos + 1 < cap) {
            slot[pos] = (unsigned char)byte;
            if (byte == 255u) slot[pos + 1] = 0;
        }
        stuffed += __popcll(ff);
    }
    if (lane == 0) lengths[(size_t)frame * s.intervals + k] = (int)min((long long)(nbytes + stuffed), cap);
}

__global__ __launch_bounds__(256) void k_jpeg_compact(const unsigned char *__restrict__ slots, const int *__restrict__ lengths, Shape s,
                                                      unsigned char *__restrict__ scans, long long scan_stride, long long capacity,
                                                      int *__restrict__ lengths_out) {
    __shared__ long long s_part[256];
    const int tid = threadIdx.x, k = blockIdx.x, frame = blockIdx.y;
    const int *len = lengths + (size_t)frame * s.intervals;
    long long before = 0;
    for (int i = tid; i < k; i += 256) before += len[i] + 2;
    s_part[tid] = before;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    const long long off = s_part[0];
    const int n = len[k], last = k == s.intervals - 1;
    if (off + n + (last ? 0 : 2) > capacity) return;                      // cannot happen with lengths within their slots
    const unsigned char *src = slots + ((size_t)frame * s.intervals + k) * s.slot;
    unsigned char *dst = scans + (size_t)frame * scan_stride + off;
    for (int i = tid; i < n; i += 256) dst[i] = src[i];
    if (tid == 0) {
        if (last) lengths_out[frame] = (int)(off + n);
        else { dst[n] = 0xFF; dst[n + 1] = (unsigned char)(0xD0 + (k & 7)); }
    }
}

bool shape_of(int n, int h, int w, int row_stride, int restart, Shape *s) {
    if (n < 1 || n > 4096 || h < 1 || w < 1 || h > LIMIT || w > LIMIT || restart < 1 || restart > MAX_RESTART) return false;
    s->n = n; s->h = h; s->w = w; s->row_stride = row_stride; s->restart = restart;
    s->mx = (w + 15) / 16;
    s->mcus = s->mx * ((h + 15) / 16);
    s->intervals = (s->mcus + restart - 1) / restart;
    s->slot = (long long)align_up((size_t)interval_capacity(restart), 16);
    return true;
}

struct Layout { size_t coef, lengths, slots, total; };
Layout layout_of(const Shape &s) {
    Layout l;
    l.coef = 0;
    l.lengths = align_up((size_t)s.n * s.mcus * 384 * sizeof(short), 256);
    l.slots = align_up(l.lengths + (size_t)s.n * s.intervals * sizeof(int), 256);
    l.total = l.slots + (size_t)s.n * s.intervals * (size_t)s.slot;
    return l;
}
}  // namespace

extern "C" long long lav_jpeg_scan_capacity(int h, int w, int restart_mcus) {
    Shape s;
    if (!shape_of(1, h, w, 0, restart_mcus, &s)) return 0;          // (the row stride plays no part in the sizes)
    const int last = s.mcus - (s.intervals - 1) * restart_mcus;
    return (long long)(s.intervals - 1) * (interval_capacity(restart_mcus) + 2) + interval_capacity(last);
}

extern "C" size_t lav_jpeg_workspace_bytes(int n, int h, int w, int restart_mcus) {
    Shape s;
    if (!shape_of(n, h, w, 0, restart_mcus, &s)) return 0;
    return layout_of(s).total;
}

extern "C" int lav_jpeg_encode(const unsigned char *frames, int n, int h, int w, int row_stride, const int *quality_tables, int restart_mcus,
                               unsigned char *scans_out, long long scan_stride, int *lengths_out, void *workspace, size_t workspace_bytes,
                               void *stream) {
    LAV_REQUIRE(frames && quality_tables && scans_out && lengths_out && workspace, "lav_jpeg_encode: null argument");
    Shape s;
    LAV_REQUIRE(shape_of(n, h, w, row_stride, restart_mcus, &s), "lav_jpeg_encode: %d frames of %d x %d, restart interval %d (1 .. 4096 frames, sides 1 .. %d, interval 1 .. %d)",
                n, h, w, restart_mcus, LIMIT, MAX_RESTART);
    LAV_REQUIRE(row_stride >= 3 * w, "lav_jpeg_encode: row stride %d below %d bytes", row_stride, 3 * w);
    const long long capacity = lav_jpeg_scan_capacity(h, w, restart_mcus);
    LAV_REQUIRE(capacity <= 0x7FFFFFFFll, "lav_jpeg_encode: a scan of up to %lld bytes has no int32 length", capacity);
    LAV_REQUIRE(scan_stride >= capacity, "lav_jpeg_encode: scan stride %lld below the capacity %lld", scan_stride, capacity);
    LAV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(quality_tables) & 3) == 0 && (reinterpret_cast<uintptr_t>(lengths_out) & 3) == 0,
                "lav_jpeg_encode: workspace must be 256-byte, tables and lengths 4-byte aligned");
    const Layout l = layout_of(s);
    if (workspace_bytes < l.total) return fail(LAV_EWORKSPACE, "lav_jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    char *ws = static_cast<char *>(workspace);
    short *coef = reinterpret_cast<short *>(ws + l.coef);
    int *lengths = reinterpret_cast<int *>(ws + l.lengths);
    unsigned char *slots = reinterpret_cast<unsigned char *>(ws + l.slots);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("jpeg_encode", st);
    hipLaunchKernelGGL(k_jpeg_coef, dim3(s.mcus, n), dim3(256), 0, st, frames, quality_tables, s, coef);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3(s.intervals, n), dim3(64), 0, st, coef, quality_tables, s, slots, lengths);
    hipLaunchKernelGGL(k_jpeg_compact, dim3(s.intervals, n), dim3(256), 0, st, slots, lengths, s, scans_out, scan_stride, capacity, lengths_out);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
