// Offline point painting (lav/data_paint.py, lav/utils/point_painting.py of the reference): a batch of recorded frames'
// LiDAR sweeps painted with their cameras' class probabilities in one launch, and the uint8 -> float32 image conversion
// that feeds the segmenter.
//
// lav_paint (paint.hip) is the agent's painter: one cloud, at most 4 cameras, float32 projection (InferModel's arithmetic),
// fused (n, lidar_dim + 4) rows.  The data collector's painter projects in FLOAT64 (CoordConverter.lidar_to_cam works on
// numpy doubles) over all 5 cameras and stores only the (n, 4) scores; lav_amd.data.datasets.CameraProjection.pixels /
// paint_from_cameras restate it on the CPU, and this kernel follows them:
//   xyz -> double;  world = l2w . [x y z 1];  cam = w2c . world;  (X, Y, Z) = (cam_y, -cam_z, cam_x);  p = K . (X, Y, Z)
//   every product and every sum rounded separately (no FMA contraction), terms in k order;
//   u = trunc(p0 / (1e-5 + p2)), v = trunc(p1 / (1e-5 + p2)), d = trunc(p2)   (numpy's astype(int): int64, INT64_MIN for a
//   non-finite or out-of-range value - never valid);  valid: d >= 0, 0 <= u < w, 0 <= v < h;
//   painted[c] = s[c + 1] * (1 - s[0]) in float32 (data_paint.py:75); a later camera overwrites an earlier one; zeros else.
// One thread per point.  The frame of a point is found by a binary search over the frames + 1 offsets staged in LDS; the
// points of a frame are consecutive, so consecutive workgroups gather from the same frame's maps.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {
using namespace lav;
constexpr int MAX_CAM_F64 = 8;
constexpr int MAX_FRAMES = 1024;      // offsets staged in LDS: (MAX_FRAMES + 1) ints

struct PaintFramesArgs {
    lav_camera_f64 cam[MAX_CAM_F64];
    int ncam, frames, total, lidar_dim, h, w;
};

__device__ __forceinline__ double dmv4(const double *m, double x, double y, double z, double w) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), __dmul_rn(m[3], w));
}
__device__ __forceinline__ double dmv3(const double *m, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z));
}
// ndarray.astype(int) of a double: truncation toward zero; false (and INT64_MIN) where the value is not finite or does not fit
__device__ __forceinline__ bool to_int64(double v, long long &out) {
    if (!(fabs(v) < 9223372036854775808.0)) {
        out = LLONG_MIN;
        return false;
    }
    out = (long long)v;
    return true;
}
// the int32 record of such a value: saturated; INT32_MIN also stands for "invalid"
__device__ __forceinline__ int sat32(long long v) {
    return v < (long long)INT32_MIN ? INT32_MIN : v > (long long)INT32_MAX ? INT32_MAX : (int)v;
}

template <int SEM_C>
__global__ __launch_bounds__(256) void k_paint_frames(PaintFramesArgs a, const float *__restrict__ lidar, const int *__restrict__ offsets,
                                                      const float *__restrict__ sem, float *__restrict__ painted_out, int *__restrict__ uvz) {
    __shared__ int s_off[MAX_FRAMES + 1];
    for (int k = threadIdx.x; k <= a.frames; k += blockDim.x) s_off[k] = offsets[k];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    // frame f: the last one with offsets[f] <= i, within [0, frames - 1] whatever the offsets hold (empty frames are skipped)
    int lo = 0, hi = a.frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int frame = lo;
    const float *p = lidar + (long)i * a.lidar_dim;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    float painted[SEM_C];
#pragma unroll
    for (int c = 0; c < SEM_C; ++c) painted[c] = 0.f;
    const long plane = (long)a.h * a.w;
    const float *fsem = sem + (long)frame * a.ncam * (SEM_C + 1) * plane;
    for (int cam = 0; cam < a.ncam; ++cam) {
        const lav_camera_f64 &cm = a.cam[cam];
        const double wx = dmv4(cm.l2w + 0, x, y, z, 1.0), wy = dmv4(cm.l2w + 4, x, y, z, 1.0);
        const double wz = dmv4(cm.l2w + 8, x, y, z, 1.0), ww = dmv4(cm.l2w + 12, x, y, z, 1.0);
        const double cx = dmv4(cm.w2c + 0, wx, wy, wz, ww), cy = dmv4(cm.w2c + 4, wx, wy, wz, ww);
        const double cz = dmv4(cm.w2c + 8, wx, wy, wz, ww);
        const double X = cy, Y = -cz, Z = cx;  // point_painting.py:35
        const double p0 = dmv3(cm.K + 0, X, Y, Z), p1 = dmv3(cm.K + 3, X, Y, Z), p2 = dmv3(cm.K + 6, X, Y, Z);
        const double den = __dadd_rn(1e-5, p2);
        long long u, v, d;
        const bool ok_u = to_int64(__ddiv_rn(p0, den), u), ok_v = to_int64(__ddiv_rn(p1, den), v), ok_d = to_int64(p2, d);
        if (uvz) {
            int *o = uvz + ((long)cam * a.total + i) * 3;
            o[0] = sat32(u); o[1] = sat32(v); o[2] = sat32(d);
        }
        if (ok_u && ok_v && ok_d && d >= 0 && u >= 0 && u < a.w && v >= 0 && v < a.h) {
            const float *s = fsem + (long)cam * (SEM_C + 1) * plane + (long)v * a.w + u;
            const float keep = __fsub_rn(1.f, s[0]);
#pragma unroll
            for (int c = 0; c < SEM_C; ++c) painted[c] = __fmul_rn(s[(c + 1) * plane], keep);
        }
    }
    if constexpr (SEM_C == 4) {
        *reinterpret_cast<float4 *>(painted_out + (long)i * 4) = make_float4(painted[0], painted[1], painted[2], painted[3]);
    } else {
#pragma unroll
        for (int c = 0; c < SEM_C; ++c) painted_out[(long)i * SEM_C + c] = painted[c];
    }
}

// (n, h, w, C_SRC) uint8 -> (n, 3, h, w) float32, channels 0..2 (reversed: 2..0).  VEC: four pixels per thread (plane % 4 == 0).
template <int C_SRC, bool VEC>
__global__ __launch_bounds__(256) void k_u8_to_f32(const unsigned char *__restrict__ img, long plane, long groups, int reverse,
                                                   float *__restrict__ out) {
    constexpr int PX = VEC ? 4 : 1;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;   // group of PX pixels; groups = n * plane / PX
    if (g >= groups) return;
    const long pix = g * PX;                                       // never straddles two images: plane % PX == 0
    const long n = pix / plane, off = pix - n * plane;
    unsigned char b[PX * C_SRC];
    if constexpr (VEC) {
        const unsigned int *src = reinterpret_cast<const unsigned int *>(img + pix * C_SRC);   // 4 * C_SRC bytes, 4-byte aligned
#pragma unroll
        for (int k = 0; k < C_SRC; ++k) {
            const unsigned int wd = src[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[4 * k + j] = (unsigned char)(wd >> (8 * j));
        }
    } else {
#pragma unroll
        for (int k = 0; k < C_SRC; ++k) b[k] = img[pix * C_SRC + k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sc = reverse ? 2 - c : c;
        float *o = out + (n * 3 + c) * plane + off;
        if constexpr (VEC) {
            *reinterpret_cast<float4 *>(o) = make_float4((float)b[sc], (float)b[C_SRC + sc], (float)b[2 * C_SRC + sc], (float)b[3 * C_SRC + sc]);
        } else {
            o[0] = (float)b[sc];
        }
    }
}
}  // namespace

extern "C" int lav_paint_frames(const float *lidar, const int *offsets, int frames, int total, int lidar_dim, const float *sem, int ncam,
                                int sem_c, int h, int w, const lav_camera_f64 *h_cams, float *painted, int *uvz, void *stream) {
    LAV_REQUIRE(frames >= 1 && frames <= MAX_FRAMES, "lav_paint_frames: frames %d outside [1,%d]", frames, MAX_FRAMES);
    LAV_REQUIRE(total >= 0 && lidar_dim >= 3 && h >= 1 && w >= 1 && offsets && sem && h_cams && ((lidar && painted) || total == 0),
                "lav_paint_frames: bad argument");
    LAV_REQUIRE(ncam >= 1 && ncam <= MAX_CAM_F64, "lav_paint_frames: ncam %d outside [1,%d]", ncam, MAX_CAM_F64);
    LAV_REQUIRE(sem_c == 4, "lav_paint_frames: sem_c %d not instantiated (4)", sem_c);
    LAV_REQUIRE(reinterpret_cast<uintptr_t>(painted) % 16 == 0, "lav_paint_frames: painted must be 16-byte aligned");
    LAV_REQUIRE((long)total + 255 < (long)INT32_MAX, "lav_paint_frames: %d points", total);
    if (total == 0) return LAV_OK;
    PaintFramesArgs a;
    for (int c = 0; c < MAX_CAM_F64; ++c) a.cam[c] = h_cams[c < ncam ? c : 0];
    a.ncam = ncam; a.frames = frames; a.total = total; a.lidar_dim = lidar_dim; a.h = h; a.w = w;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tok = timer_begin("paint_frames", st);
    hipLaunchKernelGGL((k_paint_frames<4>), dim3((total + 255) / 256), dim3(256), 0, st, a, lidar, offsets, sem, painted, uvz);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}

extern "C" int lav_image_u8_to_f32(const unsigned char *img, int n, int h, int w, int c_src, int reverse, float *out, void *stream) {
    LAV_REQUIRE(n >= 0 && h >= 1 && w >= 1 && ((img && out) || n == 0), "lav_image_u8_to_f32: bad argument");
    LAV_REQUIRE(c_src == 3 || c_src == 4, "lav_image_u8_to_f32: %d source channels (3 or 4)", c_src);
    if (n == 0) return LAV_OK;
    const long plane = (long)h * w;
    const bool vec = plane % 4 == 0 && reinterpret_cast<uintptr_t>(img) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const long groups = (long)n * plane / (vec ? 4 : 1);
    LAV_REQUIRE((groups + 255) / 256 < (long)INT32_MAX, "lav_image_u8_to_f32: %ld pixel groups", groups);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    const int tok = timer_begin("image_u8_to_f32", st);
    if (c_src == 3 && vec) hipLaunchKernelGGL((k_u8_to_f32<3, true>), grid, block, 0, st, img, plane, groups, reverse, out);
    else if (c_src == 3) hipLaunchKernelGGL((k_u8_to_f32<3, false>), grid, block, 0, st, img, plane, groups, reverse, out);
    else if (vec) hipLaunchKernelGGL((k_u8_to_f32<4, true>), grid, block, 0, st, img, plane, groups, reverse, out);
    else hipLaunchKernelGGL((k_u8_to_f32<4, false>), grid, block, 0, st, img, plane, groups, reverse, out);
    timer_end(tok, st);
    LAV_LAUNCH_CHECK();
    return LAV_OK;
}
