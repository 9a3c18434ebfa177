// Coverage rules of the drawing records that debug_view.hip and log_view.hip share (lav_amd.agent.debug_view.covers, in 64-bit integers).
// A record starts with kind (0 dot, 1 segment), x0, y0, x1, y1, radius; what follows is the including kernel's own.
#pragma once
#include "common.hpp"

namespace lav {
// whether the record covers panel pixel (x, y): lav_amd.agent.debug_view.covers, in 64-bit integers
__device__ __forceinline__ bool covers(const int *r, int x, int y) {
    const long long vx = (long long)x - r[1], vy = (long long)y - r[2];
    if (r[0] == 0) return vx * vx + vy * vy <= (long long)r[5] * r[5];
    const long long dx = (long long)r[3] - r[1], dy = (long long)r[4] - r[2];
    const long long dd = dx * dx + dy * dy, t = vx * dx + vy * dy;
    if (t <= 0) return vx * vx + vy * vy <= 1;
    if (t >= dd) {
        const long long ux = (long long)x - r[3], uy = (long long)y - r[4];
        return ux * ux + uy * uy <= 1;
    }
    const long long c = vx * dy - vy * dx, a = c < 0 ? -c : c;
    return a < (1ll << 22) && a * a <= dd;
}
__device__ __forceinline__ bool touches(const int *r, int bx0, int by0, int bx1, int by1) {      // the record's box against [bx0, bx1] x [by0, by1]
    const int rad = r[5];
    return min(r[1], r[3]) - rad <= bx1 && max(r[1], r[3]) + rad >= bx0 && min(r[2], r[4]) - rad <= by1 && max(r[2], r[4]) + rad >= by0;
}
}  // namespace lav
