// NV12 <-> packed BGR bytes, shared by frameio.hip and render.hip ("Frame formats").
// BT.601 limited range in 20-bit fixed point, plain 32-bit integer arithmetic (every intermediate stays below 2^30 in
// magnitude); `>>` is the arithmetic shift.  tests/nv12_ref.py states the same two conversions in numpy, and every NV12
// route of the library equals "convert with the first, run the packed-BGR route, convert with the second" byte for byte.
#pragma once
#include "common.h"

// frames of up to three views: Y plane and interleaved UV plane of frame 0, one pitch per view (bytes per row of BOTH
// planes, even, >= w), `fs` bytes between consecutive frames of a view (both planes)
struct Nv12Views {
    const unsigned char* y[3];
    const unsigned char* uv[3];
    long long fs[3];
    int pitch[3];
};

__device__ __forceinline__ int nv12_sat8(int v) { return min(max(v, 0), 255); }

// (Y, U, V) -> c = (B, G, R)
__device__ __forceinline__ void nv12_to_bgr(int Y, int U, int V, int (&c)[3]) {
    const int l = max(Y - 16, 0) * 1220542 + (1 << 19), u = U - 128, v = V - 128;
    c[0] = nv12_sat8((l + 2116026 * u) >> 20);
    c[1] = nv12_sat8((l - 409993 * u - 852492 * v) >> 20);
    c[2] = nv12_sat8((l + 1673527 * v) >> 20);
}

// pixel (y, x) of a frame: its Y byte and the chroma pair of its 2 x 2 block (no chroma interpolation), the pair as ONE
// 16-bit load (uv is 2-byte aligned and the pitch even: the entry points refuse anything else)
__device__ __forceinline__ void nv12_pixel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp, int pitch,
                                           int y, int x, int (&c)[3]) {
    const int Y = yp[(long long)y * pitch + x];
    const unsigned uv = *reinterpret_cast<const unsigned short*>(uvp + (long long)(y >> 1) * pitch + (x & ~1));
    nv12_to_bgr(Y, (int)(uv & 255u), (int)(uv >> 8), c);
}

__device__ __forceinline__ unsigned char bgr_to_y(int b, int g, int r) {
    return (unsigned char)((269484 * r + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20);
}
// sums of the four B, G, R bytes of a 2 x 2 block -> U | V << 8 of their rounded means
__device__ __forceinline__ unsigned short bgr4_to_uv(int sb, int sg, int sr) {
    const int b = (sb + 2) >> 2, g = (sg + 2) >> 2, r = (sr + 2) >> 2;
    const int u = (-155188 * r - 305135 * g + 460324 * b + (128 << 20) + (1 << 19)) >> 20;
    const int v = (460324 * r - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20;
    return (unsigned short)((u & 255) | ((v & 255) << 8));
}
