// Decoded NV12 surfaces -> packed BGR frames, a list of surfaces per launch (libstabstitch_surfaces.so,
// include/stabstitch_surfaces.h).
//
// The streaming stitchers' batched uint8 routes (push_many_u8, MultiOnlineStitcher.push_u8, HostFrameStream) take packed BGR; a
// decoder delivers NV12 surfaces out of a pool, each with its own planes and pitch.  This is the converter in front of those routes:
// all surfaces of a call -- k frames of every view -- in ONE launch, the surfaces in gridDim.z, their pointers and pitches in the
// kernel arguments (96 x 20 bytes).  The colour statement is nv12_to_bgr of nv12.h, not restated here.
//
// Memory-bound, 1.5 bytes in and 3 bytes out per pixel.  ALIGNED: a thread owns 8 pixels x 2 rows -- one 8-byte load per Y row, one
// 8-byte load of their four chroma pairs, three 8-byte stores per row; 32 lanes cover 256 contiguous bytes of a Y row and 768 of an
// output row.  Otherwise a thread owns one 2 x 2 block: byte loads of Y, the chroma pair as one 16-bit load (nv12_pixel's), byte
// stores.  No LDS, no scratch, no atomics.
#include "common.h"
#include "nv12.h"

#include "../../include/stabstitch_surfaces.h"

namespace {

struct SfSurfaces {
    const unsigned char* y[SSF_MAX_SURFACES];
    const unsigned char* uv[SSF_MAX_SURFACES];
    int pitch[SSF_MAX_SURFACES];
};

// A saturated channel value, made opaque to the compiler before it is packed next to others.  Left visible, hipcc fuses "shift by 20,
// saturate, place two bytes" into v_ashr_pk_u8_i32 and ORs the other two bytes of the word into its result -- but on gfx950 that
// instruction leaves the upper half of its destination register as it was, and the stale bits came out in bytes 2 and 3 of every
// word the aligned instantiation stored (LAB_NOTES.md, "NV12 at batch rates").  The barrier costs no instruction.
__device__ __forceinline__ unsigned sf_byte(int c) {
    unsigned v = (unsigned)c;
    asm volatile("" : "+v"(v));
    return v;
}

// 8 pixels of one row: their Y bytes in (lo, hi), the four chroma pairs in (uvlo, uvhi) -> 24 bytes B, G, R, B, .. as three 8-byte stores
__device__ __forceinline__ void sf_row8(uint2 yy, uint2 uv, unsigned char* __restrict__ o) {
    unsigned wds[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned yw = i < 4 ? yy.x : yy.y, cw = i < 4 ? uv.x : uv.y;
        const int Y = (int)((yw >> (8 * (i & 3))) & 255u);
        const int U = (int)((cw >> (16 * ((i >> 1) & 1))) & 255u), V = (int)((cw >> (16 * ((i >> 1) & 1) + 8)) & 255u);
        int c[3];
        nv12_to_bgr(Y, U, V, c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int b = 3 * i + ch;
            wds[b >> 2] |= sf_byte(c[ch]) << (8 * (b & 3));
        }
    }
    uint2* o8 = reinterpret_cast<uint2*>(o);
    o8[0] = make_uint2(wds[0], wds[1]);
    o8[1] = make_uint2(wds[2], wds[3]);
    o8[2] = make_uint2(wds[4], wds[5]);
}

// surface s = blockIdx.z; out [surfaces][h][w][3] with `out_stride` bytes between frames.
// ALIGNED: block 32 x 8, thread = 8 pixels x 2 rows (w % 8 == 0, so a thread is inside or outside the frame as a whole).
// else:    block 64 x 4, thread = 2 x 2 pixels.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void sf_convert_kernel(SfSurfaces sf, unsigned char* __restrict__ out, long long out_stride, int h,
                                                         int w) {
    const int s = blockIdx.z;
    const unsigned char* __restrict__ yp = sf.y[s];
    const unsigned char* __restrict__ uvp = sf.uv[s];
    const int pitch = sf.pitch[s];
    unsigned char* __restrict__ o = out + (long long)s * out_stride;
    if (ALIGNED) {
        const int x = (blockIdx.x * 32 + (threadIdx.x & 31)) * 8;
        const int r = blockIdx.y * 8 + (threadIdx.x >> 5);             // the row pair
        if (x >= w || 2 * r >= h) return;
        const long long row = (long long)(2 * r) * pitch + x;
        const uint2 y0 = *reinterpret_cast<const uint2*>(yp + row);
        const uint2 y1 = *reinterpret_cast<const uint2*>(yp + row + pitch);
        const uint2 uv = *reinterpret_cast<const uint2*>(uvp + (long long)r * pitch + x);
        unsigned char* po = o + ((long long)(2 * r) * w + x) * 3;
        sf_row8(y0, uv, po);
        sf_row8(y1, uv, po + (long long)w * 3);
    } else {
        const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2;
        const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
        if (x >= w || 2 * r >= h) return;
        const unsigned uv = *reinterpret_cast<const unsigned short*>(uvp + (long long)r * pitch + x);
        const int U = (int)(uv & 255u), V = (int)(uv >> 8);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const unsigned char* py = yp + (long long)(2 * r + dy) * pitch + x;
            unsigned char* po = o + ((long long)(2 * r + dy) * w + x) * 3;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                int c[3];
                nv12_to_bgr((int)py[dx], U, V, c);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) po[3 * dx + ch] = (unsigned char)sf_byte(c[ch]);
            }
        }
    }
}

bool sf_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" {

SSF_API int ssf_version(void) { return 1; }

SSF_API int ssf_nv12_to_bgr(const unsigned char* const* y, const unsigned char* const* uv, const int* pitch, int surfaces, int h, int w,
                            unsigned char* out, long long out_stride, void* stream) {
    if (!y || !uv || !pitch || !out || surfaces < 1 || surfaces > SSF_MAX_SURFACES || h <= 0 || w <= 0 || (h & 1) || (w & 1) ||
        (long long)h * w >= (1ll << 31) || h > 8 * 65535 || out_stride < 3ll * h * w)
        return SSF_ERR_ARG;
    SfSurfaces sf;
    bool aligned = w % 8 == 0 && out_stride % 8 == 0 && sf_aligned8(out);
    for (int s = 0; s < surfaces; ++s) {
        if (!y[s] || !uv[s] || (pitch[s] & 1) || pitch[s] < w || (reinterpret_cast<uintptr_t>(uv[s]) & 1u)) return SSF_ERR_ARG;
        sf.y[s] = y[s];
        sf.uv[s] = uv[s];
        sf.pitch[s] = pitch[s];
        aligned = aligned && pitch[s] % 8 == 0 && sf_aligned8(y[s]) && sf_aligned8(uv[s]);
    }
    for (int s = surfaces; s < SSF_MAX_SURFACES; ++s) {
        sf.y[s] = sf.uv[s] = nullptr;
        sf.pitch[s] = 0;
    }
    if (aligned)
        hipLaunchKernelGGL((sf_convert_kernel<true>), dim3(ss_cdiv(w / 8, 32), ss_cdiv(h / 2, 8), surfaces), dim3(256), 0,
                           (hipStream_t)stream, sf, out, out_stride, h, w);
    else
        hipLaunchKernelGGL((sf_convert_kernel<false>), dim3(ss_cdiv(w / 2, 64), ss_cdiv(h / 2, 4), surfaces), dim3(256), 0,
                           (hipStream_t)stream, sf, out, out_stride, h, w);
    return hipGetLastError() == hipSuccess ? SSF_OK : SSF_ERR_LAUNCH;
}

}  // extern "C"
