// The direct warp of MULTIBAND fusion (libstabstitch_mbwarp.so, include/stabstitch_mbwarp.h).
//
// MULTIBAND used to warp a stacked copy of its input: ops.multiband_stack writes U [n * V][4][h][w] (B, G, R and the weight plane
// min(x + 1, w - x) * min(y + 1, h - y)) and ss_tps_warp_mask_nchw (render.hip) reads it back.  Here one launch goes from the caller's
// frames -- fp32 planes or decoded uint8 -- to P [n][V][5][hc][wc]: the colour taps are gathered from the frames themselves, the weight
// plane's taps are computed from the tap indices (small integers, one rounding of their product: the value U holds), and the
// exposure gains of ss_exposure_update, when given, scale the sampled colours as the fused renders do (fminf(g * s, 255)).
//
// Same geometry as tps_warp_kernel: 256 threads, a tile of 64 columns x 8 rows, wave w owns rows w and w + 4, the spline through
// tps_rows_table / tps_eval_rows (device_math.h) -- the sampling coordinates, and without gains every plane, equal the two-step path
// bit for bit (-ffp-contract=off: the FAST taps below are written with plain operators, as render.hip's are).
#include "common.h"
#include "device_math.h"

#include "../../include/stabstitch_mbwarp.h"

namespace {

// ---- restated from render.hip (which is not edited; it shares no header with this library): taps_fast, the term order of
// sample_fast / fast_mask, warp_rows_coords
struct MwFastTaps {
    int x0, y0, x1, y1;
    float w00, w01, w10, w11;
    bool vx0, vx1, vy0, vy1;
};
__device__ __forceinline__ MwFastTaps mw_taps_fast(float xn, float yn, int W, int H) {
    MwFastTaps t;
    float x = ((xn + 1.f) / 2.f) * (float)(W - 1);
    float y = ((yn + 1.f) / 2.f) * (float)(H - 1);
    float xf = fminf(fmaxf(floorf(x), -4.f), (float)W + 4.f);
    float yf = fminf(fmaxf(floorf(y), -4.f), (float)H + 4.f);
    t.x0 = (int)xf; t.y0 = (int)yf; t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
    t.w00 = (xf + 1.f - x) * (yf + 1.f - y); t.w01 = (x - xf) * (yf + 1.f - y);
    t.w10 = (xf + 1.f - x) * (y - yf); t.w11 = (x - xf) * (y - yf);
    t.vx0 = (unsigned)t.x0 < (unsigned)W; t.vx1 = (unsigned)t.x1 < (unsigned)W;
    t.vy0 = (unsigned)t.y0 < (unsigned)H; t.vy1 = (unsigned)t.y1 < (unsigned)H;
    return t;
}
// sample_fast's sum, term by term: the taps inside the image in the order (x0,y0), (x1,y0), (x0,y1), (x1,y1); tap(x, y) is only
// called for a tap inside.  With tap = 1 it is fast_mask (1 * w is w).
template <typename F>
__device__ __forceinline__ float mw_fast_sum(const MwFastTaps& t, F&& tap) {
    float r = 0.f;
    if (t.vx0 && t.vy0) r = __fadd_rn(r, __fmul_rn(tap(t.x0, t.y0), t.w00));
    if (t.vx1 && t.vy0) r = __fadd_rn(r, __fmul_rn(tap(t.x1, t.y0), t.w01));
    if (t.vx0 && t.vy1) r = __fadd_rn(r, __fmul_rn(tap(t.x0, t.y1), t.w10));
    if (t.vx1 && t.vy1) r = __fadd_rn(r, __fmul_rn(tap(t.x1, t.y1), t.w11));
    return r;
}
// blend4 over the four clamped taps in tps_warp_kernel's order: (x0,y0), (x0,y1), (x1,y0), (x1,y1)
template <typename F>
__device__ __forceinline__ float mw_normal_sum(const SsTaps& t, F&& tap) {
    return blend4(t, tap(t.x0, t.y0), tap(t.x0, t.y1), tap(t.x1, t.y0), tap(t.x1, t.y1));
}
__device__ __forceinline__ void mw_rows_coords(const float* __restrict__ src, const float* __restrict__ T, ss_f2* tab, int lane, int x,
                                               int ya, int yb, int hc, int wc, ss_f2& xn, ss_f2& yn) {
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
    tps_rows_table(src, gya, gyb, lane, tab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the same wave reads it back: ordering only
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    tps_eval_rows(src, T, tab, gx, gya, gyb, xn, yn);
}

struct MwViews {
    const void* img[3];
};

// one colour value of the pixel (x, y) of a frame: fp32 planes [3][h][w], or a decoded frame [h][w][3] (three byte loads per tap from
// one address, as sample3_u8: a pixel's 3 bytes have no alignment a wider load could use without reading past the last pixel)
template <bool U8>
__device__ __forceinline__ float mw_tap(const void* __restrict__ img, int x, int y, int ch, int w, long long hw) {
    const long long pix = (long long)y * w + x;
    if (U8) return (float)static_cast<const unsigned char*>(img)[pix * 3 + ch];
    return static_cast<const float*>(img)[ch * hw + pix];
}
// the weight plane at (x, y): ops.multiband_weight_plane's value, its one rounding included (the product exceeds 2^24 on large frames)
__device__ __forceinline__ float mw_weight(int x, int y, int w, int h) {
    return __fmul_rn((float)min(x + 1, w - x), (float)min(y + 1, h - y));
}

// item b = frame * views + view rides in gridDim.z; out [items][5][hc][wc]
template <bool U8, bool GAINS>
__global__ __launch_bounds__(256) void mw_warp_kernel(MwViews rv, const float* __restrict__ source, const float* __restrict__ T,
                                                      const float* __restrict__ gains, float* __restrict__ out, int views, int h,
                                                      int w, int hc, int wc, int mode) {
    __shared__ ss_f2 dytab[4][64];
    const int b = blockIdx.z;
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lx;
    const int ya = blockIdx.y * 8 + wv, yb = ya + 4;
    if (ya >= hc) return;                       // whole waves only: lanes past the canvas edge still help build the table
    ss_f2 xn2, yn2;
    mw_rows_coords(source + (long long)b * SS_NV * 2, T + (long long)b * 2 * SS_NT, dytab[wv], lx, x, ya, yb, hc, wc, xn2, yn2);
    if (x >= wc) return;
    const int f = b / views, k = b - f * views;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    const void* base = k == 0 ? rv.img[0] : (k == 1 ? rv.img[1] : rv.img[2]);
    const void* img = static_cast<const char*>(base) + f * 3 * hw * (long long)(U8 ? 1 : sizeof(float));
    float g[3] = {1.f, 1.f, 1.f};
    if (GAINS) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) g[ch] = gains[(long long)b * 3 + ch];
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int y = rr ? yb : ya;
        if (y >= hc) break;
        const float xn = rr ? xn2.y : xn2.x, yn = rr ? yn2.y : yn2.x;
        float v[5];
        if (mode == SSW_WARP_NORMAL) {
            const SsTaps t = taps_normal(xn, yn, w, h);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                v[ch] = mw_normal_sum(t, [&](int tx, int ty) { return mw_tap<U8>(img, tx, ty, ch, w, hw); });
            v[3] = mw_normal_sum(t, [&](int tx, int ty) { return mw_weight(tx, ty, w, h); });
            v[4] = blend4(t, 1.f, 1.f, 1.f, 1.f);
        } else {
            const MwFastTaps t = mw_taps_fast(xn, yn, w, h);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                v[ch] = mw_fast_sum(t, [&](int tx, int ty) { return mw_tap<U8>(img, tx, ty, ch, w, hw); });
            v[3] = mw_fast_sum(t, [&](int tx, int ty) { return mw_weight(tx, ty, w, h); });
            v[4] = mw_fast_sum(t, [](int, int) { return 1.f; });
        }
        if (GAINS) {                            // the colours only: the weight plane and the mask are geometry
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = fminf(__fmul_rn(g[ch], v[ch]), 255.f);
        }
        float* o = out + (long long)b * 5 * ohw + (long long)y * wc + x;
#pragma unroll
        for (int p = 0; p < 5; ++p) o[p * ohw] = v[p];
    }
}

int mw_status() { return hipGetLastError() == hipSuccess ? SSW_OK : SSW_ERR_LAUNCH; }

template <bool U8>
int mw_launch(const void* const* imgs, const float* source, const float* T, const float* gains, float* out, int frames, int views,
              int h, int w, int hc, int wc, int mode, void* stream) {
    if (!imgs || !source || !T || !out || views < 2 || views > SSW_MAX_VIEWS || h <= 1 || w <= 1 || hc <= 1 || wc <= 1 ||
        (mode != SSW_WARP_NORMAL && mode != SSW_WARP_FAST) || frames <= 0 || (long long)frames * views > SSW_MAX_ITEMS ||
        ss_cdiv(hc, 8) > 65535)
        return SSW_ERR_ARG;
    MwViews rv;
    for (int i = 0; i < 3; ++i) rv.img[i] = i < views ? imgs[i] : nullptr;
    for (int i = 0; i < views; ++i)
        if (!rv.img[i]) return SSW_ERR_ARG;
    const dim3 grid(ss_cdiv(wc, 64), ss_cdiv(hc, 8), frames * views);
    if (gains)
        hipLaunchKernelGGL((mw_warp_kernel<U8, true>), grid, dim3(256), 0, (hipStream_t)stream, rv, source, T, gains, out, views, h, w,
                           hc, wc, mode);
    else
        hipLaunchKernelGGL((mw_warp_kernel<U8, false>), grid, dim3(256), 0, (hipStream_t)stream, rv, source, T, gains, out, views, h, w,
                           hc, wc, mode);
    return mw_status();
}

}  // namespace

extern "C" {

SSW_API int ssw_version(void) { return 1; }

SSW_API int ssw_multiband_warp(const float* const* imgs, const float* source, const float* T, const float* gains, float* out, int frames,
                               int views, int h, int w, int hc, int wc, int mode, void* stream) {
    return mw_launch<false>(reinterpret_cast<const void* const*>(imgs), source, T, gains, out, frames, views, h, w, hc, wc, mode, stream);
}

SSW_API int ssw_multiband_warp_u8(const unsigned char* const* imgs, const float* source, const float* T, const float* gains, float* out,
                                  int frames, int views, int h, int w, int hc, int wc, int mode, void* stream) {
    return mw_launch<true>(reinterpret_cast<const void* const*>(imgs), source, T, gains, out, frames, views, h, w, hc, wc, mode, stream);
}

}  // extern "C"
