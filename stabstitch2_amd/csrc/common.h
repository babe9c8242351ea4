// Shared helpers for libstabstitch_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stabstitch_hip.h"

#define SS_GRID_H 6
#define SS_GRID_W 8
#define SS_NV 63   // (SS_GRID_H+1)*(SS_GRID_W+1) control points
#define SS_NT 66   // SS_NV + 3 TPS coefficients per coordinate

static inline int ss_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SS_OK : SS_ERR_LAUNCH;
}

static inline int ss_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// exact n / d for n < 65536, 1 <= d < 65536, branch free:  q = umulhi(n, mul) + (n & mask)
//   d > 1: mul = ceil(2^32 / d), mask = 0;   d == 1: mul = 0, mask = ~0 (identity)
struct SsFastDiv {
    uint32_t mul, mask;
};
static inline SsFastDiv ss_fastdiv_make(uint32_t d) {
    SsFastDiv f;
    if (d <= 1) { f.mul = 0u; f.mask = 0xFFFFFFFFu; }
    else { f.mul = (uint32_t)(((1ull << 32) + d - 1) / d); f.mask = 0u; }
    return f;
}
__device__ __forceinline__ uint32_t ss_fastdiv(uint32_t n, SsFastDiv f) { return __umulhi(n, f.mul) + (n & f.mask); }

// exact n / d for every 32-bit n (Granlund-Montgomery round-up method): t = umulhi(n, mul); q = (t + ((n - t) >> sh1)) >> sh2
struct SsDiv32 {
    uint32_t mul, sh1, sh2;
};
static inline SsDiv32 ss_div32_make(uint32_t d) {
    SsDiv32 f;
    if (d <= 1) { f.mul = 0u; f.sh1 = 0u; f.sh2 = 0u; return f; }
    const uint32_t l = 32u - (uint32_t)__builtin_clz(d - 1u);          // ceil(log2 d)
    f.mul = (uint32_t)(((((1ull << l) - d) << 32) / d) + 1ull);
    f.sh1 = 1u;
    f.sh2 = l - 1u;
    return f;
}
__device__ __forceinline__ uint32_t ss_div32(uint32_t n, SsDiv32 f) {
    const uint32_t t = __umulhi(n, f.mul);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

__device__ __forceinline__ float ss_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float ss_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float ss_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// overflow watcher of a streaming canvas (geom.hip: ss_canvas_watch has the state's layout); used by geom.hip and render.hip
__device__ __forceinline__ void canvas_watch_update(float xmin, float xmax, float ymin, float ymax, bool bad, float guard, int* wi,
                                                    float* wf) {
    xmin = ss_wave_min(xmin); xmax = ss_wave_max(xmax); ymin = ss_wave_min(ymin); ymax = ss_wave_max(ymax);
    // fminf / fmaxf drop a NaN operand: a NaN control point would vanish from the extremes, so it is carried as a flag of its own
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (threadIdx.x == 0) {
        const float lo = fminf(xmin, ymin), hi = fmaxf(xmax, ymax);
        const int seen = wi[0];
        // (half a pixel of a 4096-wide canvas: the canvas is the first window's OWN bbox when margin = 0, its extremes sit on +-1;
        // `near` gets the same slack when the guard is smaller than it, else fp32 rounding alone would ask for a growth)
        const float slack = 2.5e-4f;
        const bool out = anybad || lo < -1.0f - slack || hi > 1.0f + slack;
        const float g = guard > slack ? guard : -slack;
        const bool near = out || lo < -1.0f + g || hi > 1.0f - g;
        if (out) { wi[1] += 1; if (wi[2] < 0) wi[2] = seen; }
        if (near) wi[3] += 1;
        wi[0] = seen + 1;
        wf[0] = fminf(wf[0], xmin); wf[1] = fmaxf(wf[1], xmax); wf[2] = fminf(wf[2], ymin); wf[3] = fmaxf(wf[3], ymax);
    }
}

// Device-side refit of a streaming canvas whose OUTPUT SIZE is fixed (viewport hout x wout; online.py: grow='refit').  The render
// kernels take the pixel count and the box separately and the box is read on the device, so zooming out is a rewrite of four
// floats.  State per stream: box [4] (wmin, wmax, hmin, hmax in HR px), epoch (growths so far), ext0 [2] (the extents the canvas
// was set with).  All arithmetic in __f*_rn intrinsics, one operation after the other: ONE sequential fp32 reading, restated in
// numpy by tests/test_canvas_fit_abi.py.
struct SsCanvasFit {
    float* box;          // [streams][4]
    int* epoch;          // [streams]
    float* ext0;         // [streams][2] (width, height): written when the canvas is set, read by the fit
    float margin, zoom_limit, wout, hout;
};

// letterbox (x0, x1, y0, y1) about its centre to the aspect wout : hout -- it only ever expands; untouched when ow * hout == oh * wout
struct SsBox {
    float x0, x1, y0, y1;
};
__device__ __forceinline__ SsBox canvas_fit_aspect(SsBox b, float wout, float hout) {
    const float ow = __fsub_rn(b.x1, b.x0), oh = __fsub_rn(b.y1, b.y0);
    const float pw = __fmul_rn(ow, hout), ph = __fmul_rn(oh, wout);
    if (pw > ph) {
        const float d = __fmul_rn(__fsub_rn(__fdiv_rn(pw, wout), oh), 0.5f);
        b.y0 = __fsub_rn(b.y0, d); b.y1 = __fadd_rn(b.y1, d);
    } else if (ph > pw) {
        const float d = __fmul_rn(__fsub_rn(__fdiv_rn(ph, hout), ow), 0.5f);
        b.x0 = __fsub_rn(b.x0, d); b.x1 = __fadd_rn(b.x1, d);
    }
    return b;
}

// Lane 0, right after canvas_watch_update on the same rows: when the running extents wf came within the guard of an edge, re-fix
// the box around itself and everything seen on it (_CanvasWatch._needed_bbox's formula), grown by the margin and fitted to the
// viewport's aspect.  Refused -- box, epoch and wf untouched, such frames stay cropped and counted as under grow='never' -- when a
// new coordinate is not finite, when an extent would exceed zoom_limit x the initial one (a diverging mesh must not shrink the
// picture to nothing), or when no side moves by half a pixel (_CanvasWatch._regrow's rule).  A commit resets wf: the extents were
// measured on the old box; the counters of watch_i are stream totals and go on.
__device__ __forceinline__ void canvas_fit_update(const SsCanvasFit& fit, int s, float guard, float* wf) {
    const float slack = 2.5e-4f;
    const float g = guard > slack ? guard : -slack;
    const float lo = fminf(wf[0], wf[2]), hi = fmaxf(wf[1], wf[3]);
    if (!(lo < __fadd_rn(-1.0f, g) || hi > __fsub_rn(1.0f, g))) return;
    float* box = fit.box + 4 * s;
    const float wmin = box[0], wmax = box[1], hmin = box[2], hmax = box[3];
    const float ow = __fsub_rn(wmax, wmin), oh = __fsub_rn(hmax, hmin);
    float x0 = __fadd_rn(wmin, __fmul_rn(__fmul_rn(__fadd_rn(fminf(wf[0], -1.0f), 1.0f), ow), 0.5f));
    float x1 = __fadd_rn(wmin, __fmul_rn(__fmul_rn(__fadd_rn(fmaxf(wf[1], 1.0f), 1.0f), ow), 0.5f));
    float y0 = __fadd_rn(hmin, __fmul_rn(__fmul_rn(__fadd_rn(fminf(wf[2], -1.0f), 1.0f), oh), 0.5f));
    float y1 = __fadd_rn(hmin, __fmul_rn(__fmul_rn(__fadd_rn(fmaxf(wf[3], 1.0f), 1.0f), oh), 0.5f));
    // (wmin + (wmax - wmin) may round an ulp short of wmax: the needed box is a union, it contains the old one)
    x0 = fminf(x0, wmin); x1 = fmaxf(x1, wmax); y0 = fminf(y0, hmin); y1 = fmaxf(y1, hmax);
    const float gw = __fmul_rn(fit.margin, __fsub_rn(x1, x0)), gh = __fmul_rn(fit.margin, __fsub_rn(y1, y0));
    x0 = __fsub_rn(x0, gw); x1 = __fadd_rn(x1, gw); y0 = __fsub_rn(y0, gh); y1 = __fadd_rn(y1, gh);
    const SsBox fb = canvas_fit_aspect(SsBox{x0, x1, y0, y1}, fit.wout, fit.hout);
    x0 = fb.x0; x1 = fb.x1; y0 = fb.y0; y1 = fb.y1;
    const float big = __FLT_MAX__;       // (finite: |v| <= FLT_MAX is false for an infinity and for a NaN)
    if (!(fabsf(x0) <= big && fabsf(x1) <= big && fabsf(y0) <= big && fabsf(y1) <= big)) return;
    if (__fsub_rn(x1, x0) > __fmul_rn(fit.zoom_limit, fit.ext0[2 * s]) ||
        __fsub_rn(y1, y0) > __fmul_rn(fit.zoom_limit, fit.ext0[2 * s + 1]))
        return;
    const float moved = fmaxf(fmaxf(__fsub_rn(wmin, x0), __fsub_rn(x1, wmax)), fmaxf(__fsub_rn(hmin, y0), __fsub_rn(y1, hmax)));
    if (moved < 0.5f) return;
    box[0] = x0; box[1] = x1; box[2] = y0; box[3] = y1;
    fit.epoch[s] += 1;
    wf[0] = INFINITY; wf[1] = -INFINITY; wf[2] = INFINITY; wf[3] = -INFINITY;
}


#ifdef SS_TUNING
// tools/ build only: buffer for per-workgroup s_memtime stamps (set through ss_debug_ptr, conv.hip)
extern unsigned long long* ss_tuning_dbg;
#endif
