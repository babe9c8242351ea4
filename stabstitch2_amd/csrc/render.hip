// Dense thin-plate-spline warp and fusion (K12/K13).
//
// The reference materialises a [B,66,Hc*Wc] basis tensor (~500 MB at 720p) and makes ~15
// elementwise passes over it before a bmm and a gather.  Here one thread owns one
// canvas pixel: the 63 RBF terms of both views are evaluated together in registers (packed fp32 math,
// hardware log2) from wave-uniform control points / coefficients (scalar loads, no LDS), the sampling coordinate never leaves the register file, the
// bilinear taps are gathered straight from the planar source frames, and for the AVERAGE mode the
// two (three) views are fused before the single store.  HBM traffic = source frames once (L2 absorbs
// the 4-tap overlap) + the canvas once.
#include <type_traits>

#include "common.h"
#include "device_math.h"
#include "nv12.h"

// grid_sample(bilinear, zeros, align_corners=True) taps: x = (xn+1)/2*(W-1), out-of-range taps -> 0
// the four taps of one coordinate: corner indices, weights, and which rows / columns lie inside the image
struct SsFastTaps {
    int x0, y0, x1, y1;
    float w00, w01, w10, w11;
    bool vx0, vx1, vy0, vy1;
};
__device__ __forceinline__ SsFastTaps taps_fast(float xn, float yn, int W, int H) {
    SsFastTaps t;
    float x = ((xn + 1.f) / 2.f) * (float)(W - 1);
    float y = ((yn + 1.f) / 2.f) * (float)(H - 1);
    float xf = fminf(fmaxf(floorf(x), -4.f), (float)W + 4.f);
    float yf = fminf(fmaxf(floorf(y), -4.f), (float)H + 4.f);
    t.x0 = (int)xf; t.y0 = (int)yf; t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
    // ATen grid_sampler_2d: nw = (ix_se - ix)(iy_se - iy), ne = (ix - ix_sw)(iy_sw - iy), ...
    t.w00 = (xf + 1.f - x) * (yf + 1.f - y); t.w01 = (x - xf) * (yf + 1.f - y);
    t.w10 = (xf + 1.f - x) * (y - yf); t.w11 = (x - xf) * (y - yf);
    t.vx0 = (unsigned)t.x0 < (unsigned)W; t.vx1 = (unsigned)t.x1 < (unsigned)W;
    t.vy0 = (unsigned)t.y0 < (unsigned)H; t.vy1 = (unsigned)t.y1 < (unsigned)H;
    return t;
}
__device__ __forceinline__ float sample_fast(const float* __restrict__ pl, float xn, float yn, int W, int H) {
    const SsFastTaps t = taps_fast(xn, yn, W, H);
    float r = 0.f;
    if (t.vx0 && t.vy0) r += pl[(long long)t.y0 * W + t.x0] * t.w00;
    if (t.vx1 && t.vy0) r += pl[(long long)t.y0 * W + t.x1] * t.w01;
    if (t.vx0 && t.vy1) r += pl[(long long)t.y1 * W + t.x0] * t.w10;
    if (t.vx1 && t.vy1) r += pl[(long long)t.y1 * W + t.x1] * t.w11;
    return r;
}

// zero padding on an all-ones plane: sum of the in-range tap weights (grid_sample of a ones image)
__device__ __forceinline__ float fast_mask(float xn, float yn, int w, int h) {
    float xx = ((xn + 1.f) / 2.f) * (float)(w - 1), yy = ((yn + 1.f) / 2.f) * (float)(h - 1);
    float xf = fminf(fmaxf(floorf(xx), -4.f), (float)w + 4.f);
    float yf = fminf(fmaxf(floorf(yy), -4.f), (float)h + 4.f);
    int x0 = (int)xf, y0 = (int)yf;
    bool vx0 = (unsigned)x0 < (unsigned)w, vx1 = (unsigned)(x0 + 1) < (unsigned)w;
    bool vy0 = (unsigned)y0 < (unsigned)h, vy1 = (unsigned)(y0 + 1) < (unsigned)h;
    float r = 0.f;
    if (vx0 && vy0) r += (xf + 1.f - xx) * (yf + 1.f - yy);
    if (vx1 && vy0) r += (xx - xf) * (yf + 1.f - yy);
    if (vx0 && vy1) r += (xf + 1.f - xx) * (yy - yf);
    if (vx1 && vy1) r += (xx - xf) * (yy - yf);
    return r;
}

// Both rows of a wave (tile = 64 columns x 8 rows, wave w owns rows w and w + 4) through tps_eval_rows: the row-only part
// of the radial terms from the wave's own LDS table.  -> normalised sampling coordinates of (x, ya) and (x, yb).
__device__ __forceinline__ void warp_rows_coords(const float* __restrict__ src, const float* __restrict__ T, ss_f2* tab,
                                                 int lane, int x, int ya, int yb, int hc, int wc, ss_f2& xn, ss_f2& yn) {
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
    tps_rows_table(src, gya, gyb, lane, tab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the same wave reads it back: ordering only
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    tps_eval_rows(src, T, tab, gx, gya, gyb, xn, yn);
}

// append_mask: emit one extra channel = warp of an all-ones plane (test_online_tra.py:144-147)
__global__ __launch_bounds__(256) void tps_warp_kernel(const float* __restrict__ U, const float* __restrict__ source,
                                                       const float* __restrict__ T, float* __restrict__ out, int c,
                                                       int h, int w, int hc, int wc, int mode, int append_mask) {
    __shared__ ss_f2 dytab[4][64];
    const int b = blockIdx.z;
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lx;
    const int ya = blockIdx.y * 8 + wv, yb = ya + 4;
    if (ya >= hc) return;                       // whole waves only: lanes past the canvas edge still help build the table
    ss_f2 xn2, yn2;
    warp_rows_coords(source + (long long)b * SS_NV * 2, T + (long long)b * 2 * SS_NT, dytab[wv], lx, x, ya, yb, hc, wc, xn2, yn2);
    if (x >= wc) return;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    const int co = c + (append_mask ? 1 : 0);
    const float* in = U + (long long)b * c * hw;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int y = rr ? yb : ya;
        if (y >= hc) break;
        const float xn = rr ? xn2.y : xn2.x, yn = rr ? yn2.y : yn2.x;
        float* o = out + (long long)b * co * ohw + (long long)y * wc + x;
        if (mode == SS_WARP_NORMAL) {
            SsTaps t = taps_normal(xn, yn, w, h);
            long long ia = (long long)t.y0 * w + t.x0, ib = (long long)t.y1 * w + t.x0;
            long long ic = (long long)t.y0 * w + t.x1, id = (long long)t.y1 * w + t.x1;
            for (int ch = 0; ch < c; ++ch) {
                const float* pl = in + ch * hw;
                o[ch * ohw] = blend4(t, pl[ia], pl[ib], pl[ic], pl[id]);
            }
            if (append_mask) o[c * ohw] = blend4(t, 1.f, 1.f, 1.f, 1.f);
        } else {
            for (int ch = 0; ch < c; ++ch) o[ch * ohw] = sample_fast(in + ch * hw, xn, yn, w, h);
            if (append_mask) o[c * ohw] = fast_mask(xn, yn, w, h);
        }
    }
}

static int launch_warp(const float* U, const float* source, const float* T, float* out, int b, int c, int h, int w,
                       int hc, int wc, int mode, int append_mask, void* stream) {
    if (!U || !source || !T || !out || b <= 0 || c <= 0 || h <= 1 || w <= 1 || hc <= 1 || wc <= 1 ||
        (mode != SS_WARP_NORMAL && mode != SS_WARP_FAST) || b > 65535 || ss_cdiv(hc, 8) > 65535)      // (items and row tiles: grid.z, grid.y)
        return SS_ERR_ARG;
    dim3 g(ss_cdiv(wc, 64), ss_cdiv(hc, 8), b);
    hipLaunchKernelGGL(tps_warp_kernel, g, dim3(256), 0, (hipStream_t)stream, U, source, T, out, c, h, w, hc, wc, mode,
                       append_mask);
    return ss_launch_status();
}

extern "C" int ss_tps_warp_nchw(const float* U, const float* source, const float* T, float* out, int b, int c, int h,
                                int w, int hc, int wc, int mode, void* stream) {
    return launch_warp(U, source, T, out, b, c, h, w, hc, wc, mode, 0, stream);
}

extern "C" int ss_tps_warp_mask_nchw(const float* U, const float* source, const float* T, float* out, int b, int c,
                                     int h, int w, int hc, int wc, int mode, void* stream) {
    return launch_warp(U, source, T, out, b, c, h, w, hc, wc, mode, 1, stream);
}

// ------------------------------------------------------------------------------------------------
// fused render, AVERAGE fusion (test_online_tra.py:138-142; three-view chaining threeview:486-490)
struct RenderViews {
    const float* img[3];
};
// the same views with per-view, per-channel exposure gains [frames][views][3] (ss_exposure_update): a sampled value s of view v,
// channel c enters the fusion as fminf(g[v][c] * s, 255) -- the clamp because the uint8 sink wraps (render_to_u8)
struct GainViews : RenderViews {
    const float* gains;
};
__device__ __forceinline__ void apply_gains(const float* __restrict__ g, float (&v)[3]) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = fminf(__fmul_rn(g[ch], v[ch]), 255.f);
}
// a descriptor of frame 0 -> of frame f: image pointers by img_fs BYTES, gains by VIEWS * 3, NV12 planes by their own fs[k]
template <int VIEWS>
__device__ __forceinline__ void views_to_frame(RenderViews& rv, long long f, long long img_fs) {
#pragma unroll
    for (int k = 0; k < VIEWS; ++k)
        rv.img[k] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(rv.img[k]) + f * img_fs);
}
template <int VIEWS>
__device__ __forceinline__ void views_to_frame(GainViews& rv, long long f, long long img_fs) {
    views_to_frame<VIEWS>(static_cast<RenderViews&>(rv), f, img_fs);
    rv.gains += f * (VIEWS * 3);
}
template <int VIEWS>
__device__ __forceinline__ void views_to_frame(Nv12Views& nv, long long f) {
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) { nv.y[k] += f * nv.fs[k]; nv.uv[k] += f * nv.fs[k]; }
}

// ---- host dispatch: the run-time (views, u8, ..) of an entry point as compile-time constants, so that a launcher names each of its
// kernels once: f gets one std::bool_constant per flag / std::integral_constant<int, VIEWS> and instantiates on their values
template <typename F>
static void with_flags(bool b0, bool b1, F&& f) {
    if (b0) { if (b1) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else { if (b1) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}
template <typename F>
static void with_views(int views, bool u8, F&& f) {       // views = 2 or 3: every caller has checked it
    with_flags(views == 3, u8, [&](auto three, auto U8) { f(std::integral_constant<int, decltype(three)::value ? 3 : 2>{}, U8); });
}
// the view pointers of an entry point (+ its exposure gains, nullptr without) -> the kernels' descriptor; false: a view is missing
static bool views_make(GainViews& gv, const void* const* imgs, int views, const float* gains) {
    for (int i = 0; i < 3; ++i) gv.img[i] = i < views ? static_cast<const float*>(imgs[i]) : nullptr;
    gv.gains = gains;
    for (int i = 0; i < views; ++i)
        if (!gv.img[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void tps_warp_views_kernel(RenderViews rv, const float* __restrict__ source,
                                                             const float* __restrict__ T, float* __restrict__ out,
                                                             int h, int w, int hc, int wc, int mode) {
    __shared__ ss_f2 dytab[4][64];
    const int b = blockIdx.z;
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lx;
    const int ya = blockIdx.y * 8 + wv, yb = ya + 4;
    if (ya >= hc) return;
    ss_f2 xn2, yn2;
    warp_rows_coords(source + (long long)b * SS_NV * 2, T + (long long)b * 2 * SS_NT, dytab[wv], lx, x, ya, yb, hc, wc, xn2, yn2);
    if (x >= wc) return;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    const float* in = b == 0 ? rv.img[0] : (b == 1 ? rv.img[1] : rv.img[2]);
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int y = rr ? yb : ya;
        if (y >= hc) break;
        const float xn = rr ? xn2.y : xn2.x, yn = rr ? yn2.y : yn2.x;
        float* o = out + (long long)b * 4 * ohw + (long long)y * wc + x;
        if (mode == SS_WARP_NORMAL) {
            SsTaps t = taps_normal(xn, yn, w, h);
            long long ia = (long long)t.y0 * w + t.x0, ib = (long long)t.y1 * w + t.x0;
            long long ic = (long long)t.y0 * w + t.x1, id = (long long)t.y1 * w + t.x1;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* pl = in + ch * hw;
                o[ch * ohw] = blend4(t, pl[ia], pl[ib], pl[ic], pl[id]);
            }
            o[3 * ohw] = blend4(t, 1.f, 1.f, 1.f, 1.f);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch * ohw] = sample_fast(in + ch * hw, xn, yn, w, h);
            o[3 * ohw] = fast_mask(xn, yn, w, h);
        }
    }
}

extern "C" int ss_tps_warp_views(const float* const* imgs, const float* source, const float* T, float* out, int views,
                                 int h, int w, int hc, int wc, int mode, void* stream) {
    if (!imgs || !source || !T || !out || views < 1 || views > 3 || h <= 1 || w <= 1 || hc <= 1 || wc <= 1 ||
        (mode != SS_WARP_NORMAL && mode != SS_WARP_FAST))
        return SS_ERR_ARG;
    RenderViews rv;
    for (int i = 0; i < 3; ++i) rv.img[i] = i < views ? imgs[i] : nullptr;
    for (int i = 0; i < views; ++i)
        if (!rv.img[i]) return SS_ERR_ARG;
    dim3 g(ss_cdiv(wc, 64), ss_cdiv(hc, 8), views);
    hipLaunchKernelGGL(tps_warp_views_kernel, g, dim3(256), 0, (hipStream_t)stream, rv, source, T, out, h, w, hc, wc,
                       mode);
    return ss_launch_status();
}

// small canvas-sized elementwise helpers of the harnesses
__global__ void affine_kernel(const float* __restrict__ in, float* __restrict__ out, float add, float mul, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __fmul_rn(__fadd_rn(in[i], add), mul);
}
extern "C" int ss_add_mul(const float* in, float* out, float add, float mul, long long n, void* stream) {
    if (!in || !out || n <= 0) return SS_ERR_ARG;
    hipLaunchKernelGGL(affine_kernel, dim3(ss_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, in, out, add, mul, n);
    return ss_launch_status();
}
__global__ void mask_union_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                  long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __fsub_rn(__fadd_rn(a[i], b[i]), __fmul_rn(a[i], b[i]));
}
extern "C" int ss_mask_union(const float* a, const float* b, float* out, long long n, void* stream) {
    if (!a || !b || !out || n <= 0) return SS_ERR_ARG;
    hipLaunchKernelGGL(mask_union_kernel, dim3(ss_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
    return ss_launch_status();
}

__device__ __forceinline__ float avg_fuse(float a, float b) {
    float s = __fadd_rn(__fadd_rn(a, b), 1e-6f);
    return __fadd_rn(__fmul_rn(a, a / s), __fmul_rn(b, b / s));
}

// ---- footprints: which 64 x 8 canvas tiles can a view contribute to? -------------------------------------------------
// Outside a view's footprint the reference's clamped-index sampler returns no image content, only the rounding residue
// of (P + Q) - P - Q (|r| <~ 1e-2 grey levels, different on every machine -- DESIGN.md 4); yet those pixels cost the full
// 63-term spline evaluation, and on the benchmark canvas a third of all (pixel, view) pairs lie there.  With a footprint
// block the fused render skips them and treats the view's contribution as exactly 0.
//   lattice[v][i][j] = (xn, yn) = sampling coordinate of view v at canvas pixel (x = 32 j, y = 8 i), i <= ceil(hc / 8),
//   j <= 2 ceil(wc / 64) (half-tile spacing along the long side of a tile: a tile is judged on its four corners AND the
//   midpoints of its two long edges; the last row / column lies on or beyond the canvas edge: the spline is defined everywhere);
//   hull[v] = (xmin, xmax, ymin, ymax): bounding box of the view's 63 control points in normalised canvas coordinates --
//   the view's mesh on the canvas; its border vertices map exactly onto the image border (TPS interpolation).
// A tile is OUTSIDE view v when BOTH hold:
//   (a) it lies outside the mesh hull grown by 8 canvas pixels, and
//   (b) the exactly evaluated sampling coordinates of its four corners and two long-edge midpoints all lie beyond the same
//       image side by more than 8 source pixels (to come back, the spline would have to bend by 8 px within 32 canvas
//       pixels OUTSIDE its own mesh hull, where it has no control points and extrapolates smoothly).
// This is a test, not a proof: callers who need the reference's arithmetic at every pixel pass footprint = NULL.
// (A rigorous interpolation-error bound from sum |T_k| was tried instead of (b)'s fixed margin: the RBF weights of a
// near-affine warp cancel, the bound does not -- it came out at 100-140 source pixels and kept a third of the skippable
// tiles.)  tests/test_gpu_parity.py::test_render_footprint_skipping checks on pipeline meshes that every skipped pixel is
// outside (validity mask of the full evaluation ~ 0) and that nothing else changes.
// FIT (a compile-time flag: a new instantiation, FIT = 0 is the kernel as it was): the wave that ran the watcher goes on with
// canvas_fit_update (common.h) on its stream's box -- the box's last reader of the push is the splines launch in front of this one,
// and nothing else in this launch looks at it.
// (the fit's state is a parameter of the FIT instantiation only: `Fit` is SsCanvasFit there and empty for FIT = 0)
template <int FIT, typename... Fit>
__global__ void render_lattice_kernel(const float* __restrict__ source, const float* __restrict__ T,
                                      float* __restrict__ fp, long long frame_stride, int views, int hc, int wc,
                                      int ny, int nx, float guard, int* __restrict__ watch_i, float* __restrict__ watch_f,
                                      Fit... fits) {
    const int fv = blockIdx.y;                       // frame * views + view
    const int frame = fv / views, view = fv - frame * views;
    float* lattice = fp + frame * frame_stride + (long long)view * ny * nx * 2;
    float* margin = fp + frame * frame_stride + (long long)views * ny * nx * 2 + 4 * view;       // hull (xmin, xmax, ymin, ymax)
    const float* src = source + (long long)fv * SS_NV * 2;
    const float* Tx = T + (long long)fv * 2 * SS_NT;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && view == 0 && threadIdx.x >= 64 && threadIdx.x < 68)       // the frame's tile-class counters (render_order_kernel)
        reinterpret_cast<unsigned*>(fp + frame * frame_stride + (long long)views * ny * nx * 2 + 4 * views)[threadIdx.x - 64] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 2) {       // hull of the control points: thread 0 -> x range, thread 1 -> y range
        float lo = INFINITY, hi = -INFINITY;
        for (int k = 0; k < SS_NV; ++k) {
            const float c = src[2 * k + threadIdx.x];
            lo = fminf(lo, c);
            hi = fmaxf(hi, c);
        }
        margin[2 * threadIdx.x] = lo;
        margin[2 * threadIdx.x + 1] = hi;
    }
    if (watch_i && blockIdx.x == 0 && view == 0 && threadIdx.x < 64) {
        // the streaming canvas' overflow watcher over ALL views of this frame (canvas_watch_kernel's arithmetic; frame = stream):
        // the control points are read here anyway, and a launch of its own is a node on the push's critical path
        const float* s = source + (long long)frame * views * SS_NV * 2;
        float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
        bool bad = false;
        for (int k = threadIdx.x; k < views * SS_NV; k += 64) {
            const float x = s[2 * k], y = s[2 * k + 1];
            bad = bad || x != x || y != y;
            xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
            ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
        }
        canvas_watch_update(xmin, xmax, ymin, ymax, bad, guard, watch_i + frame * 4, watch_f + frame * 4);
        if constexpr (FIT == 1) {
            if (threadIdx.x == 0) canvas_fit_update((fits, ...), frame, guard, watch_f + frame * 4);
        }
    }
    if (idx >= ny * nx) return;
    const int i = idx / nx, j = idx - i * nx;
    const float gx = -1.f + 2.f * (float)(32 * j) / (float)(wc - 1), gy = -1.f + 2.f * (float)(8 * i) / (float)(hc - 1);
    float xn, yn;
    tps_eval_fast(src, Tx, Tx + SS_NT, gx, gy, xn, yn);
    lattice[idx * 2] = xn;
    lattice[idx * 2 + 1] = yn;
}

// bit v set = view v may contribute to tile (by, bx)
__device__ __forceinline__ unsigned tile_views(const float* __restrict__ fp, int views, int by, int bx, int ny, int nx,
                                               int h, int w, int hc, int wc) {
    const float* hull = fp + (long long)views * ny * nx * 2;
    // the tile in normalised canvas coordinates, grown by 8 canvas pixels
    const float sxn = 2.f / (float)(wc - 1), syn = 2.f / (float)(hc - 1);
    const float tx0 = -1.f + sxn * (float)(64 * bx - 8), tx1 = -1.f + sxn * (float)(64 * bx + 63 + 8);
    const float ty0 = -1.f + syn * (float)(8 * by - 8), ty1 = -1.f + syn * (float)(8 * by + 7 + 8);
    const float mx = 1.f + 16.f / (float)w, my = 1.f + 16.f / (float)h;       // 8 source pixels beyond the image
    unsigned mask = 0u;
    for (int v = 0; v < views; ++v) {
        const float* L = fp + ((long long)v * ny * nx + (long long)by * nx + 2 * bx) * 2;      // lattice column 2 bx = pixel 64 bx
        float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {            // corners and long-edge midpoints
                const float xs = L[(r * nx + c) * 2], ys = L[(r * nx + c) * 2 + 1];
                xlo = fminf(xlo, xs); xhi = fmaxf(xhi, xs);
                ylo = fminf(ylo, ys); yhi = fmaxf(yhi, ys);
            }
        const bool off_hull = tx1 < hull[4 * v] || tx0 > hull[4 * v + 1] || ty1 < hull[4 * v + 2] || ty0 > hull[4 * v + 3];
        const bool off_image = xlo > mx || xhi < -mx || ylo > my || yhi < -my;
        if (!(off_hull && off_image)) mask |= 1u << v;
    }
    return mask;
}


// Tile order of one frame: the fused render takes its tiles most expensive class first (tiles reached by 3, 2, 1, 0 views cost
// ~2 : 1 : 0.5 : 0 spline evaluations per pixel).  With ~11 workgroups per CU and mixed costs a row-major order left the CUs 25 %
// apart (measured: 55 us per frame against 45 for the cost-weighted sum of the tile classes); longest-first hands the expensive
// tiles out evenly and fills in with the cheap ones.
//   entry = bx | by << 12 | mask << 24
// Round 6: one LIST per class (4 x nt entries behind 4 counters that render_lattice_kernel zeroes) instead of one sorted table: a
// tile's slot no longer depends on the totals of the classes in front of it, so the tiles are classified by nt / 256 workgroups,
// one tile per thread, one global atomic per wave and class -- 3-4 us instead of the single workgroup's 9 (two views, 3100 tiles) /
// 16 us (three views, 4158) on a streaming push's critical path.  The render finds its tile from the counters (render_tile_entry).
// Which tile a workgroup of a class gets depends on the atomics' arrival order; every tile is still rendered exactly once.
__global__ __launch_bounds__(256) void render_order_kernel(float* __restrict__ fp, long long frame_stride, int views, int h,
                                                           int w, int hc, int wc, int ny, int nx) {
    float* f = fp + (long long)blockIdx.y * frame_stride;
    unsigned* cnt = reinterpret_cast<unsigned*>(f + (long long)views * ny * nx * 2 + 4 * views);
    unsigned* lists = cnt + 4;
    const int nbx = (nx - 1) / 2, nby = ny - 1, nt = nbx * nby;
    const int t = blockIdx.x * 256 + (int)threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int by = t / nbx, bx = t - by * nbx;
    const unsigned mm = t < nt ? tile_views(f, views, by, bx, ny, nx, h, w, hc, wc) : 0xFFu;
    const int c = mm == 0xFFu ? -1 : 3 - __popc(mm);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long b = __ballot(c == k);
        if (b == 0ull) continue;                    // (wave-uniform)
        unsigned wb = 0u;
        if (lane == 0) wb = atomicAdd(&cnt[k], (unsigned)__popcll(b));
        wb = (unsigned)__shfl((int)wb, 0, 64);
        if (c == k) lists[(long long)k * nt + wb + (unsigned)__popcll(b & below)] = (unsigned)bx | ((unsigned)by << 12) | (mm << 24);
    }
}

// the i-th tile of a frame in cost order: class lists back to back
__device__ __forceinline__ unsigned render_tile_entry(const float* __restrict__ fp, int views, int ny, int nx, unsigned i) {
    const unsigned* cnt = reinterpret_cast<const unsigned*>(fp + (long long)views * ny * nx * 2 + 4 * views);
    const unsigned nt = (unsigned)((nx - 1) / 2 * (ny - 1));
    const unsigned c0 = cnt[0], c1 = cnt[1], c2 = cnt[2];
    unsigned k = 0u, off = i;
    if (i >= c0) { k = 1u; off = i - c0; }
    if (i >= c0 + c1) { k = 2u; off = i - c0 - c1; }
    if (i >= c0 + c1 + c2) { k = 3u; off = i - c0 - c1 - c2; }
    return cnt[4 + (unsigned long long)k * nt + off];
}

// this workgroup's tile (tbx, tby) of its frame -> the views that reach it: from the frame's order table (longest first), or, without
// a footprint, row-major and every view
template <int VIEWS>
__device__ __forceinline__ unsigned render_tile(const float* __restrict__ fp, int hc, int wc, int& tbx, int& tby) {
    const int ny = (hc + 7) / 8 + 1, nx = 2 * ((wc + 63) / 64) + 1, nbx = (nx - 1) / 2;
    if (fp) {
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)render_tile_entry(fp, VIEWS, ny, nx, blockIdx.x));
        tbx = (int)(e & 0xFFFu); tby = (int)((e >> 12) & 0xFFFu);
        return e >> 24;
    }
    tby = blockIdx.x / nbx; tbx = blockIdx.x - tby * nbx;
    return (1u << VIEWS) - 1u;
}

extern "C" long long ss_render_footprint_floats(int views, int hc, int wc) {
    if (views <= 0 || hc <= 1 || wc <= 1) return 0;
    return (long long)views * ((long long)(ss_cdiv(hc, 8) + 1) * (2 * ss_cdiv(wc, 64) + 1) * 2 + 4) +
           4 + 4ll * ss_cdiv(hc, 8) * ss_cdiv(wc, 64);       // + 4 class counters + 4 class lists of tiles
}

// footprints of `frames` x `views` splines in one launch: fp [frames][ lattice [views][ny][nx][2] | margin [views][2] ]
template <int FIT>
static int render_footprints_launch(const float* source, const float* T, float* fp, int frames, int views, int h, int w,
                                    int hc, int wc, float guard, int* watch_i, float* watch_f, SsCanvasFit fit, void* stream) {
    if (!source || !T || !fp || frames <= 0 || views <= 0 || views > 3 || h <= 1 || w <= 1 || hc <= 1 || wc <= 1)
        return SS_ERR_ARG;
    const int ny = ss_cdiv(hc, 8) + 1, nx = 2 * ss_cdiv(wc, 64) + 1;
    // the footprint of frame f (lattice of every view, then the margins) lives at fp + f * ss_render_footprint_floats(...)
    const long long stride = ss_render_footprint_floats(views, hc, wc);
    if (ny > 4096 || nx > 4096) return SS_ERR_UNSUPPORTED;
    // grid.y = (frame, view), capped at 65535 by HIP: whole frames per launch
    const int fmax = 65535 / views;
    for (int f0 = 0; f0 < frames; f0 += fmax) {
        const int nf = frames - f0 < fmax ? frames - f0 : fmax;
        const float* src0 = source + (long long)f0 * views * SS_NV * 2;
        const float* T0 = T + (long long)f0 * views * 2 * SS_NT;
        int* wi0 = watch_i ? watch_i + 4 * f0 : nullptr;
        float* wf0 = watch_f ? watch_f + 4 * f0 : nullptr;
        if constexpr (FIT == 1) {
            SsCanvasFit fit0 = fit;                 // (this launch's frame 0 is stream f0)
            fit0.box += 4 * f0; fit0.epoch += f0; fit0.ext0 += 2 * f0;
            hipLaunchKernelGGL((render_lattice_kernel<1, SsCanvasFit>), dim3(ss_cdiv(ny * nx, 128), nf * views), dim3(128), 0,
                               (hipStream_t)stream, src0, T0, fp + (long long)f0 * stride, stride, views, hc, wc, ny, nx, guard, wi0, wf0,
                               fit0);
        } else {
            hipLaunchKernelGGL(render_lattice_kernel<0>, dim3(ss_cdiv(ny * nx, 128), nf * views), dim3(128), 0, (hipStream_t)stream,
                               src0, T0, fp + (long long)f0 * stride, stride, views, hc, wc, ny, nx, guard, wi0, wf0);
        }
    }
    const int nt = (ny - 1) * ((nx - 1) / 2);
    for (int f0 = 0; f0 < frames; f0 += 65535) {
        const int nf = frames - f0 < 65535 ? frames - f0 : 65535;
        hipLaunchKernelGGL(render_order_kernel, dim3(ss_cdiv(nt, 256), nf), dim3(256), 0, (hipStream_t)stream, fp + (long long)f0 * stride,
                           stride, views, h, w, hc, wc, ny, nx);
    }
    return ss_launch_status();
}

extern "C" int ss_render_footprints(const float* source, const float* T, float* fp, int frames, int views, int h, int w,
                                    int hc, int wc, void* stream) {
    return render_footprints_launch<0>(source, T, fp, frames, views, h, w, hc, wc, 0.f, nullptr, nullptr, SsCanvasFit{}, stream);
}

// the same + the streaming canvas' overflow watcher (ss_canvas_watch's update of watch_i / watch_f [frames][4], frame = stream) inside
// the lattice launch: `source` is what the watcher reads, and the push saves a graph node
extern "C" int ss_render_footprints_watch(const float* source, const float* T, float* fp, int frames, int views, int h, int w,
                                          int hc, int wc, float guard, int* watch_i, float* watch_f, void* stream) {
    if (!watch_i || !watch_f || !(guard >= 0.f)) return SS_ERR_ARG;
    return render_footprints_launch<0>(source, T, fp, frames, views, h, w, hc, wc, guard, watch_i, watch_f, SsCanvasFit{}, stream);
}

// the same + the device-side refit of the streams' boxes (canvas_fit_update: ss_canvas_watch_fit has the state's layout) behind the
// watcher, in the same wave; the viewport is the canvas size hc x wc itself
extern "C" int ss_render_footprints_watch_fit(const float* source, const float* T, float* fp, int frames, int views, int h, int w,
                                              int hc, int wc, float guard, int* watch_i, float* watch_f, float* box, int* epoch,
                                              const float* ext0, float margin, float zoom_limit, void* stream) {
    if (!watch_i || !watch_f || !(guard >= 0.f) || !box || !epoch || !ext0 || !(margin >= 0.f) || !(zoom_limit >= 0.f) ||
        frames <= 0 || hc < 11 || hc > 65535 || wc < 11 || wc > 65535)
        return SS_ERR_ARG;
    SsCanvasFit fit;
    fit.box = box; fit.epoch = epoch; fit.ext0 = const_cast<float*>(ext0);       // (read only by canvas_fit_update)
    fit.margin = margin; fit.zoom_limit = zoom_limit; fit.wout = (float)wc; fit.hout = (float)hc;
    return render_footprints_launch<1>(source, T, fp, frames, views, h, w, hc, wc, guard, watch_i, watch_f, fit, stream);
}

__device__ __forceinline__ void sample3(const float* __restrict__ in, float xn, float yn, int w, int h, long long hw, int mode,
                                        float (&v)[3]) {
    if (mode == SS_WARP_NORMAL) {
        SsTaps t = taps_normal(xn, yn, w, h);
        long long ia = (long long)t.y0 * w + t.x0, ib = (long long)t.y1 * w + t.x0;
        long long ic = (long long)t.y0 * w + t.x1, id = (long long)t.y1 * w + t.x1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* pl = in + ch * hw;
            v[ch] = blend4(t, pl[ia], pl[ib], pl[ic], pl[id]);
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = sample_fast(in + ch * hw, xn, yn, w, h);
    }
}

// the same samples from a decoded uint8 frame [h][w][3] (what cv2.imread hands the reference, test_online_tra.py:252-258):
// uint8 -> fp32 is exact, so the values equal those of sample3 on the converted planes bit for bit
__device__ __forceinline__ void sample3_u8(const unsigned char* __restrict__ in, float xn, float yn, int w, int h, int mode,
                                           float (&v)[3]) {
    if (mode == SS_WARP_NORMAL) {
        SsTaps t = taps_normal(xn, yn, w, h);
        const long long ia = ((long long)t.y0 * w + t.x0) * 3, ib = ((long long)t.y1 * w + t.x0) * 3;
        const long long ic = ((long long)t.y0 * w + t.x1) * 3, id = ((long long)t.y1 * w + t.x1) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            v[ch] = blend4(t, (float)in[ia + ch], (float)in[ib + ch], (float)in[ic + ch], (float)in[id + ch]);
    } else {
        const SsFastTaps t = taps_fast(xn, yn, w, h);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {            // sample_fast, term by term
            float r = 0.f;
            if (t.vx0 && t.vy0) r += (float)in[((long long)t.y0 * w + t.x0) * 3 + ch] * t.w00;
            if (t.vx1 && t.vy0) r += (float)in[((long long)t.y0 * w + t.x1) * 3 + ch] * t.w01;
            if (t.vx0 && t.vy1) r += (float)in[((long long)t.y1 * w + t.x0) * 3 + ch] * t.w10;
            if (t.vx1 && t.vy1) r += (float)in[((long long)t.y1 * w + t.x1) * 3 + ch] * t.w11;
            v[ch] = r;
        }
    }
}
// the same samples from a decoded NV12 frame: every tap's B, G, R are nv12_to_bgr of the tap's Y byte and of the chroma pair of
// its 2 x 2 block (nv12.h), so the values equal those of sample3_u8 on the converted frame bit for bit
__device__ __forceinline__ void sample3_nv12(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp, int pitch,
                                             float xn, float yn, int w, int h, int mode, float (&v)[3]) {
    int a[3] = {0, 0, 0}, b[3] = {0, 0, 0}, c[3] = {0, 0, 0}, d[3] = {0, 0, 0};
    if (mode == SS_WARP_NORMAL) {
        SsTaps t = taps_normal(xn, yn, w, h);
        nv12_pixel(yp, uvp, pitch, t.y0, t.x0, a);
        nv12_pixel(yp, uvp, pitch, t.y1, t.x0, b);
        nv12_pixel(yp, uvp, pitch, t.y0, t.x1, c);
        nv12_pixel(yp, uvp, pitch, t.y1, t.x1, d);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = blend4(t, (float)a[ch], (float)b[ch], (float)c[ch], (float)d[ch]);
    } else {
        const SsFastTaps t = taps_fast(xn, yn, w, h);
        if (t.vx0 && t.vy0) nv12_pixel(yp, uvp, pitch, t.y0, t.x0, a);
        if (t.vx1 && t.vy0) nv12_pixel(yp, uvp, pitch, t.y0, t.x1, b);
        if (t.vx0 && t.vy1) nv12_pixel(yp, uvp, pitch, t.y1, t.x0, c);
        if (t.vx1 && t.vy1) nv12_pixel(yp, uvp, pitch, t.y1, t.x1, d);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {            // sample_fast, term by term
            float r = 0.f;
            if (t.vx0 && t.vy0) r += (float)a[ch] * t.w00;
            if (t.vx1 && t.vy0) r += (float)b[ch] * t.w01;
            if (t.vx0 && t.vy1) r += (float)c[ch] * t.w10;
            if (t.vx1 && t.vy1) r += (float)d[ch] * t.w11;
            v[ch] = r;
        }
    }
}
__device__ __forceinline__ unsigned char render_to_u8(float v) {          // `.astype(np.uint8)` (frameio.hip to_u8)
    if (!(fabsf(v) < 2147483648.f)) return 0;
    return (unsigned char)((unsigned)((int)v) & 255u);
}

// fp == nullptr: every view is evaluated at every pixel (the reference's arithmetic everywhere, residues included);
// otherwise tiles are classified by `tile_views` and a view that cannot reach a tile contributes exactly 0 there.
// U8: frames are decoded uint8 [h][w][3] and the canvas is written as the video frame uint8 [hc][wc][3] (`.astype(np.uint8)`
// of the fused values, test_online_tra.py:413) -- the fp32 frame planes and the fp32 canvas never exist in memory.
// One launch renders a whole clip: blockIdx.y = frame (the hardware hands out a frame's tiles, most expensive first,
// then the next frame's: the light tail of one frame runs beside the heavy head of the next -- 32 launch boundaries and
// 32 partially filled last rounds per clip less than one launch per frame).  Per-frame strides: `img_fs` / `out_fs` in
// BYTES (frames of a view / canvases are equally spaced), `fp_fs` in floats; source [frame][VIEWS][63][2], T [frame][VIEWS][2][66].
// Views = RenderViews, or GainViews: every sampled value scaled and clamped before the fusion sees it (a view the footprint skips
// still contributes exactly 0).  One definition for both, and a template of the KERNEL rather than a shared device body behind thin
// kernels: this way every instantiation keeps its machine code (LAB_NOTES.md, "Source-only changes").
template <int VIEWS, bool U8, bool FOLD = false, typename Views>
__global__ __launch_bounds__(256) void render_average_kernel(Views rv, const float* __restrict__ source,
                                                             const float* __restrict__ T, const float* __restrict__ fp,
                                                             float* __restrict__ out, int h, int w, int hc, int wc,
                                                             int mode, long long img_fs, long long out_fs,
                                                             long long fp_fs) {
    {
        const long long frame = blockIdx.y;
        source += frame * (VIEWS * SS_NV * 2);
        T += frame * (VIEWS * 2 * SS_NT);
        if (fp) fp += frame * fp_fs;
        out = reinterpret_cast<float*>(reinterpret_cast<char*>(out) + frame * out_fs);
        views_to_frame<VIEWS>(rv, frame, img_fs);
    }
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out);
    // workgroup = 64 x 8 canvas pixels; wave w owns rows w and w + 4 of the tile and evaluates, for every view that
    // reaches the tile, that view's spline at its 64 columns of both rows (packed over the rows)
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    int tbx, tby;
    unsigned mask = render_tile<VIEWS>(fp, hc, wc, tbx, tby);
    const int x = tbx * 64 + lx;
#ifdef SS_TUNING
    if ((mode >> 8) == 9) mask = ((tbx + tby) & 1) ? 3u : 1u;          // checkerboard of single / both
    else if ((mode >> 8) == 10) mask = (tbx < (wc + 63) / 64 / 2) ? 1u : 3u;        // left half single, right half both
    else if (mode >> 8) mask = (unsigned)(mode >> 8) - 1u;          // forced tile class (timing experiments)
    mode &= 0xFF;
#endif
    const int ya = tby * 8 + wv, yb = ya + 4;
    if (tbx * 64 >= wc || ya >= hc) return;       // (whole waves only: the lanes past the canvas edge still help build the table)
    const bool xin = x < wc;
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    if (mask == 0u) {                               // no view reaches this tile: avg_fuse(0, 0) = 0
        if (xin) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                if (U8) {
                    out8[((long long)ya * wc + x) * 3 + ch] = 0;
                    if (yb < hc) out8[((long long)yb * wc + x) * 3 + ch] = 0;
                } else {
                    out[ch * ohw + (long long)ya * wc + x] = 0.f;
                    if (yb < hc) out[ch * ohw + (long long)yb * wc + x] = 0.f;
                }
            }
        }
        return;
    }
    // every view that reaches the tile: its spline at this lane's column of the wave's two rows (packed over the rows);
    // the row-only part of the radial terms comes from a per-wave LDS table (tps_rows_table)
    __shared__ ss_f2 dytab[4][VIEWS][64];
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
#pragma unroll
    for (int k = 0; k < VIEWS; ++k)
        if (mask & (1u << k)) tps_rows_table<FOLD>(source + k * SS_NV * 2, gya, gyb, lx, dytab[wv][k]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // same wave reads it back: ordering only, no barrier
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float va[VIEWS][3], vb[VIEWS][3];
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) {
        if (mask & (1u << k)) {
            ss_f2 px, py;
            tps_eval_rows<FOLD>(source + k * SS_NV * 2, T + k * 2 * SS_NT, dytab[wv][k], gx, gya, gyb, px, py);
            if (U8) {
                const unsigned char* img8 = reinterpret_cast<const unsigned char*>(rv.img[k]);
                sample3_u8(img8, px.x, py.x, w, h, mode, va[k]);
                sample3_u8(img8, px.y, py.y, w, h, mode, vb[k]);
            } else {
                sample3(rv.img[k], px.x, py.x, w, h, hw, mode, va[k]);
                sample3(rv.img[k], px.y, py.y, w, h, hw, mode, vb[k]);
            }
            if constexpr (std::is_same<Views, GainViews>::value) {
                apply_gains(rv.gains + k * 3, va[k]);
                apply_gains(rv.gains + k * 3, vb[k]);
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { va[k][ch] = 0.f; vb[k][ch] = 0.f; }
        }
    }
    if (!xin) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        // the chained fusion in the reference's order ((1 (+) 2) (+) 3), zeros in the places of views that do not reach
        float fa = avg_fuse(va[0][ch], va[1][ch]), fb = avg_fuse(vb[0][ch], vb[1][ch]);
        if (VIEWS == 3) { fa = avg_fuse(fa, va[2][ch]); fb = avg_fuse(fb, vb[2][ch]); }
        if (U8) {
            out8[((long long)ya * wc + x) * 3 + ch] = render_to_u8(fa);
            if (yb < hc) out8[((long long)yb * wc + x) * 3 + ch] = render_to_u8(fb);
        } else {
            out[ch * ohw + (long long)ya * wc + x] = fa;
            if (yb < hc) out[ch * ohw + (long long)yb * wc + x] = fb;
        }
    }
}

// ---- FEATHER fusion (SS_FUSE_FEATHER; not the reference's -- the border-distance weights of panorama tools) ----------
// Per canvas pixel, with view v's normalised sampling coordinate (xn_v, yn_v) and its sampled channels c_v (the samplers above,
// after apply_gains where gains are given), fp32, one rounding per operation:
//     w_v = fmaxf(fminf(1 - |xn_v|, 1 - |yn_v|), 0);   num = sum_v w_v c_v,  den = sum_v w_v  (in the order of the views);
//     out = den > 0 ? num / den : 0
// A view the footprint skips has w_v = 0: exact, since a skipped tile lies outside the image, where 1 - |xn| < 0 -- the render with
// a footprint equals the render without one.  All views at once and symmetric in them, where AVERAGE chains ((1 (+) 2) (+) 3).
// The fused render "with another fusion formula": a second template of the same name under the same parameter lists, told apart
// by a leading tag type, so that the AVERAGE instantiations keep their names and their machine code.  The new kernels have no
// machine code to keep: they share one device body (feather_rows), and sums are accumulated view by view -- 2 x (3 + 1) live
// values instead of the 2 x 3 x VIEWS samples the chained fusion holds.
struct FeatherFuse {};
__device__ __forceinline__ float feather_weight(float xn, float yn) {
    return fmaxf(fminf(__fsub_rn(1.f, fabsf(xn)), __fsub_rn(1.f, fabsf(yn))), 0.f);
}
// both rows of a lane (tps_eval_rows) through every view of `mask`: sample(k, xn, yn, v) fills view k's three channels
template <int VIEWS, typename Sample>
__device__ __forceinline__ void feather_rows(unsigned mask, const float* __restrict__ source, const float* __restrict__ T,
                                             ss_f2 (*tab)[64], int lx, float gx, float gya, float gyb, Sample&& sample,
                                             float (&fa)[3], float (&fb)[3]) {
#pragma unroll
    for (int k = 0; k < VIEWS; ++k)
        if (mask & (1u << k)) tps_rows_table(source + k * SS_NV * 2, gya, gyb, lx, tab[k]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // same wave reads it back: ordering only, no barrier
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float na[3] = {0.f, 0.f, 0.f}, nb[3] = {0.f, 0.f, 0.f}, da = 0.f, db = 0.f;
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) {
        if (mask & (1u << k)) {
            ss_f2 px, py;
            tps_eval_rows(source + k * SS_NV * 2, T + k * 2 * SS_NT, tab[k], gx, gya, gyb, px, py);
            float va[3], vb[3];
            sample(k, px.x, py.x, va);
            sample(k, px.y, py.y, vb);
            const float wa = feather_weight(px.x, py.x), wb = feather_weight(px.y, py.y);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                na[ch] = __fadd_rn(na[ch], __fmul_rn(wa, va[ch]));
                nb[ch] = __fadd_rn(nb[ch], __fmul_rn(wb, vb[ch]));
            }
            da = __fadd_rn(da, wa);
            db = __fadd_rn(db, wb);
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        fa[ch] = da > 0.f ? __fdiv_rn(na[ch], da) : 0.f;
        fb[ch] = db > 0.f ? __fdiv_rn(nb[ch], db) : 0.f;
    }
}

// render_average_kernel<VIEWS, U8> with the FEATHER fuse: the same rows per wave, the same sinks
template <typename FUSE, int VIEWS, bool U8, typename Views>
__global__ __launch_bounds__(256) void render_average_kernel(Views rv, const float* __restrict__ source,
                                                             const float* __restrict__ T, const float* __restrict__ fp,
                                                             float* __restrict__ out, int h, int w, int hc, int wc,
                                                             int mode, long long img_fs, long long out_fs,
                                                             long long fp_fs) {
    static_assert(std::is_same<FUSE, FeatherFuse>::value, "the fusion tags: FeatherFuse");
    {
        const long long frame = blockIdx.y;
        source += frame * (VIEWS * SS_NV * 2);
        T += frame * (VIEWS * 2 * SS_NT);
        if (fp) fp += frame * fp_fs;
        out = reinterpret_cast<float*>(reinterpret_cast<char*>(out) + frame * out_fs);
        views_to_frame<VIEWS>(rv, frame, img_fs);
    }
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(out);
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    int tbx, tby;
    const unsigned mask = render_tile<VIEWS>(fp, hc, wc, tbx, tby);
    const int x = tbx * 64 + lx;
    const int ya = tby * 8 + wv, yb = ya + 4;
    if (tbx * 64 >= wc || ya >= hc) return;       // (whole waves only: the lanes past the canvas edge still help build the table)
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
    __shared__ ss_f2 dytab[4][VIEWS][64];
    float fa[3], fb[3];
    feather_rows<VIEWS>(mask, source, T, dytab[wv], lx, gx, gya, gyb, [&](int k, float xn, float yn, float (&v)[3]) {
        if (U8) sample3_u8(reinterpret_cast<const unsigned char*>(rv.img[k]), xn, yn, w, h, mode, v);
        else sample3(rv.img[k], xn, yn, w, h, hw, mode, v);
        if constexpr (std::is_same<Views, GainViews>::value) apply_gains(rv.gains + k * 3, v);
    }, fa, fb);
    if (x >= wc) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (U8) {
            out8[((long long)ya * wc + x) * 3 + ch] = render_to_u8(fa[ch]);
            if (yb < hc) out8[((long long)yb * wc + x) * 3 + ch] = render_to_u8(fb[ch]);
        } else {
            out[ch * ohw + (long long)ya * wc + x] = fa[ch];
            if (yb < hc) out[ch * ohw + (long long)yb * wc + x] = fb[ch];
        }
    }
}

static int render_average_launch(const void* const* imgs, const float* source, const float* T, const float* footprint,
                                 long long footprint_floats, void* out, int frames, long long img_fs, long long out_fs,
                                 int views, int h, int w, int hc, int wc, int mode, void* stream, bool u8,
                                 const float* gains = nullptr, bool with_gains = false) {
    if (with_gains && (!gains || (mode & SS_WARP_EPS_FOLD))) return SS_ERR_ARG;       // (the gain forms have no folded variant)
    if ((mode & SS_FUSE_FEATHER) && (mode & SS_WARP_EPS_FOLD)) return SS_ERR_ARG;     // (nor has FEATHER)
    if (!imgs || !source || !T || !out || frames <= 0 || (views != 2 && views != 3) || h <= 1 || w <= 1 || hc <= 1 ||
        wc <= 1 || ((mode & 0xCF) != SS_WARP_NORMAL && (mode & 0xCF) != SS_WARP_FAST))
        return SS_ERR_ARG;
#ifndef SS_TUNING
    if (mode >> 8) return SS_ERR_ARG;
#endif
    const bool fold = (mode & SS_WARP_EPS_FOLD) != 0, feather = (mode & SS_FUSE_FEATHER) != 0;
    mode &= ~(SS_WARP_EPS_FOLD | SS_FUSE_FEATHER);
    // a footprint row is only meaningful for the (views, canvas) it was built for: the kernel indexes its lattice and tile
    // order with this geometry, so a row of another size is an argument error, not an out-of-bounds read
    const long long fp_fs = ss_render_footprint_floats(views, hc, wc);
    if (footprint && footprint_floats != fp_fs) return SS_ERR_ARG;
    GainViews gv;
    if (!views_make(gv, imgs, views, gains)) return SS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    // grid.y = frame; HIP caps grid.y at 65535: longer clips go in several launches
    for (int f0 = 0; f0 < frames; f0 += 65535) {
        const int nf = frames - f0 < 65535 ? frames - f0 : 65535;
        dim3 g(ss_cdiv(wc, 64) * ss_cdiv(hc, 8), nf, 1);
        GainViews r = gv;
        for (int i = 0; i < views; ++i)
            r.img[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(gv.img[i]) + (long long)f0 * img_fs);
        if (with_gains) r.gains = gains + (long long)f0 * views * 3;
        const float* s_ = source + (long long)f0 * views * SS_NV * 2;
        const float* t_ = T + (long long)f0 * views * 2 * SS_NT;
        const float* p_ = footprint ? footprint + (long long)f0 * fp_fs : nullptr;
        float* o = reinterpret_cast<float*>(static_cast<char*>(out) + (long long)f0 * out_fs);
        with_views(views, u8, [&](auto V, auto U8) {
            auto launch = [&](auto rv, auto FOLD) {
                render_average_kernel<decltype(V)::value, decltype(U8)::value, decltype(FOLD)::value>
                    <<<g, dim3(256), 0, st>>>(rv, s_, t_, p_, o, h, w, hc, wc, mode, img_fs, out_fs, fp_fs);
            };
            auto feather_launch = [&](auto rv) {
                render_average_kernel<FeatherFuse, decltype(V)::value, decltype(U8)::value>
                    <<<g, dim3(256), 0, st>>>(rv, s_, t_, p_, o, h, w, hc, wc, mode, img_fs, out_fs, fp_fs);
            };
            // (fold: opt-in, the reference's + 1e-6 folded into the row table -- not its arithmetic; see device_math.h)
            if (feather && with_gains) feather_launch(r);
            else if (feather) feather_launch(RenderViews(r));
            else if (with_gains) launch(r, std::false_type{});
            else if (fold) launch(RenderViews(r), std::true_type{});
            else launch(RenderViews(r), std::false_type{});
        });
    }
    return ss_launch_status();
}

extern "C" int ss_render_average(const float* const* imgs, const float* source, const float* T, const float* footprint,
                                 long long footprint_floats, float* out, int views, int h, int w, int hc, int wc, int mode,
                                 void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(imgs), source, T, footprint, footprint_floats, out, 1,
                                 0, 0, views, h, w, hc, wc, mode, stream, false);
}

extern "C" int ss_render_average_u8(const unsigned char* const* frames, const float* source, const float* T,
                                    const float* footprint, long long footprint_floats, unsigned char* out, int views, int h,
                                    int w, int hc, int wc, int mode, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(frames), source, T, footprint, footprint_floats, out, 1,
                                 0, 0, views, h, w, hc, wc, mode, stream, true);
}

// The fused render from decoded NV12 frames (sample3_nv12) to the uint8 video frame, packed B, G, R (NV12OUT = false: out8 =
// [hc][wc][3]) or NV12 (NV12OUT = true: out8 = the Y plane, out_uv the interleaved UV plane, out_pitch bytes per row of both; hc and
// wc even).  Per pixel the arithmetic of render_average_kernel<VIEWS, true>: the spline of a pixel does not depend on which wave
// evaluates it, so here wave w owns rows 2 w and 2 w + 1 of the tile -- a lane holds both rows of its column, its horizontal
// neighbour is one lane away, and the chroma pair of a 2 x 2 block (tiles are 64 x 8 and even-aligned: a block never straddles
// two) is formed in registers from the bytes the BGR frame would hold.  A tile no view reaches is black: Y 16, U 128, V 128.
template <int VIEWS, bool NV12OUT>
__global__ __launch_bounds__(256) void render_average_kernel(Nv12Views nv, const float* __restrict__ source,
                                                             const float* __restrict__ T, const float* __restrict__ fp,
                                                             unsigned char* __restrict__ out8, unsigned char* __restrict__ out_uv,
                                                             int out_pitch, int h, int w, int hc, int wc, int mode, long long out_fs,
                                                             long long fp_fs) {
    {
        const long long frame = blockIdx.y;
        source += frame * (VIEWS * SS_NV * 2);
        T += frame * (VIEWS * 2 * SS_NT);
        if (fp) fp += frame * fp_fs;
        out8 += frame * out_fs;
        if (NV12OUT) out_uv += frame * out_fs;
        views_to_frame<VIEWS>(nv, frame);
    }
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int tbx, tby;
    unsigned mask = render_tile<VIEWS>(fp, hc, wc, tbx, tby);
    const int x = tbx * 64 + lx;
    const int ya = tby * 8 + 2 * wv, yb = ya + 1;
    if (tbx * 64 >= wc || ya >= hc) return;       // (whole waves only: the lanes past the canvas edge still help build the table)
    const bool xin = x < wc, rowb = yb < hc;
    unsigned char ba[3] = {0, 0, 0}, bb[3] = {0, 0, 0};       // the video frame's B, G, R bytes at (x, ya) and (x, yb)
    if (mask != 0u) {
        const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
        __shared__ ss_f2 dytab[4][VIEWS][64];
        const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
#pragma unroll
        for (int k = 0; k < VIEWS; ++k)
            if (mask & (1u << k)) tps_rows_table(source + k * SS_NV * 2, gya, gyb, lx, dytab[wv][k]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // same wave reads it back: ordering only, no barrier
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float va[VIEWS][3], vb[VIEWS][3];
#pragma unroll
        for (int k = 0; k < VIEWS; ++k) {
            if (mask & (1u << k)) {
                ss_f2 px, py;
                tps_eval_rows(source + k * SS_NV * 2, T + k * 2 * SS_NT, dytab[wv][k], gx, gya, gyb, px, py);
                sample3_nv12(nv.y[k], nv.uv[k], nv.pitch[k], px.x, py.x, w, h, mode, va[k]);
                sample3_nv12(nv.y[k], nv.uv[k], nv.pitch[k], px.y, py.y, w, h, mode, vb[k]);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { va[k][ch] = 0.f; vb[k][ch] = 0.f; }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            // the chained fusion in the reference's order ((1 (+) 2) (+) 3), zeros in the places of views that do not reach
            float fa = avg_fuse(va[0][ch], va[1][ch]), fb = avg_fuse(vb[0][ch], vb[1][ch]);
            if (VIEWS == 3) { fa = avg_fuse(fa, va[2][ch]); fb = avg_fuse(fb, vb[2][ch]); }
            ba[ch] = render_to_u8(fa);
            bb[ch] = render_to_u8(fb);
        }
    }
    if (!NV12OUT) {
        if (!xin) return;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            out8[((long long)ya * wc + x) * 3 + ch] = ba[ch];
            if (rowb) out8[((long long)yb * wc + x) * 3 + ch] = bb[ch];
        }
    } else {
        // (hc and wc are even: rowb holds, and the two lanes of a block are inside the canvas together)
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int own = (int)ba[ch] + (int)bb[ch];
            s[ch] = own + __shfl_xor(own, 1, 64);
        }
        if (!xin) return;
        out8[(long long)ya * out_pitch + x] = bgr_to_y(ba[0], ba[1], ba[2]);
        out8[(long long)yb * out_pitch + x] = bgr_to_y(bb[0], bb[1], bb[2]);
        if (!(lx & 1))
            *reinterpret_cast<unsigned short*>(out_uv + (long long)(ya >> 1) * out_pitch + x) = bgr4_to_uv(s[0], s[1], s[2]);
    }
}

// render_average_kernel<VIEWS, NV12OUT> with the FEATHER fuse: the same rows per wave (2 w, 2 w + 1), the same sinks
template <typename FUSE, int VIEWS, bool NV12OUT>
__global__ __launch_bounds__(256) void render_average_kernel(Nv12Views nv, const float* __restrict__ source,
                                                             const float* __restrict__ T, const float* __restrict__ fp,
                                                             unsigned char* __restrict__ out8, unsigned char* __restrict__ out_uv,
                                                             int out_pitch, int h, int w, int hc, int wc, int mode, long long out_fs,
                                                             long long fp_fs) {
    static_assert(std::is_same<FUSE, FeatherFuse>::value, "the fusion tags: FeatherFuse");
    {
        const long long frame = blockIdx.y;
        source += frame * (VIEWS * SS_NV * 2);
        T += frame * (VIEWS * 2 * SS_NT);
        if (fp) fp += frame * fp_fs;
        out8 += frame * out_fs;
        if (NV12OUT) out_uv += frame * out_fs;
        views_to_frame<VIEWS>(nv, frame);
    }
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int tbx, tby;
    const unsigned mask = render_tile<VIEWS>(fp, hc, wc, tbx, tby);
    const int x = tbx * 64 + lx;
    const int ya = tby * 8 + 2 * wv, yb = ya + 1;
    if (tbx * 64 >= wc || ya >= hc) return;       // (whole waves only: the lanes past the canvas edge still help build the table)
    const bool xin = x < wc, rowb = yb < hc;
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
    __shared__ ss_f2 dytab[4][VIEWS][64];
    float fa[3], fb[3];
    feather_rows<VIEWS>(mask, source, T, dytab[wv], lx, gx, gya, gyb, [&](int k, float xn, float yn, float (&v)[3]) {
        sample3_nv12(nv.y[k], nv.uv[k], nv.pitch[k], xn, yn, w, h, mode, v);
    }, fa, fb);
    unsigned char ba[3], bb[3];       // the video frame's B, G, R bytes at (x, ya) and (x, yb)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { ba[ch] = render_to_u8(fa[ch]); bb[ch] = render_to_u8(fb[ch]); }
    if (!NV12OUT) {
        if (!xin) return;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            out8[((long long)ya * wc + x) * 3 + ch] = ba[ch];
            if (rowb) out8[((long long)yb * wc + x) * 3 + ch] = bb[ch];
        }
    } else {
        // (hc and wc are even: rowb holds, and the two lanes of a block are inside the canvas together)
        int s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int own = (int)ba[ch] + (int)bb[ch];
            s[ch] = own + __shfl_xor(own, 1, 64);
        }
        if (!xin) return;
        out8[(long long)ya * out_pitch + x] = bgr_to_y(ba[0], ba[1], ba[2]);
        out8[(long long)yb * out_pitch + x] = bgr_to_y(bb[0], bb[1], bb[2]);
        if (!(lx & 1))
            *reinterpret_cast<unsigned short*>(out_uv + (long long)(ya >> 1) * out_pitch + x) = bgr4_to_uv(s[0], s[1], s[2]);
    }
}

// NV12 views of an entry point -> the kernels' descriptor; false: a surface the NV12 routes refuse (nv12.h)
static bool nv12_views_make(Nv12Views& nv, const unsigned char* const* y, const unsigned char* const* uv, const int* pitch,
                            const long long* frame_stride, int views, int h, int w) {
    if (!y || !uv || !pitch || h < 2 || w < 2 || (h & 1) || (w & 1)) return false;
    for (int i = 0; i < 3; ++i) {
        nv.y[i] = nullptr; nv.uv[i] = nullptr; nv.pitch[i] = 0; nv.fs[i] = 0;
        if (i >= views) continue;
        if (!y[i] || !uv[i] || (pitch[i] & 1) || pitch[i] < w || (reinterpret_cast<unsigned long long>(uv[i]) & 1ull)) return false;
        if (frame_stride && (frame_stride[i] < 0 || (frame_stride[i] & 1))) return false;
        nv.y[i] = y[i]; nv.uv[i] = uv[i]; nv.pitch[i] = pitch[i]; nv.fs[i] = frame_stride ? frame_stride[i] : 0;
    }
    return true;
}

// ss_render_average_u8 with NV12 views (y / uv / pitch: host arrays of `views` entries); out_format 0: out = uint8 [hc][wc][3]
// (out_uv, out_pitch unused), 1: out = the Y plane, out_uv the UV plane, out_pitch bytes per row of both
extern "C" int ss_render_average_nv12(const unsigned char* const* y, const unsigned char* const* uv, const int* pitch,
                                      const float* source, const float* T, const float* footprint, long long footprint_floats,
                                      unsigned char* out, unsigned char* out_uv, int out_pitch, int out_format, int views, int h,
                                      int w, int hc, int wc, int mode, void* stream) {
    if (!source || !T || !out || (views != 2 && views != 3) || hc <= 1 || wc <= 1 || ((mode & ~SS_FUSE_FEATHER) != SS_WARP_NORMAL && (mode & ~SS_FUSE_FEATHER) != SS_WARP_FAST) || (out_format != 0 && out_format != 1))
        return SS_ERR_ARG;
    const bool feather = (mode & SS_FUSE_FEATHER) != 0;
    mode &= ~SS_FUSE_FEATHER;
    Nv12Views nv;
    if (!nv12_views_make(nv, y, uv, pitch, nullptr, views, h, w)) return SS_ERR_ARG;
    if (out_format == 1 && (!out_uv || (hc & 1) || (wc & 1) || (out_pitch & 1) || out_pitch < wc ||
                            (reinterpret_cast<unsigned long long>(out_uv) & 1ull)))
        return SS_ERR_ARG;
    const long long fp_fs = ss_render_footprint_floats(views, hc, wc);
    if (footprint && footprint_floats != fp_fs) return SS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(ss_cdiv(wc, 64) * ss_cdiv(hc, 8), 1, 1);
    with_views(views, out_format == 1, [&](auto V, auto NV12OUT) {
        if (feather)
            render_average_kernel<FeatherFuse, decltype(V)::value, decltype(NV12OUT)::value>
                <<<g, dim3(256), 0, st>>>(nv, source, T, footprint, out, out_uv, out_pitch, h, w, hc, wc, mode, 0ll, fp_fs);
        else
            render_average_kernel<decltype(V)::value, decltype(NV12OUT)::value>
                <<<g, dim3(256), 0, st>>>(nv, source, T, footprint, out, out_uv, out_pitch, h, w, hc, wc, mode, 0ll, fp_fs);
    });
    return ss_launch_status();
}

// whole clip, one launch: view k's frame f at views[k] + f * 3 h w floats (planar fp32 [n,3,h,w]), canvas f at
// out + f * 3 hc wc floats, source [n,V,63,2], T [n,V,2,66], footprint [n][ss_render_footprint_floats] or NULL
extern "C" int ss_render_average_clip(const float* const* views_base, const float* source, const float* T,
                                      const float* footprint, long long footprint_floats, float* out, int frames, int views,
                                      int h, int w, int hc, int wc, int mode, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(views_base), source, T, footprint, footprint_floats,
                                 out, frames, 12ll * h * w, 12ll * hc * wc, views, h, w, hc, wc, mode, stream, false);
}

// the same from decoded uint8 frames [n,h,w,3] per view to uint8 video frames [n,hc,wc,3]
extern "C" int ss_render_average_clip_u8(const unsigned char* const* views_base, const float* source, const float* T,
                                         const float* footprint, long long footprint_floats, unsigned char* out, int frames,
                                         int views, int h, int w, int hc, int wc, int mode, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(views_base), source, T, footprint, footprint_floats,
                                 out, frames, 3ll * h * w, 3ll * hc * wc, views, h, w, hc, wc, mode, stream, true);
}

// the four AVERAGE entries with exposure gains [frames][views][3] on the device (frames = 1 for the single-frame forms)
extern "C" int ss_render_average_gains(const float* const* imgs, const float* source, const float* T, const float* footprint,
                                       long long footprint_floats, float* out, int views, int h, int w, int hc, int wc, int mode,
                                       const float* gains, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(imgs), source, T, footprint, footprint_floats, out, 1,
                                 0, 0, views, h, w, hc, wc, mode, stream, false, gains, true);
}
extern "C" int ss_render_average_u8_gains(const unsigned char* const* frames, const float* source, const float* T,
                                          const float* footprint, long long footprint_floats, unsigned char* out, int views, int h,
                                          int w, int hc, int wc, int mode, const float* gains, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(frames), source, T, footprint, footprint_floats, out, 1,
                                 0, 0, views, h, w, hc, wc, mode, stream, true, gains, true);
}
extern "C" int ss_render_average_clip_gains(const float* const* views_base, const float* source, const float* T,
                                            const float* footprint, long long footprint_floats, float* out, int frames, int views,
                                            int h, int w, int hc, int wc, int mode, const float* gains, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(views_base), source, T, footprint, footprint_floats,
                                 out, frames, 12ll * h * w, 12ll * hc * wc, views, h, w, hc, wc, mode, stream, false, gains, true);
}
extern "C" int ss_render_average_clip_u8_gains(const unsigned char* const* views_base, const float* source, const float* T,
                                               const float* footprint, long long footprint_floats, unsigned char* out, int frames,
                                               int views, int h, int w, int hc, int wc, int mode, const float* gains, void* stream) {
    return render_average_launch(reinterpret_cast<const void* const*>(views_base), source, T, footprint, footprint_floats,
                                 out, frames, 3ll * h * w, 3ll * hc * wc, views, h, w, hc, wc, mode, stream, true, gains, true);
}

// ------------------------------------------------------------------------------------------------
// Exposure compensation: per-view, per-channel gains of a stream (Brown-Lowe gain compensation, the arithmetic of OpenCV's
// GainCompensator, per channel), estimated on the footprint lattice -- both views' exactly evaluated sampling coordinates at canvas
// pixels (32 j, 8 i) are a sample set of the overlap that the push has computed anyway.  Third walker of the footprint, an overload
// of render_lattice_kernel.  One workgroup per frame:
//   usable node of pair (a, b): on the canvas (8 i <= hc - 1, 32 j <= wc - 1), both stored coordinates inside [-1, 1]^2, all three
//     channels of both samples (sample3 / sample3_u8: the render's own sampler) inside [lo, hi];
//   statistics per pair and channel: n, Sa = sum I_a, Sb = sum I_b in fp64 -- per-thread sums over the nodes tid, tid + 256, ..,
//     an xor butterfly inside each wave, the four waves added in order: no atomics, one fixed order whatever the timing;
//   targets (thread 0, fp64, closed form): pairs with n < min_nodes are dropped; with m_a = Sa / n, m_b = Sb / n and
//     lambda = sigma_n^2 / sigma_g^2 the minimiser of sum n [(g_a m_a - g_b m_b)^2 / sigma_n^2 + ((1 - g_a)^2 + (1 - g_b)^2) / sigma_g^2]
//     is g = 1 + d with  A d = r,  A_aa = sum n (m_a^2 + lambda),  A_ab = -n m_a m_b,  r_a = sum n m_a (m_b - m_a)   (solved for
//     the deviation from 1: equal means give r = 0 and gains of exactly 1); a view in no kept pair keeps 1; clamped, rounded to fp32;
//   smoothing (fp32, one rounding per operation, the frames of a call in stream order): the first frame with a kept pair sets
//     s = target, later ones s += alpha (target - s), a frame without one leaves s alone; gains[f] = s after frame f.
// frames = 1: one launch.  frames > 1: the workgroups leave their targets in gains[f] (gains[f][0] = -1: no kept pair -- gain_min > 0)
// and a second launch of one thread (phase 1) walks them.
//   state [12]: gains [3][3] (rows of views beyond `views` unused), word 9 = started flag (int), 10, 11 unused
//   diag [frames][SS_EXPOSURE_DIAG] doubles (optional): [p * 9 + c * 3 + (n, Sa, Sb)] for pair p = (0,1), (0,2), (1,2) | [27 + v * 3 + c]
//     targets | [36] 1 when a pair was kept
#define SS_EXPOSURE_DIAG 40
struct ExposureArgs {
    const void* img[3];
    const float* fp;
    long long img_fs, fp_fs;          // bytes between the frames of a view, floats between footprint rows
    int frames, h, w, hc, wc, mode, phase, min_nodes;
    float lo, hi, alpha, gain_min, gain_max;
    double lambda;
    float* state;
    float* gains;
    double* diag;
};

// s <- the smoothed gains after a frame whose targets are t (kept: did the frame keep a pair?)
template <int VIEWS>
__device__ __forceinline__ void exposure_smooth(float (&s)[VIEWS * 3], int& started, const float (&t)[VIEWS * 3], bool kept, float alpha) {
    if (!kept) return;
#pragma unroll
    for (int q = 0; q < VIEWS * 3; ++q) s[q] = started ? __fadd_rn(s[q], __fmul_rn(alpha, __fsub_rn(t[q], s[q]))) : t[q];
    started = 1;
}

template <int VIEWS, bool U8>
__global__ __launch_bounds__(256) void render_lattice_kernel(ExposureArgs a) {
    constexpr int P = VIEWS * (VIEWS - 1) / 2;
    int* const state_i = reinterpret_cast<int*>(a.state);
    if (a.phase == 1) {                              // the smoothing walk over the targets the workgroups left
        if (blockIdx.x != 0 || threadIdx.x != 0) return;
        float s[VIEWS * 3], t[VIEWS * 3];
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) s[q] = a.state[q];
        int started = state_i[9];
        for (int f = 0; f < a.frames; ++f) {
            float* g = a.gains + (long long)f * (VIEWS * 3);
#pragma unroll
            for (int q = 0; q < VIEWS * 3; ++q) t[q] = g[q];
            exposure_smooth<VIEWS>(s, started, t, t[0] >= 0.f, a.alpha);
#pragma unroll
            for (int q = 0; q < VIEWS * 3; ++q) g[q] = s[q];
        }
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) a.state[q] = s[q];
        state_i[9] = started;
        return;
    }
    const long long frame = blockIdx.x;
    const int ny = (a.hc + 7) / 8 + 1, nx = 2 * ((a.wc + 63) / 64) + 1, nn = ny * nx;
    const float* lat = a.fp + frame * a.fp_fs;
    const long long hw = (long long)a.h * a.w;
    int cnt[P];
    double sa[P][3], sb[P][3];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        cnt[p] = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { sa[p][c] = 0.0; sb[p][c] = 0.0; }
    }
    for (int idx = threadIdx.x; idx < nn; idx += 256) {
        const int i = idx / nx, j = idx - i * nx;
        if (8 * i > a.hc - 1 || 32 * j > a.wc - 1) continue;       // the lattice's last row / column may lie beyond the canvas
        float v[VIEWS][3];
        bool ok[VIEWS];
#pragma unroll
        for (int k = 0; k < VIEWS; ++k) {
            const float xn = lat[((long long)k * nn + idx) * 2], yn = lat[((long long)k * nn + idx) * 2 + 1];
            ok[k] = fabsf(xn) <= 1.f && fabsf(yn) <= 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[k][c] = 0.f;
            if (ok[k]) {
                const char* img = static_cast<const char*>(a.img[k]) + frame * a.img_fs;
                if (U8) sample3_u8(reinterpret_cast<const unsigned char*>(img), xn, yn, a.w, a.h, a.mode, v[k]);
                else sample3(reinterpret_cast<const float*>(img), xn, yn, a.w, a.h, hw, a.mode, v[k]);
#pragma unroll
                for (int c = 0; c < 3; ++c) ok[k] = ok[k] && v[k][c] >= a.lo && v[k][c] <= a.hi;
            }
        }
        int p = 0;
#pragma unroll
        for (int ka = 0; ka < VIEWS; ++ka)
#pragma unroll
            for (int kb = ka + 1; kb < VIEWS; ++kb, ++p)
                if (ok[ka] && ok[kb]) {
                    cnt[p] += 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) { sa[p][c] += (double)v[ka][c]; sb[p][c] += (double)v[kb][c]; }
                }
    }
    // fixed tree: xor butterfly inside the wave (every lane ends with the same bits), then the four waves in order
    __shared__ double red[4][P][6];
    __shared__ int redn[4][P];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt[p] += __shfl_xor(cnt[p], o, 64);
#pragma unroll
            for (int c = 0; c < 3; ++c) { sa[p][c] += __shfl_xor(sa[p][c], o, 64); sb[p][c] += __shfl_xor(sb[p][c], o, 64); }
        }
        if (lane == 0) {
            redn[wv][p] = cnt[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) { red[wv][p][c] = sa[p][c]; red[wv][p][3 + c] = sb[p][c]; }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        cnt[p] = redn[0][p] + redn[1][p] + redn[2][p] + redn[3][p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sa[p][c] = ((red[0][p][c] + red[1][p][c]) + red[2][p][c]) + red[3][p][c];
            sb[p][c] = ((red[0][p][3 + c] + red[1][p][3 + c]) + red[2][p][3 + c]) + red[3][p][3 + c];
        }
    }
    bool keep[P], any = false, inv[VIEWS];
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) inv[k] = false;
    {
        int p = 0;
#pragma unroll
        for (int ka = 0; ka < VIEWS; ++ka)
#pragma unroll
            for (int kb = ka + 1; kb < VIEWS; ++kb, ++p) {
                keep[p] = cnt[p] >= a.min_nodes;
                if (keep[p]) { any = true; inv[ka] = true; inv[kb] = true; }
            }
    }
    float t[VIEWS * 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double A[VIEWS][VIEWS], r[VIEWS], d[VIEWS];
#pragma unroll
        for (int k = 0; k < VIEWS; ++k) {
            r[k] = 0.0;
#pragma unroll
            for (int l = 0; l < VIEWS; ++l) A[k][l] = 0.0;
        }
        int p = 0;
#pragma unroll
        for (int ka = 0; ka < VIEWS; ++ka)
#pragma unroll
            for (int kb = ka + 1; kb < VIEWS; ++kb, ++p)
                if (keep[p]) {
                    const double n = (double)cnt[p], ma = sa[p][c] / n, mb = sb[p][c] / n;
                    A[ka][ka] += n * (ma * ma + a.lambda);
                    A[kb][kb] += n * (mb * mb + a.lambda);
                    A[ka][kb] -= n * ma * mb;
                    A[kb][ka] -= n * ma * mb;
                    r[ka] += n * ma * (mb - ma);
                    r[kb] += n * mb * (ma - mb);
                }
#pragma unroll
        for (int k = 0; k < VIEWS; ++k)
            if (!inv[k]) A[k][k] = 1.0;                // a view in no kept pair: its row reads d = 0
        if constexpr (VIEWS == 2) {
            const double det = A[0][0] * A[1][1] - A[0][1] * A[1][0];
            d[0] = (r[0] * A[1][1] - A[0][1] * r[1]) / det;
            d[1] = (A[0][0] * r[1] - r[0] * A[1][0]) / det;
        } else {
            constexpr int X = VIEWS - 1;               // (= 2 here; keeps the V = 2 instantiation's indices inside its arrays)
            const double c00 = A[1][1] * A[X][X] - A[1][X] * A[X][1], c01 = A[1][0] * A[X][X] - A[1][X] * A[X][0],
                         c02 = A[1][0] * A[X][1] - A[1][1] * A[X][0];
            const double det = A[0][0] * c00 - A[0][1] * c01 + A[0][X] * c02;
            d[0] = (r[0] * c00 - A[0][1] * (r[1] * A[X][X] - A[1][X] * r[X]) + A[0][X] * (r[1] * A[X][1] - A[1][1] * r[X])) / det;
            d[1] = (A[0][0] * (r[1] * A[X][X] - A[1][X] * r[X]) - r[0] * c01 + A[0][X] * (A[1][0] * r[X] - r[1] * A[X][0])) / det;
            d[X] = (A[0][0] * (A[1][1] * r[X] - r[1] * A[X][1]) - A[0][1] * (A[1][0] * r[X] - r[1] * A[X][0]) + r[0] * c02) / det;
        }
#pragma unroll
        for (int k = 0; k < VIEWS; ++k) {
            double g = inv[k] ? 1.0 + d[k] : 1.0;
            g = fmin(fmax(g, (double)a.gain_min), (double)a.gain_max);
            t[k * 3 + c] = (float)g;
        }
    }
    if (a.diag) {
        double* dg = a.diag + frame * SS_EXPOSURE_DIAG;
#pragma unroll
        for (int q = 0; q < SS_EXPOSURE_DIAG; ++q) dg[q] = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dg[p * 9 + c * 3] = (double)cnt[p];
                dg[p * 9 + c * 3 + 1] = sa[p][c];
                dg[p * 9 + c * 3 + 2] = sb[p][c];
            }
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) dg[27 + q] = (double)t[q];
        dg[36] = any ? 1.0 : 0.0;
    }
    float* g = a.gains + frame * (VIEWS * 3);
    if (a.frames == 1) {                             // the whole update in this launch
        float s[VIEWS * 3];
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) s[q] = a.state[q];
        int started = state_i[9];
        exposure_smooth<VIEWS>(s, started, t, any, a.alpha);
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) { g[q] = s[q]; a.state[q] = s[q]; }
        state_i[9] = started;
    } else {
#pragma unroll
        for (int q = 0; q < VIEWS * 3; ++q) g[q] = t[q];
        if (!any) g[0] = -1.f;
    }
}

extern "C" int ss_exposure_update(const void* const* views_base, int u8, long long img_fs, const float* footprint,
                                  long long footprint_floats, long long fp_fs, int frames, int views, int h, int w, int hc, int wc,
                                  int mode, float alpha, float sigma_n, float sigma_g, float lo, float hi, int min_nodes,
                                  float gain_min, float gain_max, float* state, float* gains, double* diag, void* stream) {
    if (!views_base || !footprint || !state || !gains || frames <= 0 || frames > 65535 || (views != 2 && views != 3) || h <= 1 ||
        w <= 1 || hc <= 1 || wc <= 1 || (mode != SS_WARP_NORMAL && mode != SS_WARP_FAST) || (u8 != 0 && u8 != 1) || img_fs < 0)
        return SS_ERR_ARG;
    if (footprint_floats != ss_render_footprint_floats(views, hc, wc) || (frames > 1 && fp_fs < footprint_floats)) return SS_ERR_ARG;
    if (!(lo <= hi) || !(alpha > 0.f && alpha <= 1.f) || !(gain_min > 0.f) || !(gain_min <= gain_max) || !(gain_max < INFINITY) ||
        !(sigma_n > 0.f) || !(sigma_g > 0.f) || min_nodes < 1)
        return SS_ERR_ARG;
    ExposureArgs a;
    for (int i = 0; i < 3; ++i) a.img[i] = i < views ? views_base[i] : nullptr;
    for (int i = 0; i < views; ++i)
        if (!a.img[i]) return SS_ERR_ARG;
    a.fp = footprint; a.img_fs = img_fs; a.fp_fs = fp_fs;
    a.frames = frames; a.h = h; a.w = w; a.hc = hc; a.wc = wc; a.mode = mode; a.phase = 0; a.min_nodes = min_nodes;
    a.lo = lo; a.hi = hi; a.alpha = alpha; a.gain_min = gain_min; a.gain_max = gain_max;
    a.lambda = ((double)sigma_n * (double)sigma_n) / ((double)sigma_g * (double)sigma_g);
    a.state = state; a.gains = gains; a.diag = diag;
    hipStream_t st = (hipStream_t)stream;
    for (int phase = 0; phase < (frames > 1 ? 2 : 1); ++phase) {
        a.phase = phase;
        const dim3 g(phase ? 1 : frames), b(phase ? 64 : 256);
        with_views(views, u8 != 0, [&](auto V, auto U8) { render_lattice_kernel<decltype(V)::value, decltype(U8)::value><<<g, b, 0, st>>>(a); });
    }
    return ss_launch_status();
}

// ------------------------------------------------------------------------------------------------
// LINEAR fusion (linear_blender, test_online_tra.py:34-58).  Whole-canvas statistics (mask centroids,
// projection range of the overlap) are accumulated with device atomics into a 16-word scalar block at
// the head of the workspace; no host round trip.
//   ws: [0..15] scalars | X [hc*wc] | tmp [hc*wc]
//   scalars (as 64-bit words): 0 cnt1, 1 sumr1, 2 sumc1, 3 cnt2, 4 sumr2, 5 sumc2; floats at [12] pmin-key, [13] pmax-key
__device__ __forceinline__ unsigned f2key(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void lb_init_kernel(unsigned long long* s) {
    if (threadIdx.x < 6) s[threadIdx.x] = 0ull;
    unsigned* u = reinterpret_cast<unsigned*>(s);
    if (threadIdx.x == 0) { u[12] = 0xffffffffu; u[13] = 0u; }
}

// 2-D indexing (block = 64 columns x 4 rows, grid-stride over row groups): no per-pixel integer division
__global__ __launch_bounds__(256) void lb_centroid_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                          unsigned long long* s, int hc, int wc) {
    __shared__ unsigned long long red[6];
    if (threadIdx.x < 6) red[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned c1 = 0, r1 = 0, k1 = 0, c2 = 0, r2 = 0, k2 = 0;      // per-thread partials fit 32 bits (<= hc/ (4 gridDim.y) rows)
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (c < wc) {
        for (int r = blockIdx.y * 4 + (threadIdx.x >> 6); r < hc; r += gridDim.y * 4) {
            long long i = (long long)r * wc + c;
            if (m1[i] != 0.f) { k1 += 1; r1 += r; c1 += c; }
            if (m2[i] != 0.f) { k2 += 1; r2 += r; c2 += c; }
        }
    }
    unsigned v[6] = {k1, r1, c1, k2, r2, c2};       // a wave's sums still fit 32 bits (<= 64 lanes x ~24 rows x 1882)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        unsigned t = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&red[k], (unsigned long long)t);
    }
    __syncthreads();
    if (threadIdx.x < 6) atomicAdd(&s[threadIdx.x], red[threadIdx.x]);
}

struct LbCenters {
    float c1r, c1c, v0, v1;
};
__device__ __forceinline__ LbCenters lb_centers(const unsigned long long* s) {
    LbCenters L;
    L.c1r = (float)((double)s[1] / (double)s[0]);
    L.c1c = (float)((double)s[2] / (double)s[0]);
    float c2r = (float)((double)s[4] / (double)s[3]);
    float c2c = (float)((double)s[5] / (double)s[3]);
    L.v0 = __fsub_rn(c2r, L.c1r);
    L.v1 = __fsub_rn(c2c, L.c1c);
    return L;
}
__device__ __forceinline__ float lb_proj(const LbCenters& L, int r, int c) {
    return __fadd_rn(__fmul_rn(__fsub_rn((float)r, L.c1r), L.v0), __fmul_rn(__fsub_rn((float)c, L.c1c), L.v1));
}
__device__ __forceinline__ bool lb_overlap(float a, float b) { return rintf(__fmul_rn(a, b)) != 0.f; }

__global__ __launch_bounds__(256) void lb_range_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                                       unsigned long long* s, int hc, int wc) {
    // the centres cost four fp64 divisions: once per workgroup, not per thread (that was 55 us per frame)
    __shared__ LbCenters Ls;
    __shared__ float smn[4], smx[4];
    if (threadIdx.x == 0) Ls = lb_centers(s);
    __syncthreads();
    const LbCenters L = Ls;
    float mn = INFINITY, mx = -INFINITY;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    if (c < wc) {
        for (int r = blockIdx.y * 4 + (threadIdx.x >> 6); r < hc; r += gridDim.y * 4) {
            long long i = (long long)r * wc + c;
            if (lb_overlap(m1[i], m2[i])) {
                float p = lb_proj(L, r, c);
                mn = fminf(mn, p);
                mx = fmaxf(mx, p);
            }
        }
    }
    mn = ss_wave_min(mn);
    mx = ss_wave_max(mx);
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
        unsigned* u = reinterpret_cast<unsigned*>(s);
        if (mn != INFINITY) atomicMin(&u[12], f2key(mn));
        if (mx != -INFINITY) atomicMax(&u[13], f2key(mx));
    }
}

// X = ref_only + (1 - ovl_mask) * m1
__global__ void lb_premask_kernel(const float* __restrict__ m1, const float* __restrict__ m2,
                                  const unsigned long long* s, float* __restrict__ X, int hc, int wc) {
    __shared__ LbCenters Ls;
    if (threadIdx.x == 0) Ls = lb_centers(s);
    __syncthreads();
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= wc || r >= hc) return;
    const long long i = (long long)r * wc + c;
    const unsigned* u = reinterpret_cast<const unsigned*>(s);
    float a = m1[i], b = m2[i];
    float ovl = rintf(__fmul_rn(a, b));
    float ref_only = __fsub_rn(a, ovl);
    float om = 0.f;
    if (ovl != 0.f) {
        const LbCenters L = Ls;
        float pmin = key2f(u[12]), pmax = key2f(u[13]);
        om = __fsub_rn(lb_proj(L, r, c), pmin) / __fadd_rn(__fsub_rn(pmax, pmin), 1e-3f);
    }
    X[i] = __fadd_rn(ref_only, __fmul_rn(__fsub_rn(1.f, om), a));
}

struct Gauss21 {
    float k[21];
};

__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// separable 21-tap Gaussian, reflect border (torchvision GaussianBlur((21,21), 20))
__global__ void lb_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int hc, int wc, int vertical,
                               Gauss21 g) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= wc || r >= hc) return;
    const long long i = (long long)r * wc + c;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        int rr = vertical ? reflect_idx(r + k - 10, hc) : r;
        int cc = vertical ? c : reflect_idx(c + k - 10, wc);
        acc = fmaf(g.k[k], in[(long long)rr * wc + cc], acc);
    }
    out[i] = acc;
}

__global__ void lb_final_kernel(const float* __restrict__ ref, const float* __restrict__ tgt,
                                const float* __restrict__ m1, const float* __restrict__ m2,
                                const float* __restrict__ blur, float* __restrict__ out, float* __restrict__ mask1_out,
                                int hc, int wc) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    const long long n = (long long)hc * wc;
    if (c >= wc || r >= hc) return;
    const long long i = (long long)r * wc + c;
    float a = m1[i], b = m2[i];
    float ovl = rintf(__fmul_rn(a, b));
    float ref_only = __fsub_rn(a, ovl);
    float mk = fminf(fmaxf(__fadd_rn(__fmul_rn(blur[i], a), ref_only), 0.f), 1.f);
    if (mask1_out) mask1_out[i] = mk;
    if (out) {
        float mk2 = __fmul_rn(__fsub_rn(1.f, mk), b);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            out[ch * n + i] = __fadd_rn(__fmul_rn(ref[ch * n + i], mk), __fmul_rn(tgt[ch * n + i], mk2));
    }
}

extern "C" long long ss_linear_blend_workspace_floats(int hc, int wc) { return 32 + 2ll * hc * wc; }

extern "C" int ss_linear_blend(const float* ref, const float* tgt, const float* ref_m, const float* tgt_m, float* out,
                               float* mask1_out, int hc, int wc, float* ws, void* stream) {
    if (!ref_m || !tgt_m || !ws || (!out && !mask1_out) || (out && (!ref || !tgt)) || hc < 11 || wc < 11)
        return SS_ERR_ARG;
    if (reinterpret_cast<unsigned long long>(ws) & 7ull) return SS_ERR_ARG;      // the scalar block is 64-bit words (as the clip entry)
    // 1-D kernel exp(-0.5 (t/sigma)^2) on linspace(-10,10,21), normalised, fp32 like torchvision
    Gauss21 g;
    {
        float s = 0.f;
        for (int i = 0; i < 21; ++i) {
            float t = (float)(i - 10) / 20.0f;
            g.k[i] = expf(-0.5f * (t * t));
            s += g.k[i];
        }
        for (int i = 0; i < 21; ++i) g.k[i] /= s;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sc = reinterpret_cast<unsigned long long*>(ws);
    float* X = ws + 32;
    float* tmp = X + (long long)hc * wc;
    hipLaunchKernelGGL(lb_init_kernel, dim3(1), dim3(64), 0, st, sc);
    // few, long-running workgroups for the two reductions: every workgroup ends in atomics on the same scalars
    dim3 rg(ss_cdiv(wc, 64), ss_cdiv(hc, 16) < 8 ? ss_cdiv(hc, 16) : 8);
    hipLaunchKernelGGL(lb_centroid_kernel, rg, dim3(256), 0, st, ref_m, tgt_m, sc, hc, wc);
    hipLaunchKernelGGL(lb_range_kernel, rg, dim3(256), 0, st, ref_m, tgt_m, sc, hc, wc);
    const dim3 pg(ss_cdiv(wc, 64), ss_cdiv(hc, 4));
    hipLaunchKernelGGL(lb_premask_kernel, pg, dim3(256), 0, st, ref_m, tgt_m, (const unsigned long long*)sc, X, hc, wc);
    hipLaunchKernelGGL(lb_blur_kernel, pg, dim3(256), 0, st, (const float*)X, tmp, hc, wc, 0, g);
    hipLaunchKernelGGL(lb_blur_kernel, pg, dim3(256), 0, st, (const float*)tmp, X, hc, wc, 1, g);
    hipLaunchKernelGGL(lb_final_kernel, pg, dim3(256), 0, st, ref, tgt, ref_m, tgt_m, (const float*)X, out,
                       mask1_out, hc, wc);
    return ss_launch_status();
}

// ------------------------------------------------------------------------------------------------
// LINEAR fusion of a whole clip (round 4): the per-frame chain above -- one warp launch + seven blender launches per
// frame, 256 launches per 32-frame clip -- as THREE launches per clip (four with three views: a second blend pass), bit-identical to it:
//   A  lb_clip_warp_kernel    every view of every frame warped once (colour planes + ones-mask plane, the layout of
//                             ss_tps_warp_views), all views of a tile in ONE workgroup so that the blender's whole-canvas
//                             statistics fall out of the masks while they are still in registers: per wave and pass the six
//                             centroid sums (ballot + popcount on the scalar unit: count, sum of rows, sum of columns of the
//                             non-zero mask pixels) and, per row, the first and last overlap column of the tile;
//   R  lb_clip_reduce_kernel  per (frame, pass): the wave partials -> mask centroids -> projection range of the overlap.
//                             lb_proj is weakly monotone along a row (fp32 rounding preserves order), so its extremes over
//                             the overlap are attained at the first / last overlap column of some (row, tile) segment:
//                             the range needs those candidates only, not another pass over the masks;
//   C  lb_clip_blend_kernel   per 64 x 64 canvas tile: X = ref_only + (1 - ovl_mask) m1 on the tile + 10-pixel reflect halo
//                             -> LDS, horizontal 21-tap pass -> LDS, vertical pass, mask1, blend, store (fp32 planes or the
//                             uint8 video frame).  X and the horizontally blurred plane never exist in memory.
// Three views chain ((1 (+) 2) (+) 3) like test_online_tra_threeview.py:489-502: pass 2 takes the union mask
// m1 + m2 - m1 m2 (recomputed on the fly from the two planes) and the fused planes of pass 1.
//   ws: W [n][V][4][hc][wc] | F [n][3][hc][wc] (V = 3 only) | scalars [n][P][16] u64 | partials [n][tiles][4 waves][P][8] u32
//   scalars as in ss_linear_blend: words 0..5 = cnt1, sumr1, sumc1, cnt2, sumr2, sumc2; u32[12] / u32[13] = range keys
#define LBC_PW 8          // partial words per (wave, pass): k1, r1, c1, k2, r2, c2, candidates of row a, row b

extern "C" long long ss_linear_clip_workspace_floats(int frames, int views, int hc, int wc) {
    if (frames <= 0 || (views != 2 && views != 3) || hc <= 1 || wc <= 1) return 0;
    const long long ohw = (long long)hc * wc, p = views - 1;
    const long long tiles = (long long)ss_cdiv(wc, 64) * ss_cdiv(hc, 8);
    // (+ 1: the 64-bit scalars block starts on an even float behind W / F whatever the parity of frames * hc * wc)
    return (long long)frames * (views * 4 * ohw + (views == 3 ? 3 * ohw : 0) + p * 32 + tiles * 4 * p * LBC_PW) + 1;
}

// sum of the lane indices whose bit is set (scalar unit: six popcounts)
__device__ __forceinline__ unsigned lane_index_sum(unsigned long long m) {
    return (unsigned)__popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (unsigned)__popcll(m & 0xCCCCCCCCCCCCCCCCull) +
           4u * (unsigned)__popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (unsigned)__popcll(m & 0xFF00FF00FF00FF00ull) +
           16u * (unsigned)__popcll(m & 0xFFFF0000FFFF0000ull) + 32u * (unsigned)__popcll(m & 0xFFFFFFFF00000000ull);
}

// one 64 x 8 tile of ONE frame: rv / source / T / W are that frame's, tile_part its partials of this tile [4 waves][P][LBC_PW]
// (Views = Nv12Views: decoded NV12 frames, sampled as sample3_nv12 does; U8 is not looked at then;
//  Views = GainViews: rv.gains = this frame's exposure gains [VIEWS][3], applied to the sampled colours)
template <int VIEWS, bool U8, typename Views>
__device__ __forceinline__ void lb_warp_tile(Views rv, const float* __restrict__ source,
                                             const float* __restrict__ T, float* __restrict__ W,
                                             unsigned* __restrict__ tile_part, unsigned tile, int h, int w, int hc, int wc, int mode) {
    constexpr int P = VIEWS - 1;
    const long long hw = (long long)h * w, ohw = (long long)hc * wc;
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nbx = (wc + 63) / 64;
    const int tby = tile / nbx, tbx = tile - tby * nbx;      // (unsigned division: tile is a block index)
    unsigned* part = tile_part + wv * (P * LBC_PW);
    const int x = tbx * 64 + lx;
    const int ya = tby * 8 + wv, yb = ya + 4;
    if (ya >= hc) {                                  // a wave below the canvas: its partials are read all the same
        if (lx < P * LBC_PW) part[lx] = (lx & 7) >= 6 ? 0xFFFFFFFFu : 0u;
        return;
    }
    const bool xin = x < wc;
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    __shared__ ss_f2 dytab[4][VIEWS][64];
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) tps_rows_table(source + k * SS_NV * 2, gya, gyb, lx, dytab[wv][k]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // same wave reads it back: ordering only, no barrier
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float ma[VIEWS], mb[VIEWS];                      // the ones-mask plane of every view at the lane's pixel of row a / row b
    const bool rowb = yb < hc;
#pragma unroll
    for (int k = 0; k < VIEWS; ++k) {
        ss_f2 px, py;
        tps_eval_rows(source + k * SS_NV * 2, T + k * 2 * SS_NT, dytab[wv][k], gx, gya, gyb, px, py);
        float va[3], vb[3];
        if constexpr (std::is_same<Views, Nv12Views>::value) {
            sample3_nv12(rv.y[k], rv.uv[k], rv.pitch[k], px.x, py.x, w, h, mode, va);
            sample3_nv12(rv.y[k], rv.uv[k], rv.pitch[k], px.y, py.y, w, h, mode, vb);
        } else if (U8) {
            const unsigned char* img8 = reinterpret_cast<const unsigned char*>(rv.img[k]);
            sample3_u8(img8, px.x, py.x, w, h, mode, va);
            sample3_u8(img8, px.y, py.y, w, h, mode, vb);
        } else {
            sample3(rv.img[k], px.x, py.x, w, h, hw, mode, va);
            sample3(rv.img[k], px.y, py.y, w, h, hw, mode, vb);
        }
        if constexpr (std::is_same<Views, GainViews>::value) {       // exposure gains: the colour planes only, the masks are untouched
            apply_gains(rv.gains + k * 3, va);
            apply_gains(rv.gains + k * 3, vb);
        }
        if (mode == SS_WARP_NORMAL) {
            const SsTaps ta = taps_normal(px.x, py.x, w, h), tb = taps_normal(px.y, py.y, w, h);
            ma[k] = blend4(ta, 1.f, 1.f, 1.f, 1.f);
            mb[k] = blend4(tb, 1.f, 1.f, 1.f, 1.f);
        } else {
            ma[k] = fast_mask(px.x, py.x, w, h);
            mb[k] = fast_mask(px.y, py.y, w, h);
        }
        if (xin) {
            float* o = W + (long long)k * 4 * ohw + (long long)ya * wc + x;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch * ohw] = va[ch];
            o[3 * ohw] = ma[k];
            if (rowb) {
                o += 4ll * wc;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) o[ch * ohw] = vb[ch];
                o[3 * ohw] = mb[k];
            }
        }
    }
    // the blender's statistics of this wave's two rows, per pass: ref mask = m0 (pass 1) / m0 + m1 - m0 m1 (pass 2)
    float ra = ma[0], rb = mb[0];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float ta = ma[p + 1], tb = mb[p + 1];
        const unsigned long long r_a = __ballot(xin && ra != 0.f), r_b = __ballot(xin && rowb && rb != 0.f);
        const unsigned long long t_a = __ballot(xin && ta != 0.f), t_b = __ballot(xin && rowb && tb != 0.f);
        const unsigned long long o_a = __ballot(xin && lb_overlap(ra, ta)), o_b = __ballot(xin && rowb && lb_overlap(rb, tb));
        const unsigned k1a = (unsigned)__popcll(r_a), k1b = (unsigned)__popcll(r_b);
        const unsigned k2a = (unsigned)__popcll(t_a), k2b = (unsigned)__popcll(t_b);
        if (lx == 0) {
            unsigned* q = part + p * LBC_PW;
            q[0] = k1a + k1b;
            q[1] = k1a * (unsigned)ya + k1b * (unsigned)yb;
            q[2] = (k1a + k1b) * (unsigned)(tbx * 64) + lane_index_sum(r_a) + lane_index_sum(r_b);
            q[3] = k2a + k2b;
            q[4] = k2a * (unsigned)ya + k2b * (unsigned)yb;
            q[5] = (k2a + k2b) * (unsigned)(tbx * 64) + lane_index_sum(t_a) + lane_index_sum(t_b);
            // first | last << 16 overlap column of the row inside this tile (0xFFFFFFFF: none)
            q[6] = o_a ? (unsigned)(tbx * 64 + __ffsll((long long)o_a) - 1) | ((unsigned)(tbx * 64 + 63 - __clzll((long long)o_a)) << 16)
                       : 0xFFFFFFFFu;
            q[7] = o_b ? (unsigned)(tbx * 64 + __ffsll((long long)o_b) - 1) | ((unsigned)(tbx * 64 + 63 - __clzll((long long)o_b)) << 16)
                       : 0xFFFFFFFFu;
        }
        if (p + 1 < P) {                              // mask12 = m1 + m2 - m1 m2 (threeview:498; ss_mask_union)
            ra = __fsub_rn(__fadd_rn(ra, ta), __fmul_rn(ra, ta));
            rb = __fsub_rn(__fadd_rn(rb, tb), __fmul_rn(rb, tb));
        }
    }
}

template <int VIEWS, bool U8, typename Views>
__global__ __launch_bounds__(256) void lb_clip_warp_kernel(Views rv, const float* __restrict__ source,
                                                           const float* __restrict__ T, float* __restrict__ W,
                                                           unsigned* __restrict__ partials, int h, int w, int hc, int wc,
                                                           int mode, long long img_fs) {
    constexpr int P = VIEWS - 1;
    const long long frame = blockIdx.y;
    views_to_frame<VIEWS>(rv, frame, img_fs);
    lb_warp_tile<VIEWS, U8>(rv, source + frame * (VIEWS * SS_NV * 2), T + frame * (VIEWS * 2 * SS_NT),
                            W + frame * (VIEWS * 4) * ((long long)hc * wc),
                            partials + ((frame * gridDim.x + blockIdx.x) * 4) * (P * LBC_PW), blockIdx.x, h, w, hc, wc, mode);
}

// one (frame, pass): the frame's nw wave partials of this pass (q0, `stride` words apart) -> its scalars block s
__device__ __forceinline__ void lb_reduce_pass(const unsigned* __restrict__ q0, long long stride, int nw, int nbx,
                                               unsigned long long* __restrict__ s) {
    __shared__ unsigned long long red[6];
    __shared__ LbCenters Ls;
    __shared__ float smn[4], smx[4];
    if (threadIdx.x < 6) red[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long acc[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int i = threadIdx.x; i < nw; i += 256) {
        const unsigned* q = q0 + i * stride;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += q[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        unsigned long long t = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&red[k], t);
    }
    __syncthreads();
    if (threadIdx.x < 6) s[threadIdx.x] = red[threadIdx.x];
    if (threadIdx.x == 0) Ls = lb_centers(red);
    __syncthreads();
    const LbCenters L = Ls;
    float mn = INFINITY, mx = -INFINITY;
    // wave partial i belongs to tile i / 4, wave i % 4: rows (tile / nbx) * 8 + wave and + 4 -- the row is recomputed from
    // the partial's position, the columns come packed
    for (int i = threadIdx.x; i < nw; i += 256) {
        const unsigned* q = q0 + i * stride;
        const int tile = i >> 2, wv = i & 3;
        const int ya = (tile / nbx) * 8 + wv;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const unsigned e = q[6 + rr];
            if (e != 0xFFFFFFFFu) {
                const int r = ya + 4 * rr;
                const float p0 = lb_proj(L, r, (int)(e & 0xFFFFu)), p1 = lb_proj(L, r, (int)(e >> 16));
                mn = fminf(mn, fminf(p0, p1));
                mx = fmaxf(mx, fmaxf(p0, p1));
            }
        }
    }
    mn = ss_wave_min(mn);
    mx = ss_wave_max(mx);
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
        mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
        unsigned* u = reinterpret_cast<unsigned*>(s);
        u[12] = mn != INFINITY ? f2key(mn) : 0xffffffffu;         // (the values lb_init_kernel + atomicMin / atomicMax leave)
        u[13] = mx != -INFINITY ? f2key(mx) : 0u;
    }
}

// one workgroup per (frame, pass): wave partials -> scalars block
__global__ __launch_bounds__(256) void lb_clip_reduce_kernel(const unsigned* __restrict__ partials, unsigned long long* __restrict__ scalars,
                                                             int tiles, int nbx, int passes) {
    const int frame = blockIdx.x / passes, p = blockIdx.x - frame * passes;
    lb_reduce_pass(partials + ((long long)frame * tiles * 4) * (passes * LBC_PW) + p * LBC_PW, (long long)passes * LBC_PW,
                   tiles * 4, nbx, scalars + (long long)blockIdx.x * 16);
}

struct LbClipArgs {
    const float *ref, *tgt, *m1a, *m1b, *m2;          // m1b != nullptr: ref mask = m1a + m1b - m1a m1b
    long long ref_fs, tgt_fs, m_fs;                   // frame strides in floats (all masks share W's)
    float* out;                                       // fp32 [n][3][hc][wc] or uint8 [n][hc][wc][3]
    float* mask1_out;                                 // nullable, this pass's plane of [n][P][hc][wc]
    long long mask1_fs;
    const unsigned long long* scalars;                // this pass's block of frame 0
    long long sc_fs;                                  // u64 words between frames
};

#define LBC_T 64
#define LBC_E (LBC_T + 20)
template <bool UNION, bool U8OUT>
__global__ __launch_bounds__(256) void lb_clip_blend_kernel(LbClipArgs a, int hc, int wc, Gauss21 g) {
    __shared__ float XL[LBC_E * LBC_E];              // X on the tile + halo, reflected coordinates resolved
    __shared__ float TL[LBC_E * LBC_T];              // horizontally blurred rows of the tile + vertical halo
    __shared__ LbCenters Ls;
    __shared__ float prange[2];
    const long long frame = blockIdx.z;
    const long long ohw = (long long)hc * wc;
    const float* m1a = a.m1a + frame * a.m_fs;
    const float* m1b = UNION ? a.m1b + frame * a.m_fs : nullptr;
    const float* m2 = a.m2 + frame * a.m_fs;
    const unsigned long long* s = a.scalars + frame * a.sc_fs;
    if (threadIdx.x == 0) {
        Ls = lb_centers(s);
        const unsigned* u = reinterpret_cast<const unsigned*>(s);
        prange[0] = key2f(u[12]);
        prange[1] = key2f(u[13]);
    }
    __syncthreads();
    const LbCenters L = Ls;
    const float pmin = prange[0], pmax = prange[1];
    const int r0 = blockIdx.y * LBC_T, c0 = blockIdx.x * LBC_T;
    for (int idx = threadIdx.x; idx < LBC_E * LBC_E; idx += 256) {
        const int row = idx / LBC_E, col = idx - row * LBC_E;
        // rows / columns of a partial last tile beyond the canvas feed no stored pixel: any in-range index will do
        const int r = min(max(reflect_idx(r0 - 10 + row, hc), 0), hc - 1), c = min(max(reflect_idx(c0 - 10 + col, wc), 0), wc - 1);
        const long long i = (long long)r * wc + c;
        float ma = m1a[i];
        if (UNION) { const float mb = m1b[i]; ma = __fsub_rn(__fadd_rn(ma, mb), __fmul_rn(ma, mb)); }
        const float b = m2[i];
        const float ovl = rintf(__fmul_rn(ma, b));
        const float ref_only = __fsub_rn(ma, ovl);
        float om = 0.f;
        if (ovl != 0.f) om = __fsub_rn(lb_proj(L, r, c), pmin) / __fadd_rn(__fsub_rn(pmax, pmin), 1e-3f);
        XL[idx] = __fadd_rn(ref_only, __fmul_rn(__fsub_rn(1.f, om), ma));
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int row = wv; row < LBC_E; row += 4) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 21; ++k) acc = fmaf(g.k[k], XL[row * LBC_E + lx + k], acc);
        TL[row * LBC_T + lx] = acc;
    }
    __syncthreads();
    const int c = c0 + lx;
    if (c >= wc) return;
    const float* ref = a.ref + frame * a.ref_fs;
    const float* tgt = a.tgt + frame * a.tgt_fs;
    float* mk_out = a.mask1_out ? a.mask1_out + frame * a.mask1_fs : nullptr;
    for (int row = wv; row < LBC_T; row += 4) {
        const int r = r0 + row;
        if (r >= hc) break;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 21; ++k) acc = fmaf(g.k[k], TL[(row + k) * LBC_T + lx], acc);
        const long long i = (long long)r * wc + c;
        float ma = m1a[i];
        if (UNION) { const float mb = m1b[i]; ma = __fsub_rn(__fadd_rn(ma, mb), __fmul_rn(ma, mb)); }
        const float b = m2[i];
        const float ovl = rintf(__fmul_rn(ma, b));
        const float ref_only = __fsub_rn(ma, ovl);
        const float mk = fminf(fmaxf(__fadd_rn(__fmul_rn(acc, ma), ref_only), 0.f), 1.f);
        if (mk_out) mk_out[i] = mk;
        const float mk2 = __fmul_rn(__fsub_rn(1.f, mk), b);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = __fadd_rn(__fmul_rn(ref[ch * ohw + i], mk), __fmul_rn(tgt[ch * ohw + i], mk2));
            if (U8OUT) reinterpret_cast<unsigned char*>(a.out)[(frame * ohw + i) * 3 + ch] = render_to_u8(v);
            else a.out[(frame * 3 + ch) * ohw + i] = v;
        }
    }
}

// The same blend as a ROLLING pass down the canvas (round 4, second version; the 64 x 64-tile kernel above stays as the
// reference form and for the tests).  One WAVE owns a strip of 64 columns x `rs` rows of one frame and walks it row by row:
//   row p:  X(p, c0-10 .. c0+73) from the masks (reflected columns; lanes 0..19 take a second column) -> 84 floats of LDS
//           -> the lane's horizontal 21-tap sum hb(p) -> pushed into a 21-deep ring held in REGISTERS;
//   once the ring is full, output row p-10 = the vertical 21-tap sum over the ring, mask1, blend, store.
// No workgroup barrier, no tile halo in the row direction (only the 20 warm-up rows per strip), X / hb never in memory; the
// loads of the next row are issued before the current row's arithmetic.  Same fmaf chains as the tile kernel and as
// lb_blur_kernel: bit-identical output.  The tile kernel moved 2.2 GB per 32-frame clip at 2.7 TB/s (three phases between
// barriers, 50 KB of LDS -> 3 workgroups per CU: its loads came in bursts); this one streams.
// one blend pass of ONE frame: its planes, this pass's scalars block, its output ([3][hc][wc] fp32 or [hc][wc][3] uint8)
struct LbPass {
    const float *ref, *tgt, *m1a, *m1b, *m2;          // m1b (UNION): ref mask = m1a + m1b - m1a m1b
    float* mk_out;                                    // nullable [hc][wc]
    const unsigned long long* s;
    void* out;
};

// strip (bx, by) of 64 columns x rs rows of that frame, one wave
template <bool UNION, bool U8OUT>
__device__ __forceinline__ void lb_blend_strip(const LbPass& a, int hc, int wc, int rs, int bx, int by, const Gauss21& g) {
    __shared__ float XL[96];
    __shared__ LbCenters Ls;
    __shared__ float prange[2];
    const long long ohw = (long long)hc * wc;
    const float* __restrict__ m1a = a.m1a;
    const float* __restrict__ m1b = UNION ? a.m1b : nullptr;
    const float* __restrict__ m2 = a.m2;
    const float* __restrict__ ref = a.ref;
    const float* __restrict__ tgt = a.tgt;
    float* mk_out = a.mk_out;
    const unsigned long long* s = a.s;
    const int lane = threadIdx.x;
    if (lane == 0) {
        Ls = lb_centers(s);
        const unsigned* u = reinterpret_cast<const unsigned*>(s);
        prange[0] = key2f(u[12]);
        prange[1] = key2f(u[13]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const LbCenters L = Ls;
    const float pmin = prange[0], pden = __fadd_rn(__fsub_rn(prange[1], prange[0]), 1e-3f);
    const int c0 = bx * 64, s0 = by * rs, s1 = min(s0 + rs, hc);
    const int c = c0 + lane;
    const bool cin = c < wc, second = lane < 20;
    const int ca = min(max(reflect_idx(c0 - 10 + lane, wc), 0), wc - 1);
    const int cb = min(max(reflect_idx(c0 + 54 + lane, wc), 0), wc - 1);
    const int cc = min(c, wc - 1);
    auto xval = [&](float ma, float mb, float b, int r, int col) -> float {
        if (UNION) ma = __fsub_rn(__fadd_rn(ma, mb), __fmul_rn(ma, mb));
        const float ovl = rintf(__fmul_rn(ma, b));
        const float ref_only = __fsub_rn(ma, ovl);
        float om = 0.f;
        if (ovl != 0.f) om = __fsub_rn(lb_proj(L, r, col), pmin) / pden;
        return __fadd_rn(ref_only, __fmul_rn(__fsub_rn(1.f, om), ma));
    };
    float ring[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) ring[k] = 0.f;
    // masks of the row whose X comes next (columns ca / cb), requested one row ahead
    float nxa1, nxa1b = 0.f, nxa2, nxb1 = 0.f, nxb1b = 0.f, nxb2 = 0.f;
    auto row_of = [&](int p) { return min(max(reflect_idx(p, hc), 0), hc - 1); };
    {
        const long long i = (long long)row_of(s0 - 10) * wc;
        nxa1 = m1a[i + ca]; nxa2 = m2[i + ca];
        if (UNION) nxa1b = m1b[i + ca];
        if (second) { nxb1 = m1a[i + cb]; nxb2 = m2[i + cb]; if (UNION) nxb1b = m1b[i + cb]; }
    }
    for (int p = s0 - 10; p < s1 + 10; ++p) {
        const int r = row_of(p);
        const float xa1 = nxa1, xa1b = nxa1b, xa2 = nxa2, xb1 = nxb1, xb1b = nxb1b, xb2 = nxb2;
        if (p + 1 < s1 + 10) {                               // next row's masks
            const long long i = (long long)row_of(p + 1) * wc;
            nxa1 = m1a[i + ca]; nxa2 = m2[i + ca];
            if (UNION) nxa1b = m1b[i + ca];
            if (second) { nxb1 = m1a[i + cb]; nxb2 = m2[i + cb]; if (UNION) nxb1b = m1b[i + cb]; }
        }
        // this output row's planes (row p - 10), requested before the blur arithmetic
        const int ro = p - 10;
        const bool emit = ro >= s0;
        float oma = 0.f, omb = 0.f, ob = 0.f, orf[3] = {0.f, 0.f, 0.f}, otg[3] = {0.f, 0.f, 0.f};
        const long long io = (long long)max(ro, 0) * wc + cc;
        if (emit) {
            oma = m1a[io]; ob = m2[io];
            if (UNION) omb = m1b[io];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { orf[ch] = ref[ch * ohw + io]; otg[ch] = tgt[ch * ohw + io]; }
        }
        XL[lane] = xval(xa1, xa1b, xa2, r, ca);
        if (second) XL[64 + lane] = xval(xb1, xb1b, xb2, r, cb);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float hb = 0.f;
#pragma unroll
        for (int k = 0; k < 21; ++k) hb = fmaf(g.k[k], XL[lane + k], hb);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the row buffer is rewritten next iteration
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 20; ++k) ring[k] = ring[k + 1];
        ring[20] = hb;
        if (emit && cin) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 21; ++k) acc = fmaf(g.k[k], ring[k], acc);
            float ma = oma;
            if (UNION) ma = __fsub_rn(__fadd_rn(ma, omb), __fmul_rn(ma, omb));
            const float ovl = rintf(__fmul_rn(ma, ob));
            const float ref_only = __fsub_rn(ma, ovl);
            const float mk = fminf(fmaxf(__fadd_rn(__fmul_rn(acc, ma), ref_only), 0.f), 1.f);
            if (mk_out) mk_out[io] = mk;
            const float mk2 = __fmul_rn(__fsub_rn(1.f, mk), ob);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float v = __fadd_rn(__fmul_rn(orf[ch], mk), __fmul_rn(otg[ch], mk2));
                if (U8OUT) static_cast<unsigned char*>(a.out)[io * 3 + ch] = render_to_u8(v);
                else static_cast<float*>(a.out)[ch * ohw + io] = v;
            }
        }
    }
}

template <bool UNION, bool U8OUT>
__global__ __launch_bounds__(64) void lb_clip_blend_rows_kernel(LbClipArgs a, int hc, int wc, int rs, Gauss21 g) {
    const long long frame = blockIdx.z;
    const long long ohw = (long long)hc * wc;
    LbPass p;
    p.ref = a.ref + frame * a.ref_fs;
    p.tgt = a.tgt + frame * a.tgt_fs;
    p.m1a = a.m1a + frame * a.m_fs;
    p.m1b = UNION ? a.m1b + frame * a.m_fs : nullptr;
    p.m2 = a.m2 + frame * a.m_fs;
    p.mk_out = a.mask1_out ? a.mask1_out + frame * a.mask1_fs : nullptr;
    p.s = a.scalars + frame * a.sc_fs;
    p.out = U8OUT ? static_cast<void*>(reinterpret_cast<unsigned char*>(a.out) + frame * ohw * 3)
                  : static_cast<void*>(a.out + frame * 3 * ohw);
    lb_blend_strip<UNION, U8OUT>(p, hc, wc, rs, blockIdx.x, blockIdx.y, g);
}

static Gauss21 lb_gauss() {
    // 1-D kernel exp(-0.5 (t/sigma)^2) on linspace(-10,10,21), normalised, fp32 like torchvision (as ss_linear_blend)
    Gauss21 g;
    float s = 0.f;
    for (int i = 0; i < 21; ++i) {
        float t = (float)(i - 10) / 20.0f;
        g.k[i] = expf(-0.5f * (t * t));
        s += g.k[i];
    }
    for (int i = 0; i < 21; ++i) g.k[i] /= s;
    return g;
}

// rows per strip of the rolling blend kernel: 0 = default (96), > 0 = that many, < 0 = the 64 x 64-tile kernel instead
// (ss_linear_clip_set_rows: an A/B and test knob; both forms give the same bits)
static int g_lb_rows = 0;
extern "C" int ss_linear_clip_set_rows(int rows) {
    g_lb_rows = rows;
    return SS_OK;
}

static int render_linear_clip_launch(const void* const* views_base, const float* source, const float* T, void* out,
                                     float* mask1_out, int frames, int views, int h, int w, int hc, int wc, int mode,
                                     float* ws, void* stream, bool u8, const float* gains = nullptr, bool with_gains = false) {
    if (with_gains && !gains) return SS_ERR_ARG;
    if (!views_base || !source || !T || !out || !ws || frames <= 0 || frames > 65535 || (views != 2 && views != 3) || h <= 1 ||
        w <= 1 || hc < 11 || wc < 11 || wc > 65535 || hc > 65535 || (mode != SS_WARP_NORMAL && mode != SS_WARP_FAST))
        return SS_ERR_ARG;
    GainViews gv;
    if (!views_make(gv, views_base, views, gains)) return SS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long ohw = (long long)hc * wc;
    const int P = views - 1, nbx = ss_cdiv(wc, 64), tiles = nbx * ss_cdiv(hc, 8);
    float* W = ws;
    float* F = W + (long long)frames * views * 4 * ohw;
    long long sc_off = (long long)frames * views * 4 * ohw + (views == 3 ? (long long)frames * 3 * ohw : 0);
    sc_off += sc_off & 1;                                  // 8-byte alignment of the u64 block by construction (ws is 8-byte aligned)
    if (reinterpret_cast<unsigned long long>(ws) & 7ull) return SS_ERR_ARG;
    unsigned long long* scalars = reinterpret_cast<unsigned long long*>(ws + sc_off);
    unsigned* partials = reinterpret_cast<unsigned*>(scalars + (long long)frames * P * 16);
    const long long img_fs = u8 ? 3ll * h * w : 12ll * h * w;
    const dim3 ga(tiles, frames);
    auto warp = [&](auto rv) {
        with_views(views, u8, [&](auto V, auto U8) {
            lb_clip_warp_kernel<decltype(V)::value, decltype(U8)::value>
                <<<ga, dim3(256), 0, st>>>(rv, source, T, W, partials, h, w, hc, wc, mode, img_fs);
        });
    };
    if (with_gains) warp(gv); else warp(RenderViews(gv));
    hipLaunchKernelGGL(lb_clip_reduce_kernel, dim3(frames * P), dim3(256), 0, st, (const unsigned*)partials, scalars, tiles, nbx, P);
    const Gauss21 g = lb_gauss();
    const dim3 gc(ss_cdiv(wc, LBC_T), ss_cdiv(hc, LBC_T), frames);
    // rolling form: strips of 64 columns x rs rows, one wave each; rs so that a 720p canvas gives ~30 waves per CU
    const int rs = g_lb_rows > 0 ? g_lb_rows : 96;
    const dim3 gr(ss_cdiv(wc, 64), ss_cdiv(hc, rs), frames);
    const bool rolling = g_lb_rows >= 0;
    LbClipArgs a;
    a.m_fs = views * 4 * ohw;
    a.ref = W; a.ref_fs = a.m_fs;
    a.tgt = W + 4 * ohw; a.tgt_fs = a.m_fs;
    a.m1a = W + 3 * ohw; a.m1b = nullptr; a.m2 = W + 7 * ohw;
    a.mask1_out = mask1_out; a.mask1_fs = P * ohw;
    a.scalars = scalars; a.sc_fs = P * 16;
    auto blend = [&](bool second_pass, bool u8out) {      // a's pass: the rolling form, or the 64 x 64-tile one
        with_flags(second_pass, u8out, [&](auto UNION, auto U8OUT) {
            if (rolling) lb_clip_blend_rows_kernel<decltype(UNION)::value, decltype(U8OUT)::value><<<gr, dim3(64), 0, st>>>(a, hc, wc, rs, g);
            else lb_clip_blend_kernel<decltype(UNION)::value, decltype(U8OUT)::value><<<gc, dim3(256), 0, st>>>(a, hc, wc, g);
        });
    };
    if (views == 2) {
        a.out = static_cast<float*>(out);
        blend(false, u8);
    } else {
        a.out = F;
        blend(false, false);
        a.ref = F; a.ref_fs = 3 * ohw;
        a.tgt = W + 8 * ohw;
        a.m1b = W + 7 * ohw; a.m2 = W + 11 * ohw;
        a.mask1_out = mask1_out ? mask1_out + ohw : nullptr;
        a.scalars = scalars + 16;
        a.out = static_cast<float*>(out);
        blend(true, u8);
    }
    return ss_launch_status();
}

// whole clip, LINEAR fusion: view k's frame f at views_base[k] + f * 3 h w floats (planar fp32 [n,3,h,w]) -> out [n,3,hc,wc];
// mask1_out (nullable): the blender's mask1 of every pass [n][V-1][hc][wc]; ws: ss_linear_clip_workspace_floats(...) floats
extern "C" int ss_render_linear_clip(const float* const* views_base, const float* source, const float* T, float* out,
                                     float* mask1_out, int frames, int views, int h, int w, int hc, int wc, int mode,
                                     float* ws, void* stream) {
    return render_linear_clip_launch(reinterpret_cast<const void* const*>(views_base), source, T, out, mask1_out, frames, views,
                                     h, w, hc, wc, mode, ws, stream, false);
}

// the same from decoded uint8 frames [n,h,w,3] per view to uint8 video frames [n,hc,wc,3] (`.astype(np.uint8)` of the blend)
extern "C" int ss_render_linear_clip_u8(const unsigned char* const* views_base, const float* source, const float* T,
                                        unsigned char* out, float* mask1_out, int frames, int views, int h, int w, int hc,
                                        int wc, int mode, float* ws, void* stream) {
    return render_linear_clip_launch(reinterpret_cast<const void* const*>(views_base), source, T, out, mask1_out, frames, views,
                                     h, w, hc, wc, mode, ws, stream, true);
}

// the two clip entries with exposure gains [frames][views][3] on the device
extern "C" int ss_render_linear_clip_gains(const float* const* views_base, const float* source, const float* T, float* out,
                                           float* mask1_out, int frames, int views, int h, int w, int hc, int wc, int mode,
                                           float* ws, const float* gains, void* stream) {
    return render_linear_clip_launch(reinterpret_cast<const void* const*>(views_base), source, T, out, mask1_out, frames, views,
                                     h, w, hc, wc, mode, ws, stream, false, gains, true);
}
extern "C" int ss_render_linear_clip_u8_gains(const unsigned char* const* views_base, const float* source, const float* T,
                                              unsigned char* out, float* mask1_out, int frames, int views, int h, int w, int hc,
                                              int wc, int mode, float* ws, const float* gains, void* stream) {
    return render_linear_clip_launch(reinterpret_cast<const void* const*>(views_base), source, T, out, mask1_out, frames, views,
                                     h, w, hc, wc, mode, ws, stream, true, gains, true);
}

// ------------------------------------------------------------------------------------------------
// LINEAR fusion of up to 32 frames that each have their OWN canvas (the current frames of S live streams, or one streaming push:
// frames = 1): the clip render above with ragged sizes, still three launches (four with three views) whatever `frames` is.  The
// grids are flattened lists -- all frames' 64 x 8 warp tiles, all frames' 64 x rs blend strips -- and a workgroup finds its frame
// in a table of per-frame descriptors passed BY VALUE in the kernel arguments (1.4 KB of the 4 KB segment): the arrays are consumed
// during the call, nothing to copy to the device and nothing whose lifetime a later launch depends on.  The lookup is a binary
// search over <= 33 prefix sums on the scalar unit (blockIdx is uniform).  Per pixel the device functions of the clip kernels.
//   ws: W of frame 0, 1, .. [V][4][hc_i][wc_i] | F of frame 0, 1, .. [3][hc_i][wc_i] (V = 3 only) | scalars [n][P][16] u64 |
//       partials of frame 0, 1, .. [tiles_i][4 waves][P][8] u32          (the clip's layout where the sizes are equal)
#define LBF_MAX 32
struct LbFrameTab {
    int n;
    unsigned tile0[LBF_MAX + 1];                      // prefix sums of the frames' warp tiles (64 x 8)
    unsigned strip0[LBF_MAX + 1];                     // prefix sums of the frames' blend strips (64 x rs)
    unsigned short hc[LBF_MAX], wc[LBF_MAX];
    long long w_off[LBF_MAX], f_off[LBF_MAX];         // the frame's W / F, floats from ws
    long long part_off[LBF_MAX];                      // the frame's partials, words from the partials block
    void* out[LBF_MAX];
};

// the frame whose range of the flattened grid holds block b: pre[f] <= b < pre[f + 1] (uniform: scalar loads of the table)
__device__ __forceinline__ int lb_frame_of(const unsigned* pre, int n, unsigned b) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (b >= pre[m]) lo = m; else hi = m;
    }
    return lo;
}

extern "C" long long ss_linear_frames_workspace_floats(int frames, int views, const int* hc, const int* wc) {
    if (frames <= 0 || frames > LBF_MAX || (views != 2 && views != 3) || !hc || !wc) return 0;
    const long long p = views - 1;
    long long total = 1;                              // (+ 1: as ss_linear_clip_workspace_floats)
    for (int f = 0; f < frames; ++f) {
        if (hc[f] < 11 || wc[f] < 11 || hc[f] > 65535 || wc[f] > 65535) return 0;
        const long long ohw = (long long)hc[f] * wc[f];
        const long long tiles = (long long)ss_cdiv(wc[f], 64) * ss_cdiv(hc[f], 8);
        total += views * 4 * ohw + (views == 3 ? 3 * ohw : 0) + p * 32 + tiles * 4 * p * LBC_PW;
    }
    return total;
}

template <int VIEWS, bool U8, typename Views>
__global__ __launch_bounds__(256) void lb_frames_warp_kernel(Views rv, const float* __restrict__ source,
                                                             const float* __restrict__ T, float* __restrict__ ws,
                                                             unsigned* __restrict__ partials, int h, int w, int mode,
                                                             long long img_fs, LbFrameTab t) {
    constexpr int P = VIEWS - 1;
    const int f = lb_frame_of(t.tile0, t.n, blockIdx.x);
    const unsigned tile = blockIdx.x - t.tile0[f];
    views_to_frame<VIEWS>(rv, f, img_fs);
    lb_warp_tile<VIEWS, U8>(rv, source + (long long)f * (VIEWS * SS_NV * 2), T + (long long)f * (VIEWS * 2 * SS_NT),
                            ws + t.w_off[f], partials + t.part_off[f] + ((long long)tile * 4) * (P * LBC_PW), tile, h, w,
                            (int)t.hc[f], (int)t.wc[f], mode);
}

// the same from decoded NV12 frames (frame f of view k at y[k] / uv[k] + f * fs[k]); an overload of its own: the descriptor carries
// its frame strides, so the kernel has no img_fs argument (with one, its instruction stream changes: LAB_NOTES.md, "Source-only changes")
template <int VIEWS>
__global__ __launch_bounds__(256) void lb_frames_warp_kernel(Nv12Views nv, const float* __restrict__ source,
                                                             const float* __restrict__ T, float* __restrict__ ws,
                                                             unsigned* __restrict__ partials, int h, int w, int mode, LbFrameTab t) {
    constexpr int P = VIEWS - 1;
    const int f = lb_frame_of(t.tile0, t.n, blockIdx.x);
    const unsigned tile = blockIdx.x - t.tile0[f];
    views_to_frame<VIEWS>(nv, f);
    lb_warp_tile<VIEWS, true>(nv, source + (long long)f * (VIEWS * SS_NV * 2), T + (long long)f * (VIEWS * 2 * SS_NT),
                              ws + t.w_off[f], partials + t.part_off[f] + ((long long)tile * 4) * (P * LBC_PW), tile, h, w,
                              (int)t.hc[f], (int)t.wc[f], mode);
}

// one workgroup per (frame, pass)
__global__ __launch_bounds__(256) void lb_frames_reduce_kernel(const unsigned* __restrict__ partials,
                                                               unsigned long long* __restrict__ scalars, int passes, LbFrameTab t) {
    const int f = blockIdx.x / passes, p = blockIdx.x - f * passes;
    const int tiles = (int)(t.tile0[f + 1] - t.tile0[f]);
    lb_reduce_pass(partials + t.part_off[f] + p * LBC_PW, (long long)passes * LBC_PW, tiles * 4, ((int)t.wc[f] + 63) / 64,
                   scalars + (long long)blockIdx.x * 16);
}

// blend pass 1 (UNION = false; into the frame's output, or into F when a second pass follows) / pass 2 (UNION = true) of every frame
template <bool UNION, bool U8OUT>
__global__ __launch_bounds__(64) void lb_frames_blend_rows_kernel(float* __restrict__ ws, const unsigned long long* __restrict__ scalars,
                                                                  int views, int rs, Gauss21 g, LbFrameTab t) {
    const int f = lb_frame_of(t.strip0, t.n, blockIdx.x);
    const int strip = (int)(blockIdx.x - t.strip0[f]);
    const int hc = t.hc[f], wc = t.wc[f];
    const int nbx = (wc + 63) / 64;
    const int by = strip / nbx, bx = strip - by * nbx;
    const long long ohw = (long long)hc * wc;
    float* W = ws + t.w_off[f];
    float* F = ws + t.f_off[f];
    LbPass a;
    a.m1a = W + 3 * ohw;
    a.mk_out = nullptr;
    if (!UNION) {
        a.ref = W; a.tgt = W + 4 * ohw;
        a.m1b = nullptr; a.m2 = W + 7 * ohw;
        a.s = scalars + (long long)f * (views - 1) * 16;
        a.out = views == 2 ? t.out[f] : static_cast<void*>(F);
    } else {
        a.ref = F; a.tgt = W + 8 * ohw;
        a.m1b = W + 7 * ohw; a.m2 = W + 11 * ohw;
        a.s = scalars + ((long long)f * 2 + 1) * 16;
        a.out = t.out[f];
    }
    lb_blend_strip<UNION, U8OUT>(a, hc, wc, rs, bx, by, g);
}

// nv12 != nullptr: the views are decoded NV12 frames (views_base unused), uint8 frames out
static int render_linear_frames_launch(const void* const* views_base, const float* source, const float* T, void* const* out,
                                       int frames, int views, int h, int w, const int* hc, const int* wc, int mode, float* ws,
                                       void* stream, bool u8, const Nv12Views* nv12 = nullptr, const float* gains = nullptr,
                                       bool with_gains = false) {
    if (with_gains && (!gains || nv12)) return SS_ERR_ARG;
    if ((!views_base && !nv12) || !source || !T || !out || !hc || !wc || !ws || frames <= 0 || frames > LBF_MAX || (views != 2 && views != 3) ||
        h <= 1 || w <= 1 || (mode != SS_WARP_NORMAL && mode != SS_WARP_FAST))
        return SS_ERR_ARG;
    if (reinterpret_cast<unsigned long long>(ws) & 7ull) return SS_ERR_ARG;
    GainViews gv = {};
    if (!nv12 && !views_make(gv, views_base, views, gains)) return SS_ERR_ARG;
    const int P = views - 1;
    // rolling blend only (the 64 x 64-tile form of ss_linear_clip_set_rows(r < 0) does not exist here: default strip height)
    const int rs = g_lb_rows > 0 ? g_lb_rows : 96;
    LbFrameTab t = {};
    t.n = frames;
    long long w_total = 0, f_total = 0, part_total = 0;
    for (int f = 0; f < frames; ++f) {
        if (!out[f] || hc[f] < 11 || wc[f] < 11 || hc[f] > 65535 || wc[f] > 65535) return SS_ERR_ARG;
        const long long ohw = (long long)hc[f] * wc[f];
        const long long tiles = (long long)ss_cdiv(wc[f], 64) * ss_cdiv(hc[f], 8);
        const long long strips = (long long)ss_cdiv(wc[f], 64) * ss_cdiv(hc[f], rs);
        t.hc[f] = (unsigned short)hc[f];
        t.wc[f] = (unsigned short)wc[f];
        t.tile0[f + 1] = t.tile0[f] + (unsigned)tiles;
        t.strip0[f + 1] = t.strip0[f] + (unsigned)strips;
        t.w_off[f] = w_total;
        t.f_off[f] = f_total;                         // (relative to the F block; made absolute below)
        t.part_off[f] = part_total;
        t.out[f] = out[f];
        w_total += views * 4 * ohw;
        f_total += views == 3 ? 3 * ohw : 0;
        part_total += tiles * 4 * P * LBC_PW;
    }
    for (int f = 0; f < frames; ++f) t.f_off[f] += w_total;
    long long sc_off = w_total + f_total;
    sc_off += sc_off & 1;                             // 8-byte alignment of the u64 block, as in the clip entry
    unsigned long long* scalars = reinterpret_cast<unsigned long long*>(ws + sc_off);
    unsigned* partials = reinterpret_cast<unsigned*>(scalars + (long long)frames * P * 16);
    hipStream_t st = (hipStream_t)stream;
    const long long img_fs = u8 ? 3ll * h * w : 12ll * h * w;
    const dim3 ga(t.tile0[frames]), gr(t.strip0[frames]);
    auto warp = [&](auto rv) {
        with_views(views, u8, [&](auto V, auto U8) {
            if constexpr (std::is_same<decltype(rv), Nv12Views>::value)
                lb_frames_warp_kernel<decltype(V)::value><<<ga, dim3(256), 0, st>>>(rv, source, T, ws, partials, h, w, mode, t);
            else
                lb_frames_warp_kernel<decltype(V)::value, decltype(U8)::value>
                    <<<ga, dim3(256), 0, st>>>(rv, source, T, ws, partials, h, w, mode, img_fs, t);
        });
    };
    if (nv12) warp(*nv12); else if (with_gains) warp(gv); else warp(RenderViews(gv));
    hipLaunchKernelGGL(lb_frames_reduce_kernel, dim3(frames * P), dim3(256), 0, st, (const unsigned*)partials, scalars, P, t);
    const Gauss21 g = lb_gauss();
    const unsigned long long* sc = scalars;
    auto blend = [&](bool second_pass, bool u8out) {
        with_flags(second_pass, u8out, [&](auto UNION, auto U8OUT) {
            lb_frames_blend_rows_kernel<decltype(UNION)::value, decltype(U8OUT)::value><<<gr, dim3(64), 0, st>>>(ws, sc, views, rs, g, t);
        });
    };
    if (views == 2) {
        blend(false, u8);
    } else {
        blend(false, false);
        blend(true, u8);
    }
    return ss_launch_status();
}

// `frames` frames with their own canvases, LINEAR fusion: view k's frame f at views_base[k] + f * 3 h w floats (planar fp32
// [n,3,h,w]) -> out[f] = [3][hc[f]][wc[f]]; hc / wc / out: host arrays of `frames` entries, consumed during the call;
// ws: ss_linear_frames_workspace_floats(...) floats
extern "C" int ss_render_linear_frames(const float* const* views_base, const float* source, const float* T, float* const* out,
                                       int frames, int views, int h, int w, const int* hc, const int* wc, int mode, float* ws,
                                       void* stream) {
    return render_linear_frames_launch(reinterpret_cast<const void* const*>(views_base), source, T,
                                       reinterpret_cast<void* const*>(out), frames, views, h, w, hc, wc, mode, ws, stream, false);
}

// the same from decoded uint8 frames [n,h,w,3] per view to uint8 video frames out[f] = [hc[f]][wc[f]][3]
extern "C" int ss_render_linear_frames_u8(const unsigned char* const* views_base, const float* source, const float* T,
                                          unsigned char* const* out, int frames, int views, int h, int w, const int* hc,
                                          const int* wc, int mode, float* ws, void* stream) {
    return render_linear_frames_launch(reinterpret_cast<const void* const*>(views_base), source, T,
                                       reinterpret_cast<void* const*>(out), frames, views, h, w, hc, wc, mode, ws, stream, true);
}

// the two frames entries with exposure gains [frames][views][3] on the device
extern "C" int ss_render_linear_frames_gains(const float* const* views_base, const float* source, const float* T, float* const* out,
                                             int frames, int views, int h, int w, const int* hc, const int* wc, int mode, float* ws,
                                             const float* gains, void* stream) {
    return render_linear_frames_launch(reinterpret_cast<const void* const*>(views_base), source, T,
                                       reinterpret_cast<void* const*>(out), frames, views, h, w, hc, wc, mode, ws, stream, false,
                                       nullptr, gains, true);
}
extern "C" int ss_render_linear_frames_u8_gains(const unsigned char* const* views_base, const float* source, const float* T,
                                                unsigned char* const* out, int frames, int views, int h, int w, const int* hc,
                                                const int* wc, int mode, float* ws, const float* gains, void* stream) {
    return render_linear_frames_launch(reinterpret_cast<const void* const*>(views_base), source, T,
                                       reinterpret_cast<void* const*>(out), frames, views, h, w, hc, wc, mode, ws, stream, true,
                                       nullptr, gains, true);
}

// the same from decoded NV12 frames per view (y / uv / pitch / frame_stride: host arrays of `views` entries, frame f of view k at
// y[k] / uv[k] + f * frame_stride[k]) to uint8 video frames out[f] = [hc[f]][wc[f]][3]; NV12 frames out: ss_bgr_to_nv12 behind it
extern "C" int ss_render_linear_frames_nv12(const unsigned char* const* y, const unsigned char* const* uv, const int* pitch,
                                            const long long* frame_stride, const float* source, const float* T,
                                            unsigned char* const* out, int frames, int views, int h, int w, const int* hc,
                                            const int* wc, int mode, float* ws, void* stream) {
    if ((views != 2 && views != 3) || !frame_stride) return SS_ERR_ARG;
    Nv12Views nv;
    if (!nv12_views_make(nv, y, uv, pitch, frame_stride, views, h, w)) return SS_ERR_ARG;
    return render_linear_frames_launch(nullptr, source, T, reinterpret_cast<void* const*>(out), frames, views, h, w, hc, wc, mode,
                                       ws, stream, true, &nv);
}
