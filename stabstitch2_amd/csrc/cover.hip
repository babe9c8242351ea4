// Coverage bitmaps and the largest fully covered rectangle (libstabstitch_cover.so, include/stabstitch_cover.h).
//
// Coverage: per (frame, view) the mask value that tps_warp_kernel (render.hip) and mw_warp_kernel (mbwarp.hip) write to their mask
// plane, compared with min_mask, OR-ed over the views and packed 64 columns to a word.  Same geometry as those kernels: 256 threads,
// a tile of 64 columns x 8 rows, wave w owns rows w and w + 4, the spline through tps_rows_table / tps_eval_rows (device_math.h) --
// the sampling coordinates and the mask equal theirs bit for bit (-ffp-contract=off: the FAST weights below are written with plain
// operators, as render.hip's are).  A wave is 64 columns of one row, so its ballot IS the bitmap word; lane 0 stores it.
//
// Rectangle: column heights (one thread per column walks the rows), then per row the classic candidates -- column i limits the
// rectangle of height heights[i] between its nearest strictly smaller neighbours -- found through a min-tree over the row in LDS
// (O(log wc) steps per column, whatever the row holds), then one workgroup reduces the rows' candidates.  Integers throughout.
#include "common.h"
#include "device_math.h"

#include "../../include/stabstitch_cover.h"

namespace {

typedef unsigned long long cv_word;

// ---- restated from render.hip (which is not edited; it shares no header with this library): fast_mask, term by term;
// warp_rows_coords
__device__ __forceinline__ float cv_fast_mask(float xn, float yn, int w, int h) {
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
__device__ __forceinline__ void cv_rows_coords(const float* __restrict__ src, const float* __restrict__ T, ss_f2* tab, int lane, int x,
                                               int ya, int yb, int hc, int wc, ss_f2& xn, ss_f2& yn) {
    const float gx = linspace_at(-1.f, 1.f, wc, min(x, wc - 1));
    const float gya = linspace_at(-1.f, 1.f, hc, ya), gyb = linspace_at(-1.f, 1.f, hc, min(yb, hc - 1));
    tps_rows_table(src, gya, gyb, lane, tab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the same wave reads it back: ordering only
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    tps_eval_rows(src, T, tab, gx, gya, gyb, xn, yn);
}
__device__ __forceinline__ float cv_mask(float xn, float yn, int w, int h, int mode) {
    return mode == SSC_WARP_NORMAL ? blend4(taps_normal(xn, yn, w, h), 1.f, 1.f, 1.f, 1.f) : cv_fast_mask(xn, yn, w, h);
}

// ACC: grid.z = 1, the wave loops over the frames and ANDs them into the caller's words (it leaves once both are zero); else
// grid.z = frames, one bitmap each.  No atomics: a word belongs to one wave.  A (frame, view) is evaluated only while it can still
// change its word.
template <bool ACC>
__global__ __launch_bounds__(256) void cv_coverage_kernel(const float* __restrict__ source, const float* __restrict__ T,
                                                          cv_word* __restrict__ bitmap, int frames, int views, int h, int w, int hc,
                                                          int wc, int mode, float min_mask) {
    __shared__ ss_f2 dytab[4][64];
    const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lx;
    const int ya = blockIdx.y * 8 + wv, yb = ya + 4;
    if (ya >= hc) return;                       // whole waves only: lanes past the canvas edge still help build the table
    const int w64 = gridDim.x;
    const bool inx = x < wc, hasb = yb < hc;
    cv_word* wa = bitmap + (ACC ? 0ll : (long long)blockIdx.z * hc * w64) + (long long)ya * w64 + blockIdx.x;
    cv_word* wb = wa + 4ll * w64;
    // the bits that can still come out as 1: all columns of the canvas, or what the caller's words still hold of them
    const cv_word full = __builtin_amdgcn_ballot_w64(inx);
    cv_word acca = full, accb = hasb ? full : 0ull;
    if (ACC) {
        acca &= *wa;
        if (hasb) accb &= *wb;
    }
    const int f0 = ACC ? 0 : (int)blockIdx.z, f1 = ACC ? frames : f0 + 1;
    for (int f = f0; f < f1; ++f) {
        if ((acca | accb) == 0ull) break;       // nothing can set a bit again
        cv_word cova = 0ull, covb = 0ull;
        for (int k = 0; k < views; ++k) {
            // an OR that holds every bit still asked for cannot change the result: a tile one view covers whole (most of a canvas)
            // skips the other views' splines
            if ((acca & ~cova) == 0ull && (accb & ~covb) == 0ull) break;
            const long long b = (long long)f * views + k;
            ss_f2 xn2, yn2;
            cv_rows_coords(source + b * SS_NV * 2, T + b * 2 * SS_NT, dytab[wv], lx, x, ya, yb, hc, wc, xn2, yn2);
            cova |= __builtin_amdgcn_ballot_w64(inx && cv_mask(xn2.x, yn2.x, w, h, mode) >= min_mask);
            covb |= __builtin_amdgcn_ballot_w64(inx && cv_mask(xn2.y, yn2.y, w, h, mode) >= min_mask);
        }
        acca &= cova;
        accb &= covb;
    }
    if (lx == 0) {
        *wa = acca;
        if (hasb) *wb = accb;
    }
}

// ---- the rectangle search
// heights [hc][wc]: the run of covered pixels that ends at (y, x), upwards.  Only columns < wc exist here: pad bits are never read.
__global__ __launch_bounds__(256) void cv_heights_kernel(const cv_word* __restrict__ bitmap, int* __restrict__ heights, int hc, int wc,
                                                         int w64) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= wc) return;
    const cv_word* col = bitmap + (x >> 6);
    const int sh = x & 63;
    int run = 0;
#pragma unroll 8
    for (int y = 0; y < hc; ++y) {
        run = ((col[(long long)y * w64] >> sh) & 1ull) ? run + 1 : 0;
        heights[(long long)y * wc + x] = run;
    }
}

struct CvRect {
    int y0, x0, h, w;
};
// the order of the answer: larger area, then smaller y0, then smaller x0, then larger width
__device__ __forceinline__ bool cv_better(const CvRect& a, const CvRect& b) {
    const int aa = a.h * a.w, ab = b.h * b.w;
    if (aa != ab) return aa > ab;
    if (a.y0 != b.y0) return a.y0 < b.y0;
    if (a.x0 != b.x0) return a.x0 < b.x0;
    return a.w > b.w;
}
__device__ __forceinline__ CvRect cv_wave_best(CvRect r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        CvRect t;
        t.y0 = __shfl_xor(r.y0, o, 64); t.x0 = __shfl_xor(r.x0, o, 64); t.h = __shfl_xor(r.h, o, 64); t.w = __shfl_xor(r.w, o, 64);
        if (cv_better(t, r)) r = t;
    }
    return r;
}

// One workgroup per row y; tree [2 P] ints in LDS, P = the power of two >= wc: leaves tree[P + i] = heights[y][i] (-1 past the row:
// smaller than every height, the row's right border), tree[n] = min(tree[2 n], tree[2 n + 1]).  Column i's nearest strictly smaller
// neighbour on either side: up from the leaf until a sibling subtree on that side holds a smaller value, then down to its nearest
// leaf -- at most 2 log2 P steps.  -> cand [hc][4 waves][4] = each wave's best (y0, x0, h, w).
__global__ __launch_bounds__(256) void cv_rows_kernel(const int* __restrict__ heights, int* __restrict__ cand, int wc, int P) {
    extern __shared__ int tree[];
    const int y = blockIdx.x, tid = threadIdx.x;
    const int* row = heights + (long long)y * wc;
    for (int i = tid; i < P; i += 256) tree[P + i] = i < wc ? row[i] : -1;
    __syncthreads();
    for (int n = P >> 1; n >= 1; n >>= 1) {
        for (int j = tid; j < n; j += 256) tree[n + j] = min(tree[2 * (n + j)], tree[2 * (n + j) + 1]);
        __syncthreads();
    }
    CvRect best = {0, 0, 0, 0};
    for (int i = tid; i < wc; i += 256) {
        const int hi = tree[P + i];
        if (hi <= 0) continue;
        int L = -1, R = P;
        for (int n = P + i; n > 1; n >>= 1) {
            if ((n & 1) && tree[n - 1] < hi) {
                int m = n - 1;
                while (m < P) m = tree[2 * m + 1] < hi ? 2 * m + 1 : 2 * m;
                L = m - P;
                break;
            }
        }
        for (int n = P + i; n > 1; n >>= 1) {
            if (!(n & 1) && tree[n + 1] < hi) {
                int m = n + 1;
                while (m < P) m = tree[2 * m] < hi ? 2 * m : 2 * m + 1;
                R = m - P;
                break;
            }
        }
        const CvRect c = {y - hi + 1, L + 1, hi, R - L - 1};
        if (cv_better(c, best)) best = c;
    }
    best = cv_wave_best(best);
    if ((tid & 63) == 0) {
        int* o = cand + ((long long)y * 4 + (tid >> 6)) * 4;
        o[0] = best.y0; o[1] = best.x0; o[2] = best.h; o[3] = best.w;
    }
}

__global__ __launch_bounds__(256) void cv_reduce_kernel(const int* __restrict__ cand, int count, int even, int* __restrict__ rect) {
    __shared__ int part[4][4];
    const int tid = threadIdx.x;
    CvRect best = {0, 0, 0, 0};
    for (int i = tid; i < count; i += 256) {
        const int* c = cand + (long long)i * 4;
        const CvRect r = {c[0], c[1], c[2], c[3]};
        if (cv_better(r, best)) best = r;
    }
    best = cv_wave_best(best);
    if ((tid & 63) == 0) {
        int* p = part[tid >> 6];
        p[0] = best.y0; p[1] = best.x0; p[2] = best.h; p[3] = best.w;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            const CvRect r = {part[k][0], part[k][1], part[k][2], part[k][3]};
            if (cv_better(r, best)) best = r;
        }
        if (even) { best.h -= best.h & 1; best.w -= best.w & 1; }
        rect[0] = best.y0; rect[1] = best.x0; rect[2] = best.h; rect[3] = best.w;
    }
}

int cv_status() { return hipGetLastError() == hipSuccess ? SSC_OK : SSC_ERR_LAUNCH; }

bool cv_canvas_ok(int hc, int wc) { return hc > 1 && wc > 1 && wc <= SSC_MAX_WIDTH; }
bool cv_rect_ok(int hc, int wc) { return cv_canvas_ok(hc, wc) && (long long)hc * wc <= 0x7fffffffll; }
long long cv_cand_offset(int hc, int wc) { return ((long long)hc * wc * 4 + 7) / 8 * 8; }

}  // namespace

extern "C" {

SSC_API int ssc_version(void) { return 1; }

SSC_API long long ssc_bitmap_words(int hc, int wc) {
    if (!cv_canvas_ok(hc, wc)) return SSC_ERR_ARG;
    return (long long)hc * ss_cdiv(wc, 64);
}

SSC_API int ssc_coverage(const float* source, const float* T, unsigned long long* bitmap, int frames, int views, int h, int w, int hc,
                         int wc, int mode, float min_mask, int accumulate, void* stream) {
    if (!source || !T || !bitmap || views < 2 || views > SSC_MAX_VIEWS || h <= 1 || w <= 1 || !cv_canvas_ok(hc, wc) ||
        (mode != SSC_WARP_NORMAL && mode != SSC_WARP_FAST) || frames <= 0 || !(min_mask > 0.f && min_mask <= 1.f) ||
        ss_cdiv(hc, 8) > 65535 || (!accumulate && frames > SSC_MAX_FRAMES))
        return SSC_ERR_ARG;
    const dim3 grid(ss_cdiv(wc, 64), ss_cdiv(hc, 8), accumulate ? 1 : frames);
    if (accumulate)
        hipLaunchKernelGGL((cv_coverage_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, source, T, bitmap, frames, views, h, w,
                           hc, wc, mode, min_mask);
    else
        hipLaunchKernelGGL((cv_coverage_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, source, T, bitmap, frames, views, h, w,
                           hc, wc, mode, min_mask);
    return cv_status();
}

SSC_API long long ssc_rect_workspace_bytes(int hc, int wc) {
    if (!cv_rect_ok(hc, wc)) return SSC_ERR_ARG;
    return cv_cand_offset(hc, wc) + (long long)hc * 4 * 4 * 4;
}

SSC_API int ssc_covered_rect(const unsigned long long* bitmap, int hc, int wc, int even, void* ws, long long ws_bytes, int* rect,
                             void* stream) {
    if (!bitmap || !ws || !rect || !cv_rect_ok(hc, wc) || ws_bytes < ssc_rect_workspace_bytes(hc, wc))
        return SSC_ERR_ARG;
    int* heights = static_cast<int*>(ws);
    int* cand = reinterpret_cast<int*>(static_cast<char*>(ws) + cv_cand_offset(hc, wc));
    int P = 2;
    while (P < wc) P <<= 1;
    hipLaunchKernelGGL(cv_heights_kernel, dim3(ss_cdiv(wc, 256)), dim3(256), 0, (hipStream_t)stream, bitmap, heights, hc, wc,
                       ss_cdiv(wc, 64));
    hipLaunchKernelGGL(cv_rows_kernel, dim3(hc), dim3(256), (size_t)2 * P * sizeof(int), (hipStream_t)stream, heights, cand, wc, P);
    hipLaunchKernelGGL(cv_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cand, hc * 4, even, rect);
    return cv_status();
}

}  // extern "C"
