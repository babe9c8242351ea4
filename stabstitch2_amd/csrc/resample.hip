// A rectangle of stitched frames resampled to a fixed size with the triangle prefilter (libstabstitch_resample.so,
// include/stabstitch_resample.h).  One kernel in three output forms, one launch per call.
//
// A workgroup of 256 threads owns an output tile of 16 rows x 64 columns of one frame: lane = column, wave w owns rows 4 w .. 4 w + 3.
// The rectangle is read from the device (or taken from the arguments), the window and the per-axis scale are derived from it in
// double by every thread -- a handful of operations, the same function ssr_source_window runs on the host.
//   staged: when both supports are <= 5 px (at most 11 taps per axis) and the tile's tap rows fit RS_ROWS -- rect / out up to about
//     2.7 per axis -- wave 0 leaves the fp32 column weights and wave 1 the row weights in LDS, the horizontal pass of the source
//     rows the tile needs goes to LDS, the vertical pass reads it with the row's weights.
//   direct: everything else (huge ratios): a double loop per output pixel, weights computed where they are used.
// Both paths do the same arithmetic in the same order (the header states it), so a pixel's bits do not depend on the path; which
// path runs depends on the rectangle and the tile row only, the same for a whole workgroup, so no barrier is divergent.
// Bytes leave through LDS as whole dwords when every output row starts on one, else byte by byte; NV12 reads its 2 x 2 blocks
// back from the tile's bytes in LDS.  No atomics, no scratch; 64-bit element offsets.
#include "nv12.h"

#include "../../include/stabstitch_resample.h"

namespace {

enum { RS_F32 = 0, RS_U8 = 1, RS_NV12 = 2 };
constexpr int RS_TH = 16, RS_TW = 64;    // the output tile
constexpr int RS_K = 12;                 // taps per axis the LDS tables hold: support <= 5 -> at most 2 * 5 + 1
constexpr int RS_ROWS = 48;              // source rows of one tile in LDS: 48 * 3 * 64 * 4 = 36 KiB

struct RsAxis {
    double o, len, scale, sup;           // the window [o, o + len), len / n_out, max(scale, 1)
    int lo, hi;                          // R's integer range: the taps clamp to it
};
struct RsWindow {
    RsAxis y, x;
    bool empty;
};

// the header's "Rectangle" and "Window", term by term
__host__ __device__ inline RsWindow rs_window(int y0, int x0, int h, int w, int Hc, int Wc, int Hout, int Wout, int aspect) {
    RsWindow W;
    const long long ya = y0 > 0 ? y0 : 0, xa = x0 > 0 ? x0 : 0;
    long long yb = (long long)y0 + h, xb = (long long)x0 + w;
    if (yb > Hc) yb = Hc;
    if (xb > Wc) xb = Wc;
    W.empty = h <= 0 || w <= 0 || yb <= ya || xb <= xa;
    if (W.empty) {
        W.y = RsAxis{0.0, 0.0, 1.0, 1.0, 0, 0};
        W.x = W.y;
        return W;
    }
    const long long rh = yb - ya, rw = xb - xa;
    double fy = (double)ya, fx = (double)xa, fh = (double)rh, fw = (double)rw;
    if (aspect == SSR_ASPECT_FILL) {
        const long long a = rw * Hout, b = rh * Wout;
        if (a > b) {
            fw = (double)rh * (double)Wout / (double)Hout;
            fx = (double)xa + ((double)rw - fw) / 2.0;
        } else if (a < b) {
            fh = (double)rw * (double)Hout / (double)Wout;
            fy = (double)ya + ((double)rh - fh) / 2.0;
        }
    }
    W.y.o = fy; W.y.len = fh; W.y.scale = fh / (double)Hout; W.y.sup = W.y.scale > 1.0 ? W.y.scale : 1.0; W.y.lo = (int)ya; W.y.hi = (int)yb;
    W.x.o = fx; W.x.len = fw; W.x.scale = fw / (double)Wout; W.x.sup = W.x.scale > 1.0 ? W.x.scale : 1.0; W.x.lo = (int)xa; W.x.hi = (int)xb;
    return W;
}

// output i of an axis: its centre c, its taps [t0, t1) and the sum of their weights, added in ascending order
__device__ __forceinline__ double rs_weight(const RsAxis& a, double c, int j) {
    const double v = 1.0 - fabs(((double)j + 0.5) - c) / a.sup;
    return v > 0.0 ? v : 0.0;
}
__device__ __forceinline__ void rs_taps(const RsAxis& a, int i, double& c, int& t0, int& t1, double& sum) {
    c = a.o + a.scale * ((double)i + 0.5);
    const double l = floor((c - a.sup) + 0.5), r = floor((c + a.sup) + 0.5);
    t0 = (int)fmax(l, (double)a.lo);
    t1 = (int)fmin(r, (double)a.hi);
    sum = 0.0;
    for (int j = t0; j < t1; ++j) sum += rs_weight(a, c, j);
}
// the fp32 weight of tap j: the one rounding
__device__ __forceinline__ float rs_wf(const RsAxis& a, double c, int j, double sum) { return (float)(rs_weight(a, c, j) / sum); }

// the three channels of source pixel (y, x) of frame f
template <int FMT>
__device__ __forceinline__ void rs_pixel(const void* __restrict__ in, long long f, int Hc, int Wc, int y, int x, float (&p)[3]) {
    if (FMT == RS_F32) {
        const long long plane = (long long)Hc * Wc;
        const float* s = static_cast<const float*>(in) + f * 3 * plane + (long long)y * Wc + x;
        p[0] = s[0]; p[1] = s[plane]; p[2] = s[2 * plane];
    } else {
        const unsigned char* s = static_cast<const unsigned char*>(in) + ((f * Hc + y) * Wc + x) * 3;
        p[0] = (float)s[0]; p[1] = (float)s[1]; p[2] = (float)s[2];
    }
}

__device__ __forceinline__ unsigned char rs_byte(float v) { return (unsigned char)min(max((int)floorf(v + 0.5f), 0), 255); }

struct RsOut {
    void* p0;                            // fp32 planes | BGR bytes | Y plane
    unsigned char* uv;                   // NV12's UV plane
    long long stride;                    // bytes between frames (bytes forms)
    int pitch;                           // NV12
    int dwords;                          // BGR bytes: every output row starts on a dword and holds whole ones
};

template <int FMT>
__global__ __launch_bounds__(256) void rs_resample_kernel(const void* __restrict__ in, RsOut out, const int* __restrict__ rect_dev,
                                                          int ry, int rx, int rh, int rw, int Hc, int Wc, int Hout, int Wout,
                                                          int aspect) {
    __shared__ float hbuf[RS_ROWS][3][RS_TW];
    __shared__ float wxs[RS_K][RS_TW];
    __shared__ float wys[RS_TH][RS_K];
    __shared__ int xt0[RS_TW], xcn[RS_TW], yt0[RS_TH], ycn[RS_TH];
    __shared__ __attribute__((aligned(4))) unsigned char ot8[RS_TH][RS_TW * 3];

    const int tid = threadIdx.x, lx = tid & 63, wv = tid >> 6;
    const int tx = blockIdx.x * RS_TW, ty = blockIdx.y * RS_TH;
    const long long f = blockIdx.z;
    const int ox = tx + lx;
    if (rect_dev) { ry = rect_dev[0]; rx = rect_dev[1]; rh = rect_dev[2]; rw = rect_dev[3]; }
    const RsWindow W = rs_window(ry, rx, rh, rw, Hc, Wc, Hout, Wout, aspect);

    float acc[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.f;

    if (!W.empty) {
        bool staged = 2.0 * W.y.sup + 2.0 <= (double)RS_K && 2.0 * W.x.sup + 2.0 <= (double)RS_K;
        int row0 = 0, rows = 0;
        if (staged) {
            if (wv == 0) {
                int t0 = 0, t1 = 0;
                if (ox < Wout) {
                    double c, s;
                    rs_taps(W.x, ox, c, t0, t1, s);
                    t1 = min(t1, t0 + RS_K);
                    for (int j = t0; j < t1; ++j) wxs[j - t0][lx] = rs_wf(W.x, c, j, s);
                }
                xt0[lx] = t0; xcn[lx] = max(t1 - t0, 0);
            } else if (wv == 1 && lx < RS_TH) {
                int t0 = 0, t1 = 0;
                if (ty + lx < Hout) {
                    double c, s;
                    rs_taps(W.y, ty + lx, c, t0, t1, s);
                    t1 = min(t1, t0 + RS_K);
                    for (int j = t0; j < t1; ++j) wys[lx][j - t0] = rs_wf(W.y, c, j, s);
                }
                yt0[lx] = t0; ycn[lx] = max(t1 - t0, 0);
            }
            __syncthreads();
            const int last = min(RS_TH, Hout - ty) - 1;      // tap ranges only move forward with the output row
            row0 = yt0[0];
            rows = yt0[last] + ycn[last] - row0;
            staged = rows <= RS_ROWS;
        }
        if (staged) {
            const int t0 = xt0[lx], cn = xcn[lx];
            for (int r = wv; r < rows; r += 4) {
                float h0 = 0.f, h1 = 0.f, h2 = 0.f;
                for (int k = 0; k < cn; ++k) {
                    float p[3];
                    rs_pixel<FMT>(in, f, Hc, Wc, row0 + r, t0 + k, p);
                    const float wk = wxs[k][lx];
                    h0 = fmaf(wk, p[0], h0); h1 = fmaf(wk, p[1], h1); h2 = fmaf(wk, p[2], h2);
                }
                hbuf[r][0][lx] = h0; hbuf[r][1][lx] = h1; hbuf[r][2][lx] = h2;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int oyl = wv * 4 + q;
                const int cn_y = ycn[oyl], b = yt0[oyl] - row0;
                for (int j = 0; j < cn_y; ++j) {
                    const float wj = wys[oyl][j];
                    acc[q][0] = fmaf(wj, hbuf[b + j][0][lx], acc[q][0]);
                    acc[q][1] = fmaf(wj, hbuf[b + j][1][lx], acc[q][1]);
                    acc[q][2] = fmaf(wj, hbuf[b + j][2][lx], acc[q][2]);
                }
            }
        } else if (ox < Wout) {
            double cx, sx;
            int x0, x1;
            rs_taps(W.x, ox, cx, x0, x1, sx);
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                const int oy = ty + wv * 4 + q;
                if (oy >= Hout) break;
                double cy, sy;
                int y0, y1;
                rs_taps(W.y, oy, cy, y0, y1, sy);
                for (int j = y0; j < y1; ++j) {
                    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
                    for (int k = x0; k < x1; ++k) {
                        float p[3];
                        rs_pixel<FMT>(in, f, Hc, Wc, j, k, p);
                        const float wk = rs_wf(W.x, cx, k, sx);
                        h0 = fmaf(wk, p[0], h0); h1 = fmaf(wk, p[1], h1); h2 = fmaf(wk, p[2], h2);
                    }
                    const float wj = rs_wf(W.y, cy, j, sy);
                    acc[q][0] = fmaf(wj, h0, acc[q][0]); acc[q][1] = fmaf(wj, h1, acc[q][1]); acc[q][2] = fmaf(wj, h2, acc[q][2]);
                }
            }
        }
    }

    // ---- the tile leaves
    if (FMT == RS_F32) {
        if (ox >= Wout) return;
        const long long plane = (long long)Hout * Wout;
        float* o = static_cast<float*>(out.p0) + f * 3 * plane;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int oy = ty + wv * 4 + q;
            if (oy >= Hout) break;
            float* d = o + (long long)oy * Wout + ox;
            d[0] = acc[q][0]; d[plane] = acc[q][1]; d[2 * plane] = acc[q][2];
        }
        return;
    }
    if (FMT == RS_U8 && !out.dwords) {
        if (ox >= Wout) return;
        unsigned char* o = static_cast<unsigned char*>(out.p0) + f * out.stride;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int oy = ty + wv * 4 + q;
            if (oy >= Hout) break;
            unsigned char* d = o + ((long long)oy * Wout + ox) * 3;
            d[0] = rs_byte(acc[q][0]); d[1] = rs_byte(acc[q][1]); d[2] = rs_byte(acc[q][2]);
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned char* d = &ot8[wv * 4 + q][lx * 3];
        d[0] = rs_byte(acc[q][0]); d[1] = rs_byte(acc[q][1]); d[2] = rs_byte(acc[q][2]);
    }
    __syncthreads();
    const int cols = min(RS_TW, Wout - tx), trows = min(RS_TH, Hout - ty);
    if (FMT == RS_U8) {
        // (tx * 3 and Wout * 3 are multiples of 4 here, so cols * 3 is one too)
        const int dw = cols * 3 / 4;
        unsigned char* o = static_cast<unsigned char*>(out.p0) + f * out.stride;
        for (int i = tid; i < trows * dw; i += 256) {
            const int r = i / dw, c = i - r * dw;
            *reinterpret_cast<uint32_t*>(o + ((long long)(ty + r) * Wout + tx) * 3 + 4 * c) =
                *reinterpret_cast<const uint32_t*>(&ot8[r][4 * c]);
        }
    } else {
        // one thread = one 2 x 2 block, as canvas_u8x1_kernel's NV12 form (frameio.hip) reads it from the BGR frame
        const int bx = tid & 31, by = tid >> 5;
        if (2 * bx >= cols || 2 * by >= trows) return;
        const long long fo = f * out.stride;
        unsigned char* y0 = static_cast<unsigned char*>(out.p0) + fo + (long long)(ty + 2 * by) * out.pitch + tx + 2 * bx;
        int s[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned char* p0 = &ot8[2 * by][(2 * bx + k) * 3];
            const unsigned char* p1 = &ot8[2 * by + 1][(2 * bx + k) * 3];
            const int b0 = p0[0], g0 = p0[1], r0 = p0[2], b1 = p1[0], g1 = p1[1], r1 = p1[2];
            y0[k] = bgr_to_y(b0, g0, r0);
            y0[out.pitch + k] = bgr_to_y(b1, g1, r1);
            s[0] += b0 + b1; s[1] += g0 + g1; s[2] += r0 + r1;
        }
        *reinterpret_cast<unsigned short*>(out.uv + fo + (long long)((ty >> 1) + by) * out.pitch + tx + 2 * bx) =
            bgr4_to_uv(s[0], s[1], s[2]);
    }
}

bool rs_args_ok(const void* in, int n, int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev, int y0, int x0, int h,
                int w) {
    if (!in || n <= 0 || n > SSR_MAX_FRAMES || Hc < 1 || Wc < 1 || Hout < 1 || Wout < 1) return false;
    if ((long long)Hc * Wc > 0x7fffffffll || (long long)Hout * Wout > 0x7fffffffll) return false;
    if (ss_cdiv(Hout, RS_TH) > 65535 || ss_cdiv(Wout, RS_TW) > 65535) return false;
    if (aspect != SSR_ASPECT_STRETCH && aspect != SSR_ASPECT_FILL) return false;
    return rect_dev || (y0 >= 0 && x0 >= 0 && h >= 0 && w >= 0);
}

template <int FMT>
int rs_launch(const void* in, RsOut out, int n, int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev, int y0, int x0,
              int h, int w, void* stream) {
    const dim3 grid(ss_cdiv(Wout, RS_TW), ss_cdiv(Hout, RS_TH), n);
    hipLaunchKernelGGL((rs_resample_kernel<FMT>), grid, dim3(256), 0, (hipStream_t)stream, in, out, rect_dev, y0, x0, h, w, Hc, Wc,
                       Hout, Wout, aspect);
    return hipGetLastError() == hipSuccess ? SSR_OK : SSR_ERR_LAUNCH;
}

}  // namespace

extern "C" {

SSR_API int ssr_version(void) { return 1; }

SSR_API int ssr_source_window(const int rect[4], int Hc, int Wc, int Hout, int Wout, int aspect, double out[4]) {
    if (!rect || !out || !rs_args_ok(rect, 1, Hc, Wc, Hout, Wout, aspect, nullptr, rect[0], rect[1], rect[2], rect[3]))
        return SSR_ERR_ARG;
    const RsWindow W = rs_window(rect[0], rect[1], rect[2], rect[3], Hc, Wc, Hout, Wout, aspect);
    out[0] = W.empty ? 0.0 : W.y.o;
    out[1] = W.empty ? 0.0 : W.x.o;
    out[2] = W.empty ? 0.0 : W.y.len;
    out[3] = W.empty ? 0.0 : W.x.len;
    return SSR_OK;
}

SSR_API int ssr_resample_f32(const float* in, float* out, int n, int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev,
                             int y0, int x0, int h, int w, void* stream) {
    if (!out || !rs_args_ok(in, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w)) return SSR_ERR_ARG;
    return rs_launch<RS_F32>(in, RsOut{out, nullptr, 0, 0, 0}, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w, stream);
}

SSR_API int ssr_resample_u8(const unsigned char* in, unsigned char* out, long long out_frame_stride, int n, int Hc, int Wc, int Hout,
                            int Wout, int aspect, const int* rect_dev, int y0, int x0, int h, int w, void* stream) {
    if (!out || !rs_args_ok(in, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w) ||
        out_frame_stride < 3ll * Hout * Wout)
        return SSR_ERR_ARG;
    const int dwords = (3ll * Wout) % 4 == 0 && (((uintptr_t)out) & 3) == 0 && (out_frame_stride & 3) == 0;
    return rs_launch<RS_U8>(in, RsOut{out, nullptr, out_frame_stride, 0, dwords}, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w,
                            stream);
}

SSR_API int ssr_resample_u8_nv12(const unsigned char* in, unsigned char* y, unsigned char* uv, int pitch, long long frame_stride, int n,
                                 int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev, int y0, int x0, int h, int w,
                                 void* stream) {
    if (!y || !uv || !rs_args_ok(in, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w) || (Hout & 1) || (Wout & 1) ||
        (pitch & 1) || pitch < Wout || (((uintptr_t)uv) & 1) || (frame_stride & 1) || frame_stride < (long long)pitch * (Hout / 2 * 3))
        return SSR_ERR_ARG;
    return rs_launch<RS_NV12>(in, RsOut{y, uv, frame_stride, pitch, 0}, n, Hc, Wc, Hout, Wout, aspect, rect_dev, y0, x0, h, w, stream);
}

}  // extern "C"
