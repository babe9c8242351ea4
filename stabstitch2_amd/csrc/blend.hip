// libstabstitch_blend.so: MULTIBAND fusion of warped views (include/stabstitch_blend.h).  gfx950 only.
//
// The blend is computed in its difference form.  With the seam weights s_v a partition of unity, the last view's filled colours
// `base` = c'_{V-1} and d_v = c'_v - base for the K = V - 1 other views,
//     sum_v G(s_v) L(c'_v)  =  L(base) + sum_{v < K} G(s_v) L(d_v)
// at every level, and the pyramid of `base` collapses to `base` itself: only the K * 3 difference planes and the K weight planes
// get pyramids (4 planes for two views instead of 8), and identical views give d = 0, hence their own samples bit for bit.
//
// Workspace of one frame (floats; s_l = row stride of level l, a multiple of 4 so that every row starts 16-byte aligned):
//     pyr[l], l = 0..B   K x {d_B, d_G, d_R, s} planes of h_l x s_l
//     col[l], l = 1..B   the collapsed colour planes r_l, 3 of h_l x s_l
//     base               3 planes of h_0 x s_0;   uni: 1 plane (1 inside the union of the masks, else 0)
// Columns w_l .. s_l - 1 of a row are never meaningful: loads that touch them feed no stored value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stabstitch_blend.h"

namespace {

struct MbLevel {
    int h, w, s;
    long long a;       // h * s
};

struct MbPlan {
    int bands, K;
    MbLevel lv[SSB_MAX_BANDS + 1];
    long long pyr[SSB_MAX_BANDS + 1], col[SSB_MAX_BANDS + 1], base, uni, frame_floats;
};

// false: arguments the library refuses
bool mb_plan(int frames, int views, int hc, int wc, int bands, MbPlan* p) {
    if (frames < 1 || frames > 65535 || views < 2 || views > SSB_MAX_VIEWS || bands < 0 || bands > SSB_MAX_BANDS) return false;
    if (hc < 1 || wc < 1 || hc > 32768 || wc > 32768) return false;
    p->bands = bands;
    p->K = views - 1;
    if ((long long)frames * 4 * p->K > 65535) return false;       // frames x planes ride in gridDim.z
    int h = hc, w = wc;
    for (int l = 0; l <= bands; ++l) {
        p->lv[l].h = h; p->lv[l].w = w; p->lv[l].s = (w + 3) & ~3;
        p->lv[l].a = (long long)h * p->lv[l].s;
        if (l < bands) {
            if (h < 3 || w < 3) return false;                     // a level that is reduced reflects two pixels past its edge
            h = (h + 1) / 2; w = (w + 1) / 2;
        }
    }
    long long off = 0;
    for (int l = 0; l <= bands; ++l) { p->pyr[l] = off; off += 4LL * p->K * p->lv[l].a; }
    p->col[0] = -1;
    for (int l = 1; l <= bands; ++l) { p->col[l] = off; off += 3 * p->lv[l].a; }
    p->base = off; off += 3 * p->lv[0].a;
    p->uni = off; off += p->lv[0].a;
    p->frame_floats = off;
    return off < 0x7fffffffLL;                                    // offsets inside a frame are ints in the kernels
}

// index reflected without repeating the edge (-1 -> 1, n -> n - 2), then clamped: a tile reaches further past the plane than
// any tap that is used does, and those cells only have to be loadable
__device__ __forceinline__ int mb_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);
}

// ---------------------------------------------------------------------------------------------------------------
// prepare: the decisions (valid, union, owner), the fill, and the level-0 planes.  One thread = one canvas pixel.
template <int V>
__global__ __launch_bounds__(256) void mb_prepare_kernel(const float* __restrict__ P, float* __restrict__ ws, long long frame_floats,
                                                         long long base_off, long long uni_off, int hc, int wc, int s0) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= wc || y >= hc) return;
    const size_t plane = (size_t)hc * wc;
    const float* p = P + (size_t)blockIdx.z * (V * 5) * plane + (size_t)y * wc + x;
    float c[V][3], wgt[V];
    bool valid[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = p[(size_t)(v * 5 + k) * plane];
        wgt[v] = p[(size_t)(v * 5 + 3) * plane];
        valid[v] = p[(size_t)(v * 5 + 4) * plane] >= 0.5f;
    }
    int owner = 0;
    bool uni = false;
    float best = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (valid[v] && (!uni || wgt[v] > best)) { owner = v; best = wgt[v]; uni = true; }
    }
    float co[3] = {0.f, 0.f, 0.f};                                // the owner's colours (0 outside the union)
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) co[k] = (uni && owner == v) ? c[v][k] : co[k];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[v][k] = valid[v] ? c[v][k] : co[k];
    }
    const size_t a0 = (size_t)hc * s0;
    float* f = ws + (size_t)blockIdx.z * frame_floats + (size_t)y * s0 + x;
#pragma unroll
    for (int v = 0; v < V - 1; ++v) {
#pragma unroll
        for (int k = 0; k < 3; ++k) f[(size_t)(v * 4 + k) * a0] = c[v][k] - c[V - 1][k];
        f[(size_t)(v * 4 + 3) * a0] = owner == v ? 1.f : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) f[base_off + k * a0] = c[V - 1][k];
    f[uni_off] = uni ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// reduce: [1 4 6 4 1] / 16 along x, then along y, at the even positions.  One workgroup = a 16 x 32 tile of one plane of the coarser
// level; every plane of every frame in one launch.  The 35 x 67 input patch (2-pixel halo) is staged in LDS as 35 x 18 aligned quads:
// a quad inside the plane is one 16-byte load, a quad across an edge is four reflected loads.
#define MB_RT_W 32
#define MB_RT_H 16
#define MB_RT_Q (2 * MB_RT_W / 4 + 2)        // quads per staged row: 18
#define MB_RT_IW (4 * MB_RT_Q)               // 72
#define MB_RT_IH (2 * MB_RT_H + 3)           // 35

__global__ __launch_bounds__(256) void mb_reduce_kernel(float* __restrict__ ws, long long frame_floats, long long in_off, long long out_off,
                                                        int planes, int h, int w, int s, int ho, int wo, int so) {
    __shared__ __attribute__((aligned(16))) float tile[MB_RT_IH][MB_RT_IW];
    __shared__ float hor[MB_RT_IH][MB_RT_W + 1];
    const int fz = blockIdx.z / planes, pl = blockIdx.z - fz * planes;
    const float* in = ws + (size_t)fz * frame_floats + in_off + (size_t)pl * h * s;
    float* out = ws + (size_t)fz * frame_floats + out_off + (size_t)pl * ho * so;
    const int x0 = blockIdx.x * MB_RT_W, y0 = blockIdx.y * MB_RT_H;
    const int c0 = 2 * x0 - 4, r0 = 2 * y0 - 2;                  // plane column of tile column 0 (a multiple of 4), plane row of tile row 0
    for (int q = threadIdx.x; q < MB_RT_IH * MB_RT_Q; q += 256) {
        const int r = q / MB_RT_Q, qi = q - r * MB_RT_Q;
        const float* row = in + (size_t)mb_reflect(r0 + r, h) * s;
        const int c = c0 + 4 * qi;
        float4 v;
        if (c >= 0 && c + 3 < w) {
            v = *reinterpret_cast<const float4*>(row + c);
        } else {
            v.x = row[mb_reflect(c, w)]; v.y = row[mb_reflect(c + 1, w)];
            v.z = row[mb_reflect(c + 2, w)]; v.w = row[mb_reflect(c + 3, w)];
        }
        *reinterpret_cast<float4*>(&tile[r][4 * qi]) = v;
    }
    __syncthreads();
    // plane column 2 (x0 + xo) + j - 2 is tile column 2 xo + 2 + j
    for (int i = threadIdx.x; i < MB_RT_IH * MB_RT_W; i += 256) {
        const int r = i >> 5, xo = i & 31;
        const float* t = &tile[r][2 * xo + 2];
        hor[r][xo] = (((t[0] + t[4]) + 4.f * (t[1] + t[3])) + 6.f * t[2]) * 0.0625f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int yo = (threadIdx.x >> 5) + 8 * k, xo = threadIdx.x & 31;
        const float v = (((hor[2 * yo][xo] + hor[2 * yo + 4][xo]) + 4.f * (hor[2 * yo + 1][xo] + hor[2 * yo + 3][xo])) +
                         6.f * hor[2 * yo + 2][xo]) * 0.0625f;
        if (y0 + yo < ho && x0 + xo < wo) out[(size_t)(y0 + yo) * so + x0 + xo] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// collapse: r_l = sum_{v < K} G_l(s_v) (G_l(d_v) - expand(G_{l+1}(d_v))) + expand(r_{l+1}); the Laplacians live in registers only.
// One thread = one pixel of the coarser level = a 2 x 2 quad of this level: the nine coarse neighbours serve all four expands.
struct MbNbr {
    int xm, x0, xp, ym, y0, yp;      // the coarse 3 x 3: element offsets of its columns, and of its rows (row * stride)
};

// expand of one plane at the quad: e[0] (even y, even x), e[1] (even y, odd x), e[2] (odd y, even x), e[3] (odd y, odd x);
// even outputs (u[t-1] + 6 u[t] + u[t+1]) / 8, odd outputs (u[t] + u[t+1]) / 2, along x and then along y
__device__ __forceinline__ void mb_expand(const float* __restrict__ u, const MbNbr& n, float e[4]) {
    float ev[3], od[3];
    const int rows[3] = {n.ym, n.y0, n.yp};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float a = u[rows[j] + n.xm], b = u[rows[j] + n.x0], c = u[rows[j] + n.xp];
        ev[j] = ((a + c) + 6.f * b) * 0.125f;
        od[j] = (b + c) * 0.5f;
    }
    e[0] = ((ev[0] + ev[2]) + 6.f * ev[1]) * 0.125f;
    e[1] = ((od[0] + od[2]) + 6.f * od[1]) * 0.125f;
    e[2] = (ev[1] + ev[2]) * 0.5f;
    e[3] = (od[1] + od[2]) * 0.5f;
}

#define MB_OUT_LEVEL 0      // r_l into the workspace
#define MB_OUT_F32 1        // level 0: + base, union, clamp -> fp32 [frames][3][h][w]
#define MB_OUT_U8 2         //          the same values truncated -> uint8 [frames][h][w][3]

template <int V, bool COARSE, int OUT>
__global__ __launch_bounds__(256) void mb_collapse_kernel(float* __restrict__ ws, long long frame_floats, long long d_off, long long dc_off,
                                                          long long r_off, long long rc_off, long long base_off, long long uni_off,
                                                          void* __restrict__ outp, int h, int w, int s, int hm, int wm, int sm) {
    const int tx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ty = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (tx >= ((w + 1) >> 1) || ty >= ((h + 1) >> 1)) return;
    const int x = 2 * tx, y = 2 * ty;
    const bool hx = x + 1 < w, hy = y + 1 < h;
    float* f = ws + (size_t)blockIdx.z * frame_floats;
    const size_t a = (size_t)h * s, am = (size_t)hm * sm;
    const int top = y * s + x, bot = (hy ? y + 1 : y) * s + x;       // (a last odd row reads the row above it again: loadable, unused)
    MbNbr n;
    if (COARSE) {                                                    // tx < wm and ty < hm: the coarse level has (n + 1) / 2 per axis
        n.xm = tx > 0 ? tx - 1 : 1; n.x0 = tx; n.xp = tx + 1 < wm ? tx + 1 : wm - 2;
        n.ym = (ty > 0 ? ty - 1 : 1) * sm; n.y0 = ty * sm; n.yp = (ty + 1 < hm ? ty + 1 : hm - 2) * sm;
    }
    float acc[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[c][i] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < V - 1; ++k) {
        const float* sp = f + d_off + (size_t)(k * 4 + 3) * a;
        const float2 st = *reinterpret_cast<const float2*>(sp + top), sb = *reinterpret_cast<const float2*>(sp + bot);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* dp = f + d_off + (size_t)(k * 4 + c) * a;
            const float2 dt = *reinterpret_cast<const float2*>(dp + top), db = *reinterpret_cast<const float2*>(dp + bot);
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (COARSE) mb_expand(f + dc_off + (size_t)(k * 4 + c) * am, n, e);
            acc[c][0] += st.x * (dt.x - e[0]);
            acc[c][1] += st.y * (dt.y - e[1]);
            acc[c][2] += sb.x * (db.x - e[2]);
            acc[c][3] += sb.y * (db.y - e[3]);
        }
    }
    if (COARSE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float e[4];
            mb_expand(f + rc_off + (size_t)c * am, n, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[c][i] += e[i];
        }
    }
    if (OUT == MB_OUT_LEVEL) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* rp = f + r_off + (size_t)c * a;
            *reinterpret_cast<float2*>(rp + top) = make_float2(acc[c][0], acc[c][1]);      // x + 1 <= s - 1: inside the row
            if (hy) *reinterpret_cast<float2*>(rp + bot) = make_float2(acc[c][2], acc[c][3]);
        }
    } else {
        const float2 ut = *reinterpret_cast<const float2*>(f + uni_off + top), ub = *reinterpret_cast<const float2*>(f + uni_off + bot);
        const float u[4] = {ut.x, ut.y, ub.x, ub.y};
        const bool on[4] = {true, hx, hy, hx && hy};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* bp = f + base_off + (size_t)c * a;
            const float2 bt = *reinterpret_cast<const float2*>(bp + top), bb = *reinterpret_cast<const float2*>(bp + bot);
            const float b[4] = {bt.x, bt.y, bb.x, bb.y};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!on[i]) continue;
                const float v = u[i] >= 0.5f ? fminf(fmaxf(acc[c][i] + b[i], 0.f), 255.f) : 0.f;
                const int px = x + (i & 1), py = y + (i >> 1);
                if (OUT == MB_OUT_F32)
                    static_cast<float*>(outp)[((size_t)blockIdx.z * 3 + c) * h * w + (size_t)py * w + px] = v;
                else
                    static_cast<unsigned char*>(outp)[(((size_t)blockIdx.z * h + py) * w + px) * 3 + c] = (unsigned char)(int)v;
            }
        }
    }
}

int mb_status() { return hipGetLastError() == hipSuccess ? SSB_OK : SSB_ERR_LAUNCH; }

inline int mb_cdiv(int a, int b) { return (a + b - 1) / b; }

template <int V, bool COARSE>
void mb_launch_collapse(int out_kind, const MbPlan& p, int l, float* ws, void* out, int frames, hipStream_t st) {
    const MbLevel& L = p.lv[l];
    const MbLevel& M = p.lv[COARSE ? l + 1 : l];
    const dim3 grid(mb_cdiv((L.w + 1) / 2, 64), mb_cdiv((L.h + 1) / 2, 4), frames), block(256);
    const long long dc = COARSE ? p.pyr[l + 1] : 0, rc = COARSE ? p.col[l + 1] : 0, r = l > 0 ? p.col[l] : 0;
#define MB_GO(KIND) \
    hipLaunchKernelGGL((mb_collapse_kernel<V, COARSE, KIND>), grid, block, 0, st, ws, p.frame_floats, p.pyr[l], dc, r, rc, p.base, p.uni, out, \
                       L.h, L.w, L.s, M.h, M.w, M.s)
    if (out_kind == MB_OUT_LEVEL) MB_GO(MB_OUT_LEVEL);
    else if (out_kind == MB_OUT_F32) MB_GO(MB_OUT_F32);
    else MB_GO(MB_OUT_U8);
#undef MB_GO
}

template <int V>
int mb_run(const float* P, void* out, int final_kind, float* ws, const MbPlan& p, int frames, hipStream_t st) {
    const MbLevel& L0 = p.lv[0];
    hipLaunchKernelGGL((mb_prepare_kernel<V>), dim3(mb_cdiv(L0.w, 64), mb_cdiv(L0.h, 4), frames), dim3(256), 0, st, P, ws, p.frame_floats,
                       p.base, p.uni, L0.h, L0.w, L0.s);
    const int planes = 4 * p.K;
    for (int l = 0; l < p.bands; ++l) {
        const MbLevel& A = p.lv[l];
        const MbLevel& B = p.lv[l + 1];
        hipLaunchKernelGGL(mb_reduce_kernel, dim3(mb_cdiv(B.w, MB_RT_W), mb_cdiv(B.h, MB_RT_H), frames * planes), dim3(256), 0, st, ws,
                           p.frame_floats, p.pyr[l], p.pyr[l + 1], planes, A.h, A.w, A.s, B.h, B.w, B.s);
    }
    mb_launch_collapse<V, false>(p.bands == 0 ? final_kind : MB_OUT_LEVEL, p, p.bands, ws, out, frames, st);
    for (int l = p.bands - 1; l >= 0; --l) mb_launch_collapse<V, true>(l == 0 ? final_kind : MB_OUT_LEVEL, p, l, ws, out, frames, st);
    return mb_status();
}

int mb_blend(const float* P, void* out, int final_kind, float* ws, long long ws_floats, int frames, int views, int hc, int wc, int bands,
             void* stream) {
    MbPlan p;
    if (!P || !out || !ws || !mb_plan(frames, views, hc, wc, bands, &p)) return SSB_ERR_ARG;
    if (ws_floats < p.frame_floats * frames || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return SSB_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return views == 2 ? mb_run<2>(P, out, final_kind, ws, p, frames, st) : mb_run<3>(P, out, final_kind, ws, p, frames, st);
}

}      // namespace

extern "C" {

SSB_API int ssb_version(void) { return 1; }

SSB_API long long ssb_multiband_workspace_floats(int frames, int views, int hc, int wc, int bands) {
    MbPlan p;
    if (!mb_plan(frames, views, hc, wc, bands, &p)) return -1;
    return p.frame_floats * frames;
}

SSB_API int ssb_multiband_blend(const float* P, float* out, float* ws, long long ws_floats, int frames, int views, int hc, int wc, int bands,
                                void* stream) {
    return mb_blend(P, out, MB_OUT_F32, ws, ws_floats, frames, views, hc, wc, bands, stream);
}

SSB_API int ssb_multiband_blend_u8(const float* P, unsigned char* out, float* ws, long long ws_floats, int frames, int views, int hc, int wc,
                                   int bands, void* stream) {
    return mb_blend(P, out, MB_OUT_U8, ws, ws_floats, frames, views, hc, wc, bands, stream);
}

}
