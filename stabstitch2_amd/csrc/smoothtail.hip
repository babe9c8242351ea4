// libstabstitch_smoothtail.so: SmoothNet's three Conv3d(128,128,(5,3,3)) layers and the decoder for a stitched clip, restricted to
// the frames ss_smooth_stitch reads (include/stabstitch_smoothtail.h).
//
// The GEMM is conv.hip's: fp32 v_mfma_f32_32x32x2_f32, D[m][co] = sum_k A[m][k] * Wt[co][k], k = (dt, dh, dw, ci) walked 32 at a
// time, lane half h of an MFMA taking k = 16h + j of the tile, 64 x 64 output tiles on 2 x 2 waves.  What differs is M: ONE
// (window, frame) per M tile (63 mesh vertices + one idle row), so that
//   * the temporal taps an output frame has inside the window are the same for the whole workgroup: the K tiles of a tap in the
//     zero padding are not walked at all (they are whole tiles at the two ends of K: the walk stays one contiguous range);
//   * the input and output frames of a tile are found with one small division per workgroup (compact activations: a later window
//     holds only the frames the next layer reads).
// The sum of an output value equals conv_igemm_kernel's for the full windows bit for bit: same instruction, same k order, the K
// cut (`seg_tiles`) is the caller's -- pipeline.smooth_stage passes the cut ss_conv_nhwc makes for the same windows -- and the
// partial sums are added in the order splitk_reduce_kernel adds them.  A skipped product is a zero.
#include "common.h"

#include "../../include/stabstitch_smoothtail.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ST_T = 7;                  // frames of a window
constexpr int ST_C = 128;                // channels, in and out
constexpr int ST_GH = 7, ST_GW = 9;      // the mesh grid: SS_NV = 63 vertices
constexpr int ST_BK = 32;
constexpr int ST_LDK = ST_BK + 4;        // LDS row stride in dwords (4 * odd: conflict-free 16-byte reads)
constexpr int ST_TAP_TILES = ST_C / ST_BK;                   // 4 K tiles per filter tap
constexpr int ST_DT_TILES = 9 * ST_TAP_TILES;                // 36 K tiles per temporal tap
constexpr int ST_K = 5 * 9 * ST_C;                           // 5760
static_assert(ST_K / ST_BK == SST_K_TILES, "K tiles");

struct TailP {
    const float* in;
    const float* wgt;
    const float* bias;
    float* out;              // compact output, or the partial sums [nseg][frames_out * 63][128]
    int first_in, first_out;
    int frames_out;          // M tiles
    int seg_tiles, nseg;
    int direct;              // 1: bias + ReLU here; 0: raw partial sums, st_reduce_kernel finishes
};

// grid (frames_out, 2 cout tiles, nseg)
__global__ __launch_bounds__(256) void st_conv3d_kernel(TailP p) {
    __shared__ __attribute__((aligned(16))) float As[2][64 * ST_LDK];
    __shared__ __attribute__((aligned(16))) float Bs[2][64 * ST_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int j = blockIdx.x, n0 = blockIdx.y * 64, seg = blockIdx.z;

    // the tile's (window, output frame) and where the window's frame 0 would sit in the compact input
    const int cnt_in = ST_T - p.first_in, cnt_out = ST_T - p.first_out;
    int win = 0, fo = j;
    if (j >= ST_T) {
        const int q = (j - ST_T) / cnt_out;
        win = 1 + q;
        fo = p.first_out + (j - ST_T) - q * cnt_out;
    }
    const long long in_f0 = win == 0 ? 0ll : (long long)ST_T + (long long)(win - 1) * cnt_in - p.first_in;

    // live temporal taps: input frame fo + dt - 2 in 0..6; their K tiles form one range, cut to this segment's
    const int dlo = fo < 2 ? 2 - fo : 0, dhi = fo > 4 ? 8 - fo : 4;
    int ka = seg * p.seg_tiles, kb = ka + p.seg_tiles;
    kb = kb < SST_K_TILES ? kb : SST_K_TILES;
    ka = ka > dlo * ST_DT_TILES ? ka : dlo * ST_DT_TILES;
    kb = kb < (dhi + 1) * ST_DT_TILES ? kb : (dhi + 1) * ST_DT_TILES;

    // staging: thread (lrow, kq) carries float4 kq of rows lrow and lrow + 32 of both operands
    const int lrow = tid >> 3, kq = tid & 7;
    const int vh0 = lrow / ST_GW, vw0 = lrow - vh0 * ST_GW;
    const int vh1 = (lrow + 32) / ST_GW, vw1 = lrow + 32 - vh1 * ST_GW;      // row 63 (idle): vh1 = 7, never inside the grid
    const float* wrow0 = p.wgt + (long long)(n0 + lrow) * ST_K + kq * 4;
    const float* wrow1 = wrow0 + 32 * ST_K;

    // A tap outside the grid (and the idle row) reads the frame's first vertex, which is always there, and is zeroed on its way into
    // LDS, behind the MFMAs: a select right at the load would make every K tile wait for its own loads.
    f32x4 ra0, ra1, rb0, rb1;
    bool ok0 = false, ok1 = false;
    auto aoff = [&](int vhi, int vwi, int dh, int dw, bool& ok) -> int {
        const int y = vhi + dh - 1, x = vwi + dw - 1;
        ok = vhi < ST_GH && y >= 0 && y < ST_GH && x >= 0 && x < ST_GW;
        return ok ? (y * ST_GW + x) * ST_C : 0;
    };
    auto gload = [&](int kt) {
        const int tap = kt >> 2, ci = (kt & 3) * ST_BK + kq * 4;
        const int dt = tap / 9, rem = tap - dt * 9;
        const int dh = rem / 3, dw = rem - dh * 3;
        const float* frame = p.in + (in_f0 + fo + dt - 2) * (long long)(SS_NV * ST_C) + ci;
        ra0 = *reinterpret_cast<const f32x4*>(frame + aoff(vh0, vw0, dh, dw, ok0));
        ra1 = *reinterpret_cast<const f32x4*>(frame + aoff(vh1, vw1, dh, dw, ok1));
        rb0 = *reinterpret_cast<const f32x4*>(wrow0 + kt * ST_BK);
        rb1 = *reinterpret_cast<const f32x4*>(wrow1 + kt * ST_BK);
    };
    auto lstore = [&](int buf) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(&As[buf][lrow * ST_LDK + kq * 4]) = ok0 ? ra0 : z;
        *reinterpret_cast<f32x4*>(&As[buf][(lrow + 32) * ST_LDK + kq * 4]) = ok1 ? ra1 : z;
        *reinterpret_cast<f32x4*>(&Bs[buf][lrow * ST_LDK + kq * 4]) = rb0;
        *reinterpret_cast<f32x4*>(&Bs[buf][(lrow + 32) * ST_LDK + kq * 4]) = rb1;
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int li = lane & 31, lh = lane >> 5;
    const int aidx = (wr * 32 + li) * ST_LDK + lh * (ST_BK / 2);
    const int bidx = (wc * 32 + li) * ST_LDK + lh * (ST_BK / 2);
    auto mma_tile = [&](int buf) {
#pragma unroll
        for (int c = 0; c < ST_BK / 8; ++c) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&As[buf][aidx + c * 4]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&Bs[buf][bidx + c * 4]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    };

    // two LDS buffers, one barrier per K tile: tile kt + 1 is loaded ahead of tile kt's MFMAs and stored behind them into the
    // other buffer, which everybody left before the previous barrier
    if (ka < kb) {
        gload(ka);
        lstore(0);
    }
    __syncthreads();
    for (int kt = ka; kt < kb; ++kt) {
        const int buf = (kt - ka) & 1;
        const bool more = kt + 1 < kb;
        if (more) gload(kt + 1);
        mma_tile(buf);
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }

    // epilogue: for a fixed accumulator register the 32 lanes of a half-wave hold 32 consecutive output channels
    const int co = n0 + wc * 32 + li;
    const float bias = (p.direct && p.bias) ? p.bias[co] : 0.f;
    float* out = p.out + ((long long)seg * p.frames_out + j) * (long long)(SS_NV * ST_C) + co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = acc[r];
        if (p.direct) {
            v = v + bias;
            v = fmaxf(v, 0.f);
        }
        if (m < SS_NV) out[m * ST_C] = v;
    }
}

// out[i] = relu(sum_s partial[s][i] + bias[co]), the partial sums added in the fixed order s = 0, 1, ...
__global__ __launch_bounds__(256) void st_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                        float* __restrict__ out, long long per, int nseg) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per) return;
    const float* part = partial + idx;
    float v = 0.f;
    for (int s0 = 0; s0 < nseg; s0 += 8) {               // eight loads in flight
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = s0 + k < nseg ? part[(long long)(s0 + k) * per] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (s0 + k < nseg) v += t[k];
    }
    if (bias) v += bias[idx & (ST_C - 1)];
    out[idx] = fmaxf(v, 0.f);
}

// One wave per compact row, the four neurons one after the other, each summed as linear_kernel sums it: lanes 0..31 carry four
// products each as one fma chain, the wave adds them with the xor butterfly, lane 0 adds the bias.
__global__ __launch_bounds__(256) void st_decode_kernel(const float* __restrict__ hid, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ delta, long long rows,
                                                        int first) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long j = row / SS_NV;
    const int v = (int)(row - j * SS_NV);
    long long win = 0;
    int f = (int)j;
    if (j >= ST_T) {
        const int cnt = ST_T - first;
        const long long q = (j - ST_T) / cnt;
        win = 1 + q;
        f = first + (int)((j - ST_T) - q * cnt);
    }
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < ST_C / 4) xv = reinterpret_cast<const float4*>(hid + row * ST_C)[lane];
    float* dst = delta + ((win * ST_T + f) * SS_NV + v) * 4;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float acc = 0.f;
        if (lane < ST_C / 4) {
            const float4 wv = reinterpret_cast<const float4*>(w + o * ST_C)[lane];
            acc = fmaf(wv.x, xv.x, acc);
            acc = fmaf(wv.y, xv.y, acc);
            acc = fmaf(wv.z, xv.z, acc);
            acc = fmaf(wv.w, xv.w, acc);
        }
        float s = ss_wave_sum(acc);
        if (lane == 0) {
            s += b ? b[o] : 0.f;
            dst[o] = s;
        }
    }
}

int st_status() { return hipGetLastError() == hipSuccess ? SST_OK : SST_ERR_LAUNCH; }

bool st_windows_ok(int nw, int first) { return nw > 0 && nw <= SST_MAX_WINDOWS && first >= 0 && first < ST_T; }

}  // namespace

extern "C" {

SST_API int sst_version(void) { return 1; }

SST_API long long sst_compact_frames(int nw, int first) {
    if (!st_windows_ok(nw, first)) return 0;
    return (long long)ST_T + (long long)(nw - 1) * (ST_T - first);
}

SST_API int sst_conv3d_layer(const float* in, const float* wgt, const float* bias, float* out, float* ws, long long ws_floats, int nw,
                             int first_in, int first_out, int seg_tiles, void* stream) {
    if (!in || !wgt || !out || !st_windows_ok(nw, first_in) || !st_windows_ok(nw, first_out) || first_out < first_in ||
        first_in > (first_out > 2 ? first_out - 2 : 0) || seg_tiles < 1 || seg_tiles > SST_K_TILES)
        return SST_ERR_ARG;
    const long long frames = sst_compact_frames(nw, first_out);
    const long long per = frames * SS_NV * ST_C;
    const int nseg = (SST_K_TILES + seg_tiles - 1) / seg_tiles;
    if (nseg > 1 && (!ws || ws_floats < (long long)nseg * per)) return SST_ERR_ARG;
    if (nseg > 65535) return SST_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    TailP p;
    p.in = in; p.wgt = wgt; p.bias = bias; p.out = nseg > 1 ? ws : out;
    p.first_in = first_in; p.first_out = first_out; p.frames_out = (int)frames;
    p.seg_tiles = seg_tiles; p.nseg = nseg; p.direct = nseg == 1;
    hipLaunchKernelGGL(st_conv3d_kernel, dim3((unsigned)frames, 2, (unsigned)nseg), dim3(256), 0, st, p);
    if (nseg > 1)
        hipLaunchKernelGGL(st_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, ws, bias, out, per, nseg);
    return st_status();
}

SST_API int sst_decode_scatter(const float* hid, const float* w, const float* b, float* delta, int nw, int first, void* stream) {
    if (!hid || !w || !delta || !st_windows_ok(nw, first)) return SST_ERR_ARG;
    const long long rows = sst_compact_frames(nw, first) * SS_NV;
    hipLaunchKernelGGL(st_decode_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, hid, w, b, delta, rows,
                       first);
    return st_status();
}

}  // extern "C"
