// Correlation kernels: local cost volume (K8) and the contextual correlation layer (K3).
#include "common.h"

extern "C" int ss_conv_nhwc(const float*, const float*, const float*, const float*, float*, int, int, int, int, int,
                            int, int, int, int, int, int, int, int, int, int, int, long long, long long, long long,
                            float*, long long, void*);

// ------------------------------------------------------------------------------------------------
// cost volume.  Block = 4x16 output pixels of one image; channels walked in chunks of 16 staged channel-major in
// LDS (x2 window incl. halo, row pitch padded to a multiple of 4 floats, + x1 tile).  Thread = (4 adjacent pixels,
// one displacement row j): per channel it reads 4 x1 values and the 4+2R contiguous x2 values of window row py+j as
// 16-byte LDS reads and updates its 4 x (2R+1) accumulators -- 0.4 LDS dwords per FMA instead of 1 for the naive
// (pixel, displacement) mapping.  Results go back through LDS for coalesced NHWC stores.
#define CV_TX 16
#define CV_DEFAULT_TY 4
#define CV_CC 16

// CV_TY = tile height: 4 (round 1-3) or 8 (round 4: the window a workgroup stages is (TY + 2R) x (16 + 2R) pixels for TY x 16
// outputs -- 5.7 window pixels per output pixel at TY = 4, R = 5, 3.7 at TY = 8; the kernel's staging reads come from L2 /
// MALL at ~6 TB/s, which is what bounded it, not the LDS and not the FMAs).
template <int R, int CV_TY>
__global__ __launch_bounds__(64 * ((4 * CV_TY * (2 * R + 1) + 63) / 64)) void cost_volume_kernel(
    const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ out, int h, int w, int c,
    int out_cs, int n_fwd, int n_img, int tiles_x, int tiles_y, int split, int shift, int group) {
    constexpr int KD = 2 * R + 1;
    constexpr int D = KD * KD;
    constexpr int PG = 4 * CV_TY;                      // threads per displacement row: CV_TY rows x 4 pixel quads
    constexpr int NT = 64 * ((PG * KD + 63) / 64);      // threads per block (TY 4: 176 -> 192, 112 -> 128; TY 8: 352 -> 384, 224 -> 256)
    constexpr int WH = CV_TY + 2 * R;
    // LDS layout of one channel plane of the x2 window (rows of 26 / 22 floats = 7 / 6 slots of 16 bytes).  A ds_read_b128 is
    // served 16 lanes at a time (MI355X_MICROARCH.md, LDS: groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) over the 16 slots
    // of a 256-byte bank row; with this kernel's lane map a group holds the chunks g .. g+3 of THREE window rows -- r, r+2, r+3 or
    // r+1, r+2, r+4 (the fourth quad of lanes repeats one of them: a broadcast).  Under a plain row pitch of 28 / 24 floats two of
    // those rows overlapped in two slots: every read took two LDS cycles (rocprofv3 r03: 0.42 of the kernel's LDS cycles were
    // bank-conflict stalls).  Here row r starts at bank slot 4 r mod 16, so rows one, two and three apart are 4, 8 and 12 slots
    // apart and a group's three 4-slot runs never meet; storage stays compact because rows r and r + 2 share one 16-slot line
    // (slots 4r .. 4r+6 and 4r+8 .. 4r+14): line(r) = 2 (r >> 2) + (r & 1), address = 64 line + 4 ((4 r + chunk) & 15) floats.
    constexpr int WLINES = 2 * ((WH + 3) / 4);
    static_assert(CV_TX + 2 * R <= 28, "a window row must fit 7 slots");
    constexpr int WPIX = WLINES * 64;
    constexpr int NV = 4 + 2 * R;                       // x2 values per thread per channel (14 / 10)
    constexpr int OUTF = 4 * CV_TX * (D + 3);           // staging for the epilogue (four tile rows at a time)
    // Channel planes in groups of four (one staged item = the 4 channels of a pixel, written by one lane in four instructions):
    // the plane pitches (392 / 240 / 64 floats) are multiples of 8, so the four lanes that hold the four channel quads of one
    // pixel would hit ONE bank in every staging write (rocprofv3: 59 % of the kernel's LDS cycles were bank-conflict stalls, the
    // LDS busy 63 % of the time).  Eight floats of skew per quad put them 8 banks apart: a half-wave's 8 pixels x 4 quads cover
    // the 32 banks once.  (Multiples of 4: the 16-byte reads stay aligned.)
    constexpr int QP2 = 4 * WPIX + 8, QP1 = 4 * CV_TY * CV_TX + 8;         // quad pitches of the x2 window / the x1 tile
    constexpr int X2F = (CV_CC / 4) * QP2;
    constexpr int LDSF = (X2F > OUTF ? X2F : OUTF);
    __shared__ __attribute__((aligned(16))) float s2[LDSF];
    __shared__ __attribute__((aligned(16))) float s1f[(CV_CC / 4) * QP1];

    const int tid = threadIdx.x;
    // image n < n_fwd: cv(x1, x2) of image n; >= n_fwd: the OTHER direction cv(x2, x1) of image n - n_fwd, written behind the
    // n_fwd forward volumes (both directions of SpatialNet's stage 2, spatial_network.py:318,325, in one launch: 2 x 1536 workgroups
    // are exactly three rounds of the chip where two launches of 1.5 rounds each cost four)
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  In the natural order the
    // neighbouring tiles of an image -- which share most of their 14 x 26-pixel windows (5.7 window pixels are staged per
    // output pixel) -- land on eight different L2s and every halo is fetched again from the MALL; here XCD k walks one
    // contiguous eighth of the tile list, so a tile's neighbours are the same L2's recent work.
    const int total = tiles_x * tiles_y * n_img;
    const int per = (total + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per || tile >= total) return;
    const int bx = tile % tiles_x, by = (tile / tiles_x) % tiles_y;
    int n = tile / (tiles_x * tiles_y);
    if (n >= n_fwd) {
        const float* t = x1; x1 = x2; x2 = t;
        out += (long long)n_fwd * h * w * out_cs;
        n -= n_fwd;
    }
    const int y0 = by * CV_TY, x0 = bx * CV_TX;
    const bool active = tid < PG * KD;
    const int pg = tid & (PG - 1), j = active ? tid / PG : 0;   // pixel group (py, 4g) and displacement row
    const int py = pg >> 2, g4 = (pg & 3) * 4;
    // (Eight lanes of a 16-byte read = the four g4 of two ADJACENT window rows.  Round 3 tried a lane map that pairs rows half a
    // bank cycle apart -- 256 threads with 80 idle lanes at R = 5: slower.  Round 4 rotates the odd rows' chunks instead, above.)
    // volume n reads image n + n / group + (n >= split ? shift : 0) of both inputs (a chain of pairs stores every view once:
    // ss_cost_volume_shifted, group >= n; k frames of every view of a chain: ss_cost_volume_chain_frames, group = k).  n is uniform
    // over the workgroup: the division is scalar, once per workgroup.
    const int ni = n + n / group + (n >= split ? shift : 0);
    const float* x1n = x1 + (long long)ni * h * w * c;
    const float* x2n = x2 + (long long)ni * h * w * c;

    // accumulators as PAIRS for v_pk_fma_f32 (two fp32 FMAs per issue slot).  acc(p, i) += a[p] * v[p + i]: the window values
    // arrive as aligned register pairs (v[2t], v[2t+1]), so pixel p pairs its displacements (i, i + 1) with p + i EVEN -- even p:
    // (0,1) .. (KD-3, KD-2), left over i = KD - 1; odd p: (1,2) .. (KD-2, KD-1), left over i = 0 -- and a[p] is broadcast by
    // op_sel: no register moves (the first packed version paired (2t, 2t+1) for every p and the compiler spent 26 v_mov per 44
    // packed FMAs re-aligning the odd pixels' operands).  Each accumulator still receives its products in channel order.
    typedef float cv_f2 __attribute__((ext_vector_type(2)));
    constexpr int KP = KD / 2;
    cv_f2 accp[4][KP];
    float accs[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
        for (int i = 0; i < KP; ++i) accp[p][i] = (cv_f2){0.f, 0.f};
        accs[p] = 0.f;
    }

    // staging items of this thread (fixed over the channel loop): x2 window [row][col][quad], x1 tile [pixel][quad];
    // element offset of channel 0 of the quad, or -1 outside the image.  The loads of chunk c0 + 16 are issued into
    // registers BEFORE the FMAs of chunk c0 (the kernel runs in a single round of ~6 workgroups per CU: without the
    // prefetch every chunk paid a full global-memory latency between its two barriers: 134 -> 7x us for 32 pairs at R = 5).
    constexpr int N2 = (WH * (CV_TX + 2 * R) * (CV_CC / 4) + NT - 1) / NT;
    constexpr int N1 = (CV_TY * CV_TX * (CV_CC / 4) + NT - 1) / NT;
    static_assert(NT % 4 == 0, "channel quad of an item = tid & 3");
    int o2[N2], o1[N1];               // element offsets inside one image (< 2^31), -1 = outside
    int l2[N2], l1[N1];
    const int myq4 = (tid & 3) * 4;
#pragma unroll
    for (int k = 0; k < N2; ++k) {
        const int e = tid + k * NT;
        const int q = e % (CV_CC / 4), wp = e / (CV_CC / 4);
        const int wy = wp / (CV_TX + 2 * R), wx = wp - wy * (CV_TX + 2 * R);
        const int yy = y0 - R + wy, xx = x0 - R + wx;
        const bool in = e < WH * (CV_TX + 2 * R) * (CV_CC / 4);
        o2[k] = (in && (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) ? (yy * w + xx) * c + q * 4 : -1;
        l2[k] = in ? q * QP2 + (2 * (wy >> 2) + (wy & 1)) * 64 + (((4 * wy + (wx >> 2)) & 15) << 2) + (wx & 3) : -1;
    }
#pragma unroll
    for (int k = 0; k < N1; ++k) {
        const int e = tid + k * NT;
        const int q = e % (CV_CC / 4), pp = e / (CV_CC / 4);
        const int yy = y0 + (pp >> 4), xx = x0 + (pp & 15);
        const bool in = e < CV_TY * CV_TX * (CV_CC / 4);
        o1[k] = (in && yy < h && xx < w) ? (yy * w + xx) * c + q * 4 : -1;
        l1[k] = in ? q * QP1 + pp : -1;
    }
    // the thread's window row py + j: float offsets of its chunks g .. g + 3
    int roff[(NV + 3) / 4];
    {
        const int wr = py + j;
#pragma unroll
        for (int q = 0; q < (NV + 3) / 4; ++q) roff[q] = (2 * (wr >> 2) + (wr & 1)) * 64 + (((4 * wr + (g4 >> 2) + q) & 15) << 2);
    }
    float4 r2[N2], r1[N1];
    auto fetch = [&](int c0) {
        const bool cok = c0 + myq4 < c;
#pragma unroll
        for (int k = 0; k < N2; ++k) {
            // branch free: an invalid item reads element 0 of the image (always mapped) and is zeroed by a select -- with an
            // `if` around every load the compiler emitted ten exec-mask branches per chunk
            const bool ok = o2[k] >= 0 && cok;
            const float4 t = *reinterpret_cast<const float4*>(x2n + (ok ? o2[k] + c0 : 0));
            r2[k] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < N1; ++k) {
            const bool ok = o1[k] >= 0 && cok;
            const float4 t = *reinterpret_cast<const float4*>(x1n + (ok ? o1[k] + c0 : 0));
            r1[k] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < c; c0 += CV_CC) {
        // registers -> LDS, channel-major
#pragma unroll
        for (int k = 0; k < N2; ++k)
            if (l2[k] >= 0) {
                s2[l2[k]] = r2[k].x; s2[l2[k] + WPIX] = r2[k].y; s2[l2[k] + 2 * WPIX] = r2[k].z; s2[l2[k] + 3 * WPIX] = r2[k].w;
            }
#pragma unroll
        for (int k = 0; k < N1; ++k)
            if (l1[k] >= 0) {
                s1f[l1[k]] = r1[k].x; s1f[l1[k] + CV_TY * CV_TX] = r1[k].y; s1f[l1[k] + 2 * CV_TY * CV_TX] = r1[k].z;
                s1f[l1[k] + 3 * CV_TY * CV_TX] = r1[k].w;
            }
        __syncthreads();
        if (c0 + CV_CC < c) fetch(c0 + CV_CC);
        if (active) {
#pragma unroll 4
            for (int cc = 0; cc < CV_CC; ++cc) {      // (fully unrolled the kernel needs 204-230 registers: two waves per SIMD)
                const float4 a4 = *reinterpret_cast<const float4*>(&s1f[(cc >> 2) * QP1 + (cc & 3) * (CV_TY * CV_TX) + py * 16 + g4]);
                const float a[4] = {a4.x, a4.y, a4.z, a4.w};
                const float* row = s2 + (cc >> 2) * QP2 + (cc & 3) * WPIX;
                float v[NV];
#pragma unroll
                for (int q = 0; q < NV / 4; ++q) {
                    float4 t = *reinterpret_cast<const float4*>(row + roff[q]);
                    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
                }
                if (NV % 4) {
                    // the last two values as a full 16-byte read too (the row's 7th slot exists: 26 floats live in 7 slots of 4): an
                    // 8-byte read is served in 32-lane groups, where this kernel's lane map puts two window rows on the same banks;
                    // the 16-byte groups were laid out conflict-free above.  (The opaque asm keeps hipcc from shortening it again.)
                    typedef float cv_f4 __attribute__((ext_vector_type(4)));
                    cv_f4 t = *reinterpret_cast<const cv_f4*>(row + roff[NV / 4]);
                    asm volatile("" : "+v"(t));
                    v[NV - 2] = t[0]; v[NV - 1] = t[1];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const cv_f2 ap = {a[p], a[p]};
                    const int o = p + (p & 1);                    // first v index of the pixel's pairs (even)
#pragma unroll
                    for (int i = 0; i < KP; ++i)
                        accp[p][i] = __builtin_elementwise_fma(ap, (cv_f2){v[o + 2 * i], v[o + 2 * i + 1]}, accp[p][i]);
                    accs[p] = fmaf(a[p], (p & 1) ? v[p] : v[p + KD - 1], accs[p]);
                }
            }
        }
        __syncthreads();
    }
    // epilogue through LDS: [pixel][D+3], four tile rows per pass
    const float fc = (float)c;
#pragma unroll
    for (int half = 0; half < CV_TY / 4; ++half) {
        if (half) __syncthreads();
        if (active && (py >> 2) == half) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int i = 0; i < KD; ++i) {
                    const int ii = i - (p & 1);                 // position in the pixel's pair list (odd pixels start at i = 1)
                    const float av = (ii < 0 || ii >= 2 * KP) ? accs[p] : ((ii & 1) ? accp[p][ii >> 1].y : accp[p][ii >> 1].x);
                    float v = av / fc;
                    s2[((py & 3) * 16 + g4 + p) * (D + 3) + j * KD + i] = v > 0.f ? v : 0.1f * v;
                }
        }
        __syncthreads();
        if (out_cs == D + 3) {
            // the usual layout (channels padded to a multiple of 4 = the staging pitch): 16-byte stores, compile-time divisor.
            // (The generic loop below divides by the RUNTIME out_cs twice per 4-byte store, 41 times per thread: ~2000 integer
            // instructions beside the 7000 of the channel loop -- a quarter of the kernel, found in round 4 after the LDS
            // conflicts, the FMA count, the occupancy and the tile order had each turned out not to be the limiter.)
            constexpr int Q = (D + 3) / 4;
            for (int e = tid; e < 4 * CV_TX * Q; e += NT) {
                const int p = e / Q, q = e - p * Q;
                const int yy = y0 + half * 4 + (p >> 4), xx = x0 + (p & 15);
                if (yy < h && xx < w) {
                    float4 v = *reinterpret_cast<const float4*>(&s2[p * (D + 3) + 4 * q]);
                    if (4 * q + 1 >= D) v.y = 0.f;
                    if (4 * q + 2 >= D) v.z = 0.f;
                    if (4 * q + 3 >= D) v.w = 0.f;
                    *reinterpret_cast<float4*>(&out[(((long long)n * h + yy) * w + xx) * (D + 3) + 4 * q]) = v;
                }
            }
        } else {
            for (int e = tid; e < 4 * CV_TX * out_cs; e += NT) {
                int ch = e % out_cs;
                int p = e / out_cs;
                int yy = y0 + half * 4 + (p >> 4), xx = x0 + (p & 15);
                if (yy < h && xx < w)
                    out[(((long long)n * h + yy) * w + xx) * out_cs + ch] = ch < D ? s2[p * (D + 3) + ch] : 0.f;
            }
        }
    }
}

// tile height (process-wide A/B knob; 0 = the library's rule)
static int g_cv_ty = 0;
extern "C" int ss_cost_volume_set_tile(int ty) {
    if (ty != 0 && ty != 4 && ty != 8) return SS_ERR_ARG;
    g_cv_ty = ty;
    return SS_OK;
}

static int cv_launch(const float* x1, const float* x2, float* out, int n_fwd, int n_img, int h, int w, int c, int r, int out_cs,
                     hipStream_t st, int split = 1 << 30, int shift = 0, int group = 1 << 30) {
    if (r != 5 && r != 3) return SS_ERR_UNSUPPORTED;
    // measured (tools/bench_cv.py, 32 / 62 pairs): R = 5: 93-106 us at TY 4, 119-128 at TY 8; R = 3: 91 at TY 4, 79 at TY 8
    const int TY = g_cv_ty ? g_cv_ty : (r == 3 ? 8 : CV_DEFAULT_TY);
    const int tx = ss_cdiv(w, CV_TX), ty = ss_cdiv(h, TY);
    if ((long long)tx * ty * n_img > (1ll << 30)) return SS_ERR_UNSUPPORTED;
    dim3 g(8 * ss_cdiv((long long)tx * ty * n_img, 8));
    if (TY == 8) {
        if (r == 5) hipLaunchKernelGGL((cost_volume_kernel<5, 8>), g, dim3(384), 0, st, x1, x2, out, h, w, c, out_cs, n_fwd, n_img, tx, ty, split, shift, group);
        else hipLaunchKernelGGL((cost_volume_kernel<3, 8>), g, dim3(256), 0, st, x1, x2, out, h, w, c, out_cs, n_fwd, n_img, tx, ty, split, shift, group);
    } else {
        if (r == 5) hipLaunchKernelGGL((cost_volume_kernel<5, 4>), g, dim3(192), 0, st, x1, x2, out, h, w, c, out_cs, n_fwd, n_img, tx, ty, split, shift, group);
        else hipLaunchKernelGGL((cost_volume_kernel<3, 4>), g, dim3(128), 0, st, x1, x2, out, h, w, c, out_cs, n_fwd, n_img, tx, ty, split, shift, group);
    }
    return ss_launch_status();
}

extern "C" int ss_cost_volume(const float* x1, const float* x2, float* out, int n, int h, int w, int c, int r,
                              int out_cs, void* stream) {
    if (!x1 || !x2 || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3)) return SS_ERR_ARG;
    int D = (2 * r + 1) * (2 * r + 1);
    if (out_cs < D) return SS_ERR_ARG;
    return cv_launch(x1, x2, out, n, n, h, w, c, r, out_cs, (hipStream_t)stream);
}

// n volumes over inputs that hold every image ONCE: volume b = cv(x1[i], x2[i]) with i = b + (b >= split ? shift : 0).  A chain of S
// pairs (view s, view s + 1) keeps its S + 1 views' TemporalNet features once and asks for the 2 S volumes [first views | second
// views] with split = S, shift = 1 - S (temporal_network.py:120-147 per view; no concatenated copy of the features).
extern "C" int ss_cost_volume_shifted(const float* x1, const float* x2, float* out, int n, int h, int w, int c, int r, int out_cs,
                                      int split, int shift, void* stream) {
    if (!x1 || !x2 || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3) || split < 0 || split + shift < 0) return SS_ERR_ARG;
    int D = (2 * r + 1) * (2 * r + 1);
    if (out_cs < D) return SS_ERR_ARG;
    return cv_launch(x1, x2, out, n, n, h, w, c, r, out_cs, (hipStream_t)stream, split, shift);
}

// The temporal cost volumes of a chain of `views` views over k consecutive frames in ONE launch, from features stored once:
// x [views][k + 1][h][w][c] (slot 0 = each view's previous frame) -> out [2][views - 1][k] volumes [first views | second views] of
// the views - 1 pairs, pair-major, frame-minor: volume (hh, s, j) = cv(x[s + hh][j], x[s + hh][j + 1]) (temporal_network.py:120-174
// per view and frame).  Volume b = (hh (views - 1) + s) k + j reads image (s + hh)(k + 1) + j of x and the image after it:
// b + b / k + (b >= (views - 1) k ? (2 - views)(k + 1) : 0).  Per volume the kernel body of ss_cost_volume.
extern "C" int ss_cost_volume_chain_frames(const float* x, float* out, int views, int k, int h, int w, int c, int r, int out_cs,
                                           void* stream) {
    if (!x || !out || views < 2 || k < 1 || k > 32 || h <= 0 || w <= 0 || c <= 0 || (c & 3)) return SS_ERR_ARG;
    if (r != 3 && r != 5) return SS_ERR_ARG;
    const int D = (2 * r + 1) * (2 * r + 1);
    if (out_cs < D) return SS_ERR_ARG;
    // grid: one workgroup per 16-column tile of (at least) 4 rows of every volume; 32-bit volume indices and offsets in an image
    const long long n = 2ll * (views - 1) * k;
    if ((long long)views * (k + 1) > (1ll << 24) || (long long)h * w * c >= (1ll << 31) ||
        (long long)ss_cdiv(w, CV_TX) * ss_cdiv(h, CV_DEFAULT_TY) * n > (1ll << 30))
        return SS_ERR_ARG;
    const int pairs = views - 1;
    return cv_launch(x, x + (long long)h * w * c, out, (int)n, (int)n, h, w, c, r, out_cs, (hipStream_t)stream, pairs * k,
                     (1 - pairs) * (k + 1), k);
}

// both directions in ONE launch: out [2][n][h][w][out_cs] = cv(x1, x2), cv(x2, x1)
extern "C" int ss_cost_volume_bidir(const float* x1, const float* x2, float* out, int n, int h, int w, int c, int r,
                                    int out_cs, void* stream) {
    if (!x1 || !x2 || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3) || 2 * n > 65535) return SS_ERR_ARG;
    int D = (2 * r + 1) * (2 * r + 1);
    if (out_cs < D) return SS_ERR_ARG;
    return cv_launch(x1, x2, out, n, 2 * n, h, w, c, r, out_cs, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// CCL = L2 normalise -> per-pixel Gram D[p][k] = <n1[p], n2[k]> (fp32 MFMA, 1x1 conv with n2 as the
// filter bank) -> 3x3 patch correlation as 9 shifted sums of D -> softmax(10 x) over k -> expected shift.
// (the reference convolves with 690 3x3x256 filters, 2.19 GFLOP; the shifted-sum identity needs 0.24.)
__global__ void l2norm_kernel(const float* __restrict__ in, float* __restrict__ out, long long npix, int c) {
    long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (pix >= npix) return;
    const float* p = in + pix * c;
    float ss = 0.f;
    for (int i = lane; i < c; i += 64) ss = fmaf(p[i], p[i], ss);
    ss = ss_wave_sum(ss);
    float d = fmaxf(sqrtf(ss), 1e-12f);
    for (int i = lane; i < c; i += 64) out[pix * c + i] = p[i] / d;
}

extern "C" int ss_l2norm_nhwc(const float* in, float* out, long long n_pixels, int c, void* stream) {
    if (!in || !out || n_pixels <= 0 || c <= 0) return SS_ERR_ARG;
    hipLaunchKernelGGL(l2norm_kernel, dim3(ss_cdiv(n_pixels, 4)), dim3(256), 0, (hipStream_t)stream, in, out, n_pixels, c);
    return ss_launch_status();
}

// one wave per query position p; a lane owns 4 consecutive k (k = 256 * cnt + 4 * lane + j), so a tap of the 3 x 3 patch
// correlation is ONE 16-byte load per lane (only 4-byte aligned: the tap shifts the column by dy * w + dx) and a wave reads
// a row of D in 1 KB pieces: 27 loads per lane where the scalar mapping had 108.
struct __attribute__((packed, aligned(4))) CclF4 { float v[4]; };

__global__ void ccl_softmax_kernel(const float* __restrict__ Dm, float* __restrict__ flow_nchw,
                                   float* __restrict__ flow_nhwc4, int h, int w, float scale, SsFastDiv divW) {
    const int P = h * w;
    int n = blockIdx.y;
    int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (p >= P) return;
    const float* Db = Dm + (long long)n * P * P;
    int py = (int)ss_fastdiv((uint32_t)p, divW), pxx = p - py * w;      // (k / w by multiply-shift)
    float g[12];   // P <= 768
    int gy[12], gx[12];
    float mx = -INFINITY;
#pragma unroll
    for (int cnt = 0; cnt < 3; ++cnt) {
        const int k0 = 256 * cnt + 4 * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[4 * cnt + j] = -INFINITY;
            gy[4 * cnt + j] = gx[4 * cnt + j] = 0;
        }
        if (256 * cnt >= P) continue;                                   // wave uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = min(k0 + j, P - 1);
            gy[4 * cnt + j] = (int)ss_fastdiv((uint32_t)k, divW);
            gx[4 * cnt + j] = k - gy[4 * cnt + j] * w;
        }
        // the nine taps, branch free: all nine loads are issued before the first add (with an `if` around each the compiler
        // serialised load -> wait -> add: one L2 round trip per tap).  A tap whose query pixel is outside the image reads
        // entry 0; one whose column leaves [0, P) reads the neighbouring row (or the slack ss_ccl_workspace_floats adds
        // after the last one); the per-element select drops both.  Same order of the adds as the per-tap form.
        CclF4 tv[9];
        bool qok[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            const int qy = py + dy, qx = pxx + dx;
            qok[t] = (unsigned)qy < (unsigned)h && (unsigned)qx < (unsigned)w && k0 < P;
            const long long at = qok[t] ? (long long)(qy * w + qx) * P + (k0 + dy * w + dx) : 0ll;
            tv[t] = *reinterpret_cast<const CclF4*>(Db + at);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ky = gy[4 * cnt + j], kx = gx[4 * cnt + j];
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dy = t / 3 - 1, dx = t % 3 - 1;
                const bool ok = qok[t] && (unsigned)(ky + dy) < (unsigned)h && (unsigned)(kx + dx) < (unsigned)w;
                s += ok ? tv[t].v[j] : 0.f;
            }
            s = k0 + j < P ? s * scale : -INFINITY;
            g[4 * cnt + j] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = ss_wave_max(mx);
    float se = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        float e = expf(g[i] - mx);                                       // exp(-inf) = 0 past P
        se += e;
        sx = fmaf(e, (float)(gx[i] - pxx), sx);
        sy = fmaf(e, (float)(gy[i] - py), sy);
    }
    se = ss_wave_sum(se); sx = ss_wave_sum(sx); sy = ss_wave_sum(sy);
    if (lane == 0) {
        float fx = sx / se, fy = sy / se;
        if (flow_nchw) {
            flow_nchw[((long long)n * 2 + 0) * P + p] = fx;
            flow_nchw[((long long)n * 2 + 1) * P + p] = fy;
        }
        if (flow_nhwc4)
            *reinterpret_cast<float4*>(flow_nhwc4 + ((long long)n * P + p) * 4) = make_float4(fx, fy, 0.f, 0.f);
    }
}

extern "C" long long ss_ccl_workspace_floats(int n, int h, int w, int c) {
    long long P = (long long)h * w;
    // + slack: the softmax reads D in 16-byte pieces at shifted columns, up to w + 4 floats past the last row's end (the tap one
    // row down of the last 4-column piece); 64 covered maps up to 60 columns wide, all the pipeline has
    return (long long)n * P * (2ll * c + P) + (w + 8 > 64 ? w + 8 : 64);
}

extern "C" int ss_ccl(const float* f1, const float* f2, float* flow_nchw, float* flow_nhwc4, int n, int h, int w,
                      int c, float softmax_scale, float* ws, void* stream) {
    if (!f1 || !f2 || !ws || (!flow_nchw && !flow_nhwc4) || n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3))
        return SS_ERR_ARG;
    int P = h * w;
    if (P > 768) return SS_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    float* n1 = ws;
    float* n2 = n1 + (long long)n * P * c;
    float* Dm = n2 + (long long)n * P * c;
    long long npix = (long long)n * P;
    const long long gap = f2 - f1, img = (long long)P * c;
    if (gap == npix * c) {
        // the two views' maps are the halves of one tensor (SpatialNet's trunk output, view 1 first) and n1 / n2 are adjacent in
        // the workspace: one launch normalises both (a batch-1 push pays per launch)
        hipLaunchKernelGGL(l2norm_kernel, dim3(ss_cdiv(2 * npix, 4)), dim3(256), 0, st, f1, n1, 2 * npix, c);
    } else if (gap > 0 && gap < npix * c && gap % img == 0) {
        // the batches OVERLAP (a chain of pairs: f1 = views [0:n], f2 = views [k:k+n] of one tensor): every view once, one launch
        const long long k = gap / img;
        hipLaunchKernelGGL(l2norm_kernel, dim3(ss_cdiv((n + k) * (long long)P, 4)), dim3(256), 0, st, f1, n1, (n + k) * (long long)P, c);
        n2 = n1 + gap;
    } else {
        hipLaunchKernelGGL(l2norm_kernel, dim3(ss_cdiv(npix, 4)), dim3(256), 0, st, f1, n1, npix, c);
        hipLaunchKernelGGL(l2norm_kernel, dim3(ss_cdiv(npix, 4)), dim3(256), 0, st, f2, n2, npix, c);
    }
    int rc = ss_launch_status();
    if (rc) return rc;
    // D[p][k] = sum_c n1[p][c] n2[k][c]: "image" = n1 as a 1 x P strip, "filters" = n2 rows, one group per batch item
    rc = ss_conv_nhwc(n1, n2, nullptr, nullptr, Dm, 1, 1, 1, P, c, P, 1, 1, 1, 1, 0, 0, 0, 0, P, n, (long long)P * c,
                      (long long)P * c, (long long)P * P, nullptr, 0, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(ccl_softmax_kernel, dim3(ss_cdiv(P, 4), n), dim3(256), 0, st, (const float*)Dm, flow_nchw,
                       flow_nhwc4, h, w, softmax_scale, ss_fastdiv_make((uint32_t)w));
    return ss_launch_status();
}
