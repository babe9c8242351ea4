// libstabstitch_seam.so: the dynamic-programming seam of MULTIBAND fusion (include/stabstitch_seam.h).  gfx950 only.
//
// Three launches per call, frames in the grid of the first and the last:
//   cost    every pair's (D, nb, E) per cell, and per workgroup the rows of cells with overlap and the views' column extents: one pass over P
//   dp      one workgroup per seam: sorts the views from the extents, walks the call's frames in order (it carries xprev), keeps the two
//           live rows of M and the 2-bit back pointers in LDS, and backtracks there
//   paint   plane 3 of every view from the seams
// Everything after the per-pixel cost is integer arithmetic; the sums are integer atomics in LDS: no result depends on their order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/stabstitch_seam.h"

namespace {

#define SM_PEN (1 << 19)             // a cell without overlap in a row that has some
#define SM_TCAP (1 << 18)            // cap of the temporal term
#define SM_MCAP (1 << 30)            // cap of M
#define SM_RED 16                    // ints in front of the dp's LDS: extents (6), the end point (2 = one u64)

struct SmPlan {
    int V, NP, c, shift, hq, wq, wq4, th, gx, gy, nblk;
    long long cost, ext, seams, meta, rowf, ints;    // offsets (ints) and the total
};

inline int sm_cdiv(int a, int b) { return (a + b - 1) / b; }

// false: arguments the library refuses
bool sm_plan(int frames, int views, int hc, int wc, int cell, SmPlan* p) {
    if (frames < 1 || frames > 65535 || views < 2 || views > SSM_MAX_VIEWS) return false;
    if (hc < 1 || wc < 1 || hc > 32768 || wc > 32768) return false;
    int shift = -1;
    for (int s = 0; s <= 4; ++s) if (cell == (1 << s)) shift = s;
    if (shift < 0) return false;
    p->V = views; p->NP = views * (views - 1) / 2; p->c = cell; p->shift = shift;
    p->hq = sm_cdiv(hc, cell); p->wq = sm_cdiv(wc, cell); p->wq4 = (p->wq + 3) & ~3;
    const long long lds = 4LL * (SM_RED + 2 * p->wq4 + 3 * p->hq) + (long long)p->hq * p->wq4 / 4;
    if (lds > SSM_LDS_BYTES) return false;
    p->th = cell > 4 ? cell : 4;
    p->gx = sm_cdiv(wc, SSM_TILE_W); p->gy = sm_cdiv(hc, p->th); p->nblk = p->gx * p->gy;
    if (p->gy > 65535) return false;
    const long long cells = (long long)p->hq * p->wq4;
    long long off = 0;
    p->cost = off; off += (long long)frames * p->NP * 3 * cells;
    p->ext = off; off += (long long)frames * p->nblk * views * 2;
    p->seams = off; off += (long long)frames * (views - 1) * p->hq;
    p->meta = off; off += (long long)frames * 8;
    p->rowf = off; off += (long long)frames * p->NP * p->hq * p->gx;
    p->ints = off;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// cost: one workgroup = SSM_TILE_W columns x max(4, cell) rows of one frame, whole cells only (the tile is a multiple of every cell size
// both ways); one thread = an aligned quad of four columns, one wave = a row.  A quad whose 16 bytes are aligned and inside the row is one
// load, any other is four scalar loads (columns past the row read as invalid).

// four values of one plane row at element index e of P (x: their first column)
__device__ __forceinline__ float4 sm_ld4(const float* __restrict__ P, size_t e, bool al4, int x, int wc) {
    if (al4 && ((e & 3) == 0) && x + 3 < wc) return *reinterpret_cast<const float4*>(P + e);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x < wc) v.x = P[e];
    if (x + 1 < wc) v.y = P[e + 1];
    if (x + 2 < wc) v.z = P[e + 2];
    if (x + 3 < wc) v.w = P[e + 3];
    return v;
}

__device__ __forceinline__ float sm_at(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// the pixel cost of a pair: fp32, one rounding per operation (the build has -ffp-contract=off), truncations
__device__ __forceinline__ int sm_pixel_cost(float ba, float ga, float ra, float oa, float bb, float gb, float rb, float ob, float prior) {
    const float dc = (fabsf(ba - bb) + fabsf(ga - gb)) + fabsf(ra - rb);
    const float s = oa + ob;
    const float t = s > 0.f ? fabsf(oa - ob) / s : 0.f;
    return min(765, (int)dc) + (int)(prior * t);
}

template <int V>
__global__ __launch_bounds__(256) void sm_cost_kernel(const float* __restrict__ P, int* __restrict__ cost, int* __restrict__ ext,
                                                      int* __restrict__ rowf, int hc, int wc, int shift, int th, int hq, int wq, float prior) {
    const int wq4 = (wq + 3) & ~3;
    constexpr int NP = V * (V - 1) / 2;
    __shared__ int acc[6 * 1024];            // [NP][2][ch][cw]: at most 3 x 2 x 1024 cells (cell 1)
    __shared__ int ex[2 * V];
    __shared__ int rf[NP * 4];              // [NP][ch]: does the tile hold an overlap cell in this row of cells?
    const int cw = SSM_TILE_W >> shift, ch = th >> shift, cells = cw * ch;
    for (int i = threadIdx.x; i < NP * 2 * cells; i += 256) acc[i] = 0;
    if (threadIdx.x < 2 * V) ex[threadIdx.x] = (threadIdx.x & 1) ? -1 : INT_MAX;
    if (threadIdx.x < NP * 4) rf[threadIdx.x] = 0;
    __syncthreads();
    const int x0 = blockIdx.x * SSM_TILE_W, y0 = blockIdx.y * th;
    const int q = threadIdx.x & 63, x = x0 + 4 * q;
    const size_t plane = (size_t)hc * wc;
    const size_t ebase = (size_t)blockIdx.z * (V * 5) * plane;       // element index of this frame in P
    const bool al4 = (reinterpret_cast<uintptr_t>(P) & 15) == 0;
    int xmin[V], xmax[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { xmin[v] = INT_MAX; xmax[v] = -1; }
    for (int r = threadIdx.x >> 6; r < th; r += 4) {
        const int y = y0 + r;
        if (y >= hc || x >= wc) continue;
        float4 pl[V][5];
#pragma unroll
        for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const size_t e = (size_t)(v * 5 + k) * plane + (size_t)y * wc + x;
                pl[v][k] = sm_ld4(P, ebase + e, al4, x, wc);
            }
        }
        const int lcy = r >> shift;
        int cur = -1, sd[NP], sn[NP];
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) { sd[pr] = 0; sn[pr] = 0; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool valid[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                valid[v] = x + i < wc && sm_at(pl[v][4], i) >= 0.5f;
                if (valid[v]) { xmin[v] = min(xmin[v], x + i); xmax[v] = max(xmax[v], x + i); }
            }
            const int lcx = (4 * q + i) >> shift;
            if (lcx != cur) {                                     // the quad enters another cell (cells below 4 pixels): flush
                if (cur >= 0) {
#pragma unroll
                    for (int pr = 0; pr < NP; ++pr) {
                        if (sn[pr]) {
                            atomicAdd(&acc[((pr * 2 + 0) * ch + lcy) * cw + cur], sd[pr]);
                            atomicAdd(&acc[((pr * 2 + 1) * ch + lcy) * cw + cur], sn[pr]);
                        }
                        sd[pr] = 0; sn[pr] = 0;
                    }
                }
                cur = lcx;
            }
            int pr = 0;
#pragma unroll
            for (int a = 0; a < V; ++a) {
#pragma unroll
                for (int b = a + 1; b < V; ++b, ++pr) {
                    if (valid[a] && valid[b]) {
                        sd[pr] += sm_pixel_cost(sm_at(pl[a][0], i), sm_at(pl[a][1], i), sm_at(pl[a][2], i), sm_at(pl[a][3], i),
                                                sm_at(pl[b][0], i), sm_at(pl[b][1], i), sm_at(pl[b][2], i), sm_at(pl[b][3], i), prior);
                        sn[pr] += 1;
                    }
                }
            }
        }
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
            if (sn[pr]) {
                atomicAdd(&acc[((pr * 2 + 0) * ch + lcy) * cw + cur], sd[pr]);
                atomicAdd(&acc[((pr * 2 + 1) * ch + lcy) * cw + cur], sn[pr]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (xmax[v] >= 0) { atomicMin(&ex[2 * v], xmin[v]); atomicMax(&ex[2 * v + 1], xmax[v]); }
    }
    __syncthreads();
    const size_t grid_cells = (size_t)hq * wq4;
    const int cx0 = x0 >> shift, cy0 = y0 >> shift;
    const unsigned cc = 1u << (2 * shift);
    for (int i = threadIdx.x; i < NP * cells; i += 256) {          // D, nb and E = D c c / nb (-1: no overlap) of every whole cell
        const int pr = i / cells, rem = i - pr * cells;
        const int lcy = rem / cw, lcx = rem - lcy * cw;
        if (cx0 + lcx < wq && cy0 + lcy < hq) {
            const int d = acc[(pr * 2 + 0) * cells + rem], n = acc[(pr * 2 + 1) * cells + rem];
            int* o = cost + ((size_t)blockIdx.z * NP + pr) * 3 * grid_cells + (size_t)(cy0 + lcy) * wq4 + cx0 + lcx;
            o[0] = d;
            o[grid_cells] = n;
            o[2 * grid_cells] = n > 0 ? (int)(((unsigned)d * cc) / (unsigned)n) : -1;
            if (n > 0) rf[pr * ch + lcy] = 1;
        }
    }
    __syncthreads();
    if (threadIdx.x < NP * ch) {
        const int pr = threadIdx.x / ch, lcy = threadIdx.x - pr * ch;
        if (cy0 + lcy < hq) rowf[(((size_t)blockIdx.z * NP + pr) * hq + cy0 + lcy) * gridDim.x + blockIdx.x] = rf[threadIdx.x];
    }
    if (threadIdx.x < 2 * V) {
        const size_t blk = (size_t)blockIdx.z * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        ext[blk * (2 * V) + threadIdx.x] = ex[threadIdx.x];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// dp: workgroup p finds the seam between the views at places p and p + 1 of the sorted order, for every frame of the call in turn.
// One thread = groups of four columns (group g = thread + 256 k), so that a thread owns whole back-pointer bytes; one barrier per row.

// the dp kernel's loops stay as written: unrolled or interleaved, their loop-invariant values cost more scalar registers than there are
#define SM_PLAIN_LOOP _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")

// a workgroup barrier that orders LDS traffic only: the global loads of the next row's cost stay in flight across it
__device__ __forceinline__ void sm_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int V>
__global__ __launch_bounds__(256) void sm_dp_kernel(int* __restrict__ ws, int* __restrict__ state, int frames, int gx, int nblk, int hq, int wq,
                                                    int c, unsigned mu) {
    __shared__ __attribute__((aligned(16))) int lds[SSM_LDS_BYTES / 4];
    const int wq4 = (wq + 3) & ~3, groups = wq4 >> 2;
    int* red = lds;
    int* M = lds + SM_RED;                   // [2][wq4]
    int* xs = M + 2 * wq4;                   // [hq] the seam of this frame
    int* xprev = xs + hq;                    // [hq] the seam of the frame before
    int* rowany = xprev + hq;                // [hq] does the row hold an overlap cell?
    unsigned char* bp = reinterpret_cast<unsigned char*>(rowany + hq);       // [hq][groups] four 2-bit codes per byte
    unsigned long long* best = reinterpret_cast<unsigned long long*>(red + 8);
    constexpr int NP = V * (V - 1) / 2;
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t grid_cells = (size_t)hq * wq4;      // cost rows are padded to whole groups: 16-byte loads
    // the parts of the workspace, as sm_plan lays them out
    const int* cost = ws;
    const size_t ext_off = (size_t)frames * NP * 3 * grid_cells;
    const size_t rowf_off = ext_off + (size_t)frames * nblk * 2 * V + (size_t)frames * (V - 1) * hq + (size_t)frames * 8;
    int* hdr = state ? state + 8 * p : nullptr;
    int* sprev = state ? state + SSM_STATE_HEADER + (size_t)p * hq : nullptr;
    // the stored seam, if it was found on this grid
    bool have = false;
    int pord = -1;                           // the stored order, packed: o0 | o1 << 2 | (o2 & 3) << 4
    if (state) {
        have = hdr[0] == 1 && hdr[1] == V && hdr[2] == hq && hdr[3] == wq && hdr[4] == c;
        pord = hdr[5] | hdr[6] << 2 | (hdr[7] & 3) << 4;
        if (have) {
SM_PLAIN_LOOP
            for (int y = tid; y < hq; y += 256) xprev[y] = sprev[y];
        }
    }
    int ord = -1;
SM_PLAIN_LOOP
    for (int f = 0; f < frames; ++f) {
        // the view order from the extents
        if (tid < 6) red[tid] = (tid & 1) ? -1 : INT_MAX;
        if (tid == 0) *best = ~0ULL;
        __syncthreads();
        const int* ef = ws + ext_off + (size_t)f * nblk * 2 * V;
SM_PLAIN_LOOP
        for (int i = tid; i < nblk * 2 * V; i += 256) {
            const int k = i % (2 * V), val = ef[i];
            if (k & 1) { if (val >= 0) atomicMax(&red[k], val); }
            else if (val != INT_MAX) atomicMin(&red[k], val);
        }
        __syncthreads();
        int key[3];
        for (int v = 0; v < 3; ++v) key[v] = (v < V && red[2 * v + 1] >= 0) ? red[2 * v] + red[2 * v + 1] : INT_MAX;
        int o0 = 0, o1 = 1, o2 = V == 3 ? 2 : -1;
        if (V == 3) {                       // sort by (key, index): stable insertion on three
            if (key[o1] < key[o0]) { const int t = o0; o0 = o1; o1 = t; }
            if (key[o2] < key[o1]) { const int t = o1; o1 = o2; o2 = t; }
            if (key[o1] < key[o0]) { const int t = o0; o0 = o1; o1 = t; }
        } else if (key[1] < key[0]) { o0 = 1; o1 = 0; }
        const int va = p == 0 ? o0 : o1, vb = p == 0 ? o1 : o2;
        const int lo = min(va, vb), hi = max(va, vb);
        const int pair = V == 2 ? 0 : lo + hi - 1;
        const int* Ep = cost + (((size_t)f * NP + pair) * 3 + 2) * grid_cells;
        ord = o0 | o1 << 2 | (o2 & 3) << 4;
        const bool temporal = have && ord == pord;
        {                                   // a row is free unless a tile of the cost pass found an overlap cell in it
            const int* rf = ws + rowf_off + ((size_t)f * NP + pair) * hq * gx;
SM_PLAIN_LOOP
            for (int y = tid; y < hq; y += 256) {
                int a = 0;
SM_PLAIN_LOOP
                for (int b = 0; b < gx; ++b) a |= rf[y * gx + b];
                rowany[y] = a;
            }
        }
        __syncthreads();
        // the rows; columns wq .. wq4 - 1 hold INT_MAX in M and are nobody's predecessor
        const int4* E4 = reinterpret_cast<const int4*>(Ep);
        int4 ne = make_int4(0, 0, 0, 0);
        if (tid < groups) ne = E4[tid];
SM_PLAIN_LOOP
        for (int y = 0; y < hq; ++y) {
            const int4 e0 = ne;
            if (y + 1 < hq && tid < groups) ne = E4[(y + 1) * groups + tid];      // the next row's cost: in flight across the barrier
            const int any = rowany[y], xp = temporal ? xprev[y] : 0;
            const int* Mp = M + ((y + 1) & 1) * wq4;
            int* Mc = M + (y & 1) * wq4;
SM_PLAIN_LOOP
            for (int k = 0, g = tid; g < groups; ++k, g += 256) {
                const int x = 4 * g;
                const int4 e4 = k == 0 ? e0 : E4[y * groups + g];
                const int ec[4] = {e4.x, e4.y, e4.z, e4.w};
                int mp[6] = {INT_MAX, 0, 0, 0, 0, INT_MAX};
                if (y > 0) {
                    const int4 m4 = *reinterpret_cast<const int4*>(Mp + x);
                    mp[1] = m4.x; mp[2] = m4.y; mp[3] = m4.z; mp[4] = m4.w;
                    if (x > 0) mp[0] = Mp[x - 1];
                    if (x + 4 < wq4) mp[5] = Mp[x + 4];
                }
                int out[4];
                unsigned code = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned e = any ? (ec[i] >= 0 ? (unsigned)ec[i] : (unsigned)SM_PEN) : 0u;
                    if (temporal) e += min(mu * (unsigned)abs(x + i - xp), (unsigned)SM_TCAP);
                    int b = mp[i + 1];
                    unsigned cd = mp[i] < b ? 1u : 0u;
                    b = min(b, mp[i]);
                    cd = mp[i + 2] < b ? 2u : cd;
                    b = min(b, mp[i + 2]);
                    const int m = (int)min(e + (unsigned)b, (unsigned)SM_MCAP);
                    code |= cd << (2 * i);
                    out[i] = x + i < wq ? m : INT_MAX;
                }
                *reinterpret_cast<int4*>(Mc + x) = make_int4(out[0], out[1], out[2], out[3]);
                bp[y * groups + g] = (unsigned char)code;
            }
            sm_lds_barrier();
        }
        // the end point: the lowest x that minimises the last row
        {
            const int* Ml = M + ((hq - 1) & 1) * wq4;
            unsigned long long mine = ~0ULL;
SM_PLAIN_LOOP
            for (int x = tid; x < wq; x += 256) mine = min(mine, ((unsigned long long)(unsigned)Ml[x] << 32) | (unsigned)x);
            if (mine != ~0ULL) atomicMin(best, mine);
        }
        __syncthreads();
        // the backtrack, in LDS
        if (tid == 0) {
            int x = (int)(*best & 0xffffffffULL);
            xs[hq - 1] = x;
SM_PLAIN_LOOP
            for (int y = hq - 1; y > 0; --y) {
                const unsigned cd = (bp[y * groups + (x >> 2)] >> (2 * (x & 3))) & 3u;
                x += cd == 1 ? -1 : cd == 2 ? 1 : 0;
                xs[y - 1] = x;
            }
            int* mt = ws + ext_off + (size_t)frames * nblk * 2 * V + (size_t)frames * (V - 1) * hq + (size_t)f * 8;
            mt[3 + p] = (int)(*best >> 32);
            if (p == 0) { mt[0] = o0; mt[1] = o1; mt[2] = o2; if (V == 2) mt[4] = 0; mt[5] = 0; mt[6] = 0; mt[7] = 0; }
        }
        __syncthreads();
        int* sf = ws + ext_off + (size_t)frames * nblk * 2 * V + ((size_t)f * (V - 1) + p) * hq;
SM_PLAIN_LOOP
        for (int y = tid; y < hq; y += 256) { const int x = xs[y]; sf[y] = x; xprev[y] = x; }
        have = state != nullptr;
        pord = ord;
        __syncthreads();
    }
    if (state) {
SM_PLAIN_LOOP
        for (int y = tid; y < hq; y += 256) sprev[y] = xprev[y];
        if (tid == 0) { hdr[0] = 1; hdr[1] = V; hdr[2] = hq; hdr[3] = wq; hdr[4] = c; hdr[5] = ord & 3; hdr[6] = (ord >> 2) & 3; hdr[7] = V == 3 ? (ord >> 4) & 3 : -1; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// paint: one thread = one canvas pixel; plane 3 of the view at place k of the sorted order becomes V - |k - label|.
template <int V>
__global__ __launch_bounds__(256) void sm_paint_kernel(float* __restrict__ P, const int* __restrict__ seams, const int* __restrict__ meta, int hc,
                                                       int wc, int shift, int hq) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= wc || y >= hc) return;
    const int cx = x >> shift, cy = y >> shift;
    const int* sf = seams + (size_t)blockIdx.z * (V - 1) * hq;
    const int* mt = meta + (size_t)blockIdx.z * 8;
    const int x01 = sf[cy];
    int label = cx > x01 ? 1 : 0;
    if (V == 3) label += cx > max(sf[hq + cy], x01) ? 1 : 0;
    const size_t plane = (size_t)hc * wc;
    float* p = P + (size_t)blockIdx.z * (V * 5) * plane + (size_t)y * wc + x;
#pragma unroll
    for (int k = 0; k < V; ++k) p[(size_t)(mt[k] * 5 + 3) * plane] = (float)(V - abs(k - label));
}

int sm_status() { return hipGetLastError() == hipSuccess ? SSM_OK : SSM_ERR_LAUNCH; }

template <int V>
int sm_run(float* P, const SmPlan& p, int frames, int hc, int wc, unsigned mu, float prior, int* state, int* ws, hipStream_t st) {
    hipLaunchKernelGGL((sm_cost_kernel<V>), dim3(p.gx, p.gy, frames), dim3(256), 0, st, P, ws + p.cost, ws + p.ext, ws + p.rowf, hc, wc, p.shift, p.th,
                       p.hq, p.wq, prior);
    hipLaunchKernelGGL((sm_dp_kernel<V>), dim3(V - 1), dim3(256), 0, st, ws, state, frames, p.gx, p.nblk, p.hq, p.wq, p.c, mu);
    hipLaunchKernelGGL((sm_paint_kernel<V>), dim3(sm_cdiv(wc, 64), sm_cdiv(hc, 4), frames), dim3(256), 0, st, P, ws + p.seams, ws + p.meta,
                       hc, wc, p.shift, p.hq);
    return sm_status();
}

}      // namespace

extern "C" {

SSM_API int ssm_version(void) { return 1; }

SSM_API long long ssm_seam_workspace_bytes(int frames, int views, int hc, int wc, int cell) {
    SmPlan p;
    if (!sm_plan(frames, views, hc, wc, cell, &p)) return -1;
    return 4 * p.ints;
}

SSM_API int ssm_multiband_seam(float* P, int frames, int views, int hc, int wc, int cell, int mu, float prior, int* state,
                               long long state_ints, int* ws, long long ws_bytes, void* stream) {
    SmPlan p;
    if (!P || !ws || !sm_plan(frames, views, hc, wc, cell, &p)) return SSM_ERR_ARG;
    if (mu < 0 || mu > SSM_MU_MAX || !(prior >= 0.f && prior <= SSM_PRIOR_MAX)) return SSM_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(P) & 3) != 0 || (reinterpret_cast<uintptr_t>(state) & 3) != 0) return SSM_ERR_ARG;
    if (state && state_ints < SSM_STATE_HEADER + (long long)(views - 1) * p.hq) return SSM_ERR_ARG;
    if (ws_bytes < 4 * p.ints || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return SSM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return views == 2 ? sm_run<2>(P, p, frames, hc, wc, (unsigned)mu, prior, state, ws, st)
                      : sm_run<3>(P, p, frames, hc, wc, (unsigned)mu, prior, state, ws, st);
}

}
