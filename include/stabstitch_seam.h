/* C ABI of libstabstitch_seam.so: the content-aware seam of MULTIBAND fusion, a per-frame dynamic-programming seam finder that runs
 * between ss_tps_warp_mask_nchw (include/stabstitch_hip.h) and ssb_multiband_blend (include/stabstitch_blend.h).  gfx950 only.
 * DESIGN.md section 7f has the definition and the kernels; tests/seam_ref.py states it as an integer and fp32 program that the kernels
 * equal bit for bit.
 *
 * Every function that launches returns SSM_OK, SSM_ERR_ARG (refused before any launch) or SSM_ERR_LAUNCH.  `stream` is a
 * hipStream_t (NULL: the default stream).  Nothing here allocates or synchronises; a call is three launches whatever `frames` is, and
 * every sum is an integer sum: the result does not depend on timing or on the order of the additions. */
#ifndef STABSTITCH_SEAM_H
#define STABSTITCH_SEAM_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSM_API __declspec(dllexport)
#else
#define SSM_API __attribute__((visibility("default")))
#endif

#define SSM_OK 0
#define SSM_ERR_ARG -1
#define SSM_ERR_LAUNCH -2

#define SSM_MAX_VIEWS 3
#define SSM_MU_MAX 65535
#define SSM_PRIOR_MAX 255.0f
#define SSM_STATE_HEADER 16          /* ints in front of the seams of a state buffer */
#define SSM_LDS_BYTES 163840         /* what one workgroup can have on gfx950: the dynamic program's rows and back pointers live there */
#define SSM_TILE_W 256               /* canvas columns per workgroup of the cost pass; it covers max(4, cell) rows */

SSM_API int ssm_version(void);

/* Bytes of workspace that ssm_multiband_seam needs, or -1 for arguments it would refuse: frames 1..65535, views 2 or 3, hc and wc in
 * 1..32768, cell one of 1, 2, 4, 8, 16, and a cell grid hq = ceil(hc / cell), wq = ceil(wc / cell) whose dynamic program fits the LDS:
 * with wq4 = (wq + 3) & ~3,
 *     4 * (16 + 2 * wq4 + 3 * hq) + hq * wq4 / 4  <=  SSM_LDS_BYTES.
 * The workspace is int32, in this order (NP = views * (views - 1) / 2 pairs (0,1) | (0,1), (0,2), (1,2); nblk = ceil(wc / SSM_TILE_W) *
 * ceil(hc / max(4, cell)) workgroups of the cost pass per frame):
 *     cost   [frames][NP][3][hq][wq4]   per cell D (summed pixel cost), nb (both-valid pixels) and E (-1: nb = 0); columns past wq: unspecified
 *     ext    [frames][nblk][views][2]   first and last valid column per view, per workgroup (INT_MAX, -1: none)
 *     seams  [frames][views - 1][hq]    x(y) of each dynamic program, in the sorted view order, before the second is raised
 *     meta   [frames][8]                the sorted view order (3; -1 past `views`), the cost of each seam (2), 3 unused
 *     rowf   [frames][NP][hq][gx]       per row of cells and column of workgroups (gx = ceil(wc / SSM_TILE_W)): an overlap cell there?
 * so it is 4 * frames * (NP * (3 * hq * wq4 + hq * gx) + nblk * views * 2 + (views - 1) * hq + 8) bytes. */
SSM_API long long ssm_seam_workspace_bytes(int frames, int views, int hc, int wc, int cell);

/* P [frames][views][5][hc][wc] fp32 as ss_tps_warp_mask_nchw writes it (per view B, G, R, the warped weight plane, the ones-mask):
 * plane 3 of every view is overwritten with the seam weights views - |k - label| (k: the view's place in the sorted order).
 * mu 0..SSM_MU_MAX, prior 0..SSM_PRIOR_MAX.
 * state: NULL (no temporal term), or state_ints >= SSM_STATE_HEADER + (views - 1) * hq int32 that belong to one stream: two headers of
 * 8 ints {valid, views, hq, wq, cell, order[3]}, one per dynamic program, then xprev [views - 1][hq].  An all-zero buffer is a fresh
 * state.  The frames of a call are taken in order and the state is left as after the last one: n frames in one call equal n calls.
 * ws: ws_bytes >= ssm_seam_workspace_bytes(...), 16-byte aligned; overwritten.  P, state and ws must not overlap. */
SSM_API int ssm_multiband_seam(float* P, int frames, int views, int hc, int wc, int cell, int mu, float prior, int* state,
                               long long state_ints, int* ws, long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
