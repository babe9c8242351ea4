/* C ABI of libstabstitch_blend.so: MULTIBAND fusion (the Laplacian-pyramid blend of Burt and Adelson) of views that
 * ss_tps_warp_mask_nchw (include/stabstitch_hip.h) has warped.  gfx950 only.  DESIGN.md section 7e has the definition and the
 * kernels; tests/multiband_ref.py states it in float64 and as an fp32 program.
 *
 * Every function that launches returns SSB_OK, SSB_ERR_ARG (refused before any launch) or SSB_ERR_LAUNCH.  `stream` is a
 * hipStream_t (NULL: the default stream).  Nothing here allocates, synchronises or uses atomics: a call is 2 * bands + 2 launches
 * whatever `frames` is (frames ride in the grid), and its result does not depend on timing. */
#ifndef STABSTITCH_BLEND_H
#define STABSTITCH_BLEND_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSB_API __declspec(dllexport)
#else
#define SSB_API __attribute__((visibility("default")))
#endif

#define SSB_OK 0
#define SSB_ERR_ARG -1
#define SSB_ERR_LAUNCH -2

#define SSB_MAX_VIEWS 3
#define SSB_MAX_BANDS 6

SSB_API int ssb_version(void);

/* Floats of workspace that ssb_multiband_blend* needs, or -1 for arguments it would refuse: frames >= 1, views 2 or 3,
 * 0 <= bands <= SSB_MAX_BANDS, and every level that is reduced (levels 0 .. bands - 1; sizes n' = (n + 1) / 2 per axis) has both
 * sides >= 3.  With K = views - 1, s_l = (w_l + 3) & ~3 the row stride of level l and a_l = h_l * s_l:
 *     frames * (4 * K * sum_{l = 0..bands} a_l  +  3 * sum_{l = 1..bands} a_l  +  4 * a_0)
 * (the pyramids of K * 3 colour-difference planes and K seam-weight planes; the collapsed colour planes of the levels below the
 * canvas; the last view's filled colours and the union mask). */
SSB_API long long ssb_multiband_workspace_floats(int frames, int views, int hc, int wc, int bands);

/* P [frames][views][5][hc][wc]: per view the warped B, G, R (0..255), the warped weight plane and the ones-mask, as
 * ss_tps_warp_mask_nchw writes them for U [views][4][h][w] = frame planes + the weight plane min(x + 1, w - x) * min(y + 1, h - y).
 * out [frames][3][hc][wc] fp32: the blend, clamped to 0..255 on the union of the masks (mask >= 0.5) and 0 outside it.
 * ws: ws_floats >= ssb_multiband_workspace_floats(...) floats, 16-byte aligned; overwritten.  P, out and ws must not overlap. */
SSB_API int ssb_multiband_blend(const float* P, float* out, float* ws, long long ws_floats, int frames, int views, int hc, int wc,
                                int bands, void* stream);
/* the same values as `.astype(uint8)` (truncation), out [frames][hc][wc][3] bytes, written by the last collapse pass */
SSB_API int ssb_multiband_blend_u8(const float* P, unsigned char* out, float* ws, long long ws_floats, int frames, int views, int hc,
                                   int wc, int bands, void* stream);

#ifdef __cplusplus
}
#endif
#endif
