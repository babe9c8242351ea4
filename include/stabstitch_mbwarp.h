/* C ABI of libstabstitch_mbwarp.so: the direct warp of MULTIBAND fusion.  One launch from the caller's frames to the planes
 * P [frames][views][5][hc][wc] that ssm_multiband_seam (include/stabstitch_seam.h) and ssb_multiband_blend (include/stabstitch_blend.h)
 * read, with optional exposure gains (ss_exposure_update, include/stabstitch_hip.h) applied to the sampled colours.  gfx950 only.
 * DESIGN.md section 7g has the definition and the kernel.
 *
 * Without gains the result equals, bit for bit, ss_tps_warp_mask_nchw on the stacked planes U [frames * views][4][h][w] = B, G, R and
 * the weight plane min(x + 1, w - x) * min(y + 1, h - y); U itself is never written: the weight plane's taps are computed, not read.
 *
 * Every function that launches returns SSW_OK, SSW_ERR_ARG (refused before any launch) or SSW_ERR_LAUNCH.  `stream` is a
 * hipStream_t (NULL: the default stream).  Nothing here allocates or synchronises; a call is one launch. */
#ifndef STABSTITCH_MBWARP_H
#define STABSTITCH_MBWARP_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSW_API __declspec(dllexport)
#else
#define SSW_API __attribute__((visibility("default")))
#endif

#define SSW_OK 0
#define SSW_ERR_ARG -1
#define SSW_ERR_LAUNCH -2

#define SSW_MAX_VIEWS 3
#define SSW_MAX_ITEMS 65535          /* frames * views of one call: the (frame, view) items are the grid's z dimension */
#define SSW_WARP_NORMAL 0            /* the sampling modes of include/stabstitch_hip.h (SS_WARP_NORMAL, SS_WARP_FAST) */
#define SSW_WARP_FAST 1

SSW_API int ssw_version(void);

/* imgs: `views` (2 or 3) device pointers, view k's frames as fp32 planes [frames][3][h][w] (0..255).
 * source [frames][views][63][2], T [frames][views][2][66]: the splines, as the renders of include/stabstitch_hip.h take them.
 * gains: NULL, or [frames][views][3] fp32: a sampled value s of view v, channel c is written as fminf(gains[v][c] * s, 255).
 * out = P [frames][views][5][hc][wc]: per view the warped B, G, R, the warped weight plane and the ones-mask; planes 3 and 4 never
 * see the gains.  h, w, hc, wc > 1; frames >= 1 and frames * views <= SSW_MAX_ITEMS; mode SSW_WARP_NORMAL or SSW_WARP_FAST. */
SSW_API int ssw_multiband_warp(const float* const* imgs, const float* source, const float* T, const float* gains, float* out, int frames,
                               int views, int h, int w, int hc, int wc, int mode, void* stream);

/* The same from decoded frames [frames][h][w][3] uint8 (uint8 -> fp32 is exact: the planes equal those of ssw_multiband_warp on the
 * converted frames bit for bit). */
SSW_API int ssw_multiband_warp_u8(const unsigned char* const* imgs, const float* source, const float* T, const float* gains, float* out,
                                  int frames, int views, int h, int w, int hc, int wc, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif
