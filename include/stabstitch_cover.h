/* C ABI of libstabstitch_cover.so: which canvas pixels a stitched frame covers, and the largest axis-aligned rectangle that every
 * frame of a clip (or of a stream so far) covers.  gfx950 only.  DESIGN.md section 7l has the definition and the kernels.
 *
 * Coverage.  Per view v and canvas pixel, mask_v is the value ss_tps_warp_mask_nchw (include/stabstitch_hip.h) and ssw_multiband_warp
 * (include/stabstitch_mbwarp.h) write to their mask plane, bit for bit: the same spline evaluation in the same tile geometry, the
 * same taps.  A pixel is covered in a frame when mask_v >= min_mask for at least one view, and in a clip when every frame covers it.
 *
 * Bitmap.  [hc][ceil(wc / 64)] 64-bit words; bit i of word j of a row is column 64 j + i.  The bits of columns >= wc are written
 * as 0 by ssc_coverage and are never read as covered by ssc_covered_rect, whatever they hold.
 *
 * Every function that launches returns SSC_OK, SSC_ERR_ARG (refused before any launch) or SSC_ERR_LAUNCH; the two size queries
 * return SSC_ERR_ARG for sizes the launches refuse.  `stream` is a hipStream_t (NULL: the default stream).  Nothing here allocates,
 * synchronises or copies to the host. */
#ifndef STABSTITCH_COVER_H
#define STABSTITCH_COVER_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSC_API __declspec(dllexport)
#else
#define SSC_API __attribute__((visibility("default")))
#endif

#define SSC_OK 0
#define SSC_ERR_ARG -1
#define SSC_ERR_LAUNCH -2

#define SSC_MAX_VIEWS 3
#define SSC_MAX_FRAMES 65535         /* frames of one call without `accumulate`: they are the grid's z dimension */
/* the widest canvas: the search keeps one row's heights and a min-tree over them in LDS, 2 * 4 bytes per column rounded up to a
 * power of two -- 64 KiB at 8192 columns, what a launch gets without opting into more */
#define SSC_MAX_WIDTH 8192
#define SSC_WARP_NORMAL 0            /* the sampling modes of include/stabstitch_hip.h (SS_WARP_NORMAL, SS_WARP_FAST) */
#define SSC_WARP_FAST 1

SSC_API int ssc_version(void);

/* 64-bit words of one hc x wc bitmap: hc * ceil(wc / 64).  SSC_ERR_ARG for hc, wc <= 1 or wc > SSC_MAX_WIDTH. */
SSC_API long long ssc_bitmap_words(int hc, int wc);

/* source [frames][views][63][2], T [frames][views][2][66]: the splines, as the renders of include/stabstitch_hip.h take them, of
 * views (2 or 3) images of h x w on a canvas of hc x wc.  One launch.
 * accumulate == 0: bitmap [frames][hc][W64], one bitmap per frame, every word written.
 * accumulate != 0: bitmap [hc][W64] is the caller's running state: every word becomes itself AND the coverage of all `frames`
 * frames (a fresh state holds ones in the columns < wc).  No atomics: a word belongs to one wave, which loops over the frames.
 * h, w, hc, wc > 1; wc <= SSC_MAX_WIDTH; frames >= 1 (<= SSC_MAX_FRAMES without accumulate); 0 < min_mask <= 1. */
SSC_API int ssc_coverage(const float* source, const float* T, unsigned long long* bitmap, int frames, int views, int h, int w, int hc,
                         int wc, int mode, float min_mask, int accumulate, void* stream);

/* bytes of the workspace ssc_covered_rect needs on a hc x wc canvas (column heights int32 [hc][wc], four candidates per row).
 * SSC_ERR_ARG for sizes ssc_covered_rect refuses. */
SSC_API long long ssc_rect_workspace_bytes(int hc, int wc);

/* rect int32 [4] on the device = (y0, x0, h, w): the covered rectangle of largest area; among those the smallest y0, then the
 * smallest x0, then the largest width.  (0, 0, 0, 0) for a bitmap without a covered pixel.  even != 0: afterwards h -= h & 1 and
 * w -= w & 1, same origin.  Three launches of integer arithmetic; the time does not depend on the bitmap's contents beyond
 * O(log wc) steps per column.  ws: ws_bytes >= ssc_rect_workspace_bytes(hc, wc) bytes of device memory, 8-byte aligned.
 * hc, wc > 1; wc <= SSC_MAX_WIDTH; hc * wc < 2^31. */
SSC_API int ssc_covered_rect(const unsigned long long* bitmap, int hc, int wc, int even, void* ws, long long ws_bytes, int* rect,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
