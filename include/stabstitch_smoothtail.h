/* C ABI of libstabstitch_smoothtail.so: SmoothNet's Conv3d stack for a stitched clip, restricted to what the stitch reads.
 * ss_smooth_stitch (include/stabstitch_hip.h) reads the decoder output of window 0 at its 7 frames and of every later window at
 * frame 6 only; with temporal taps 5 and padding 2 a later window therefore needs output frames 2..6, 4..6 and 6 of the three
 * Conv3d(128,128,(5,3,3)) layers.  Here a layer computes exactly those frames, on compact activations, and never multiplies a
 * temporal tap that falls into the zero padding.  gfx950 only.  DESIGN.md section 7j has the kernel.
 *
 * The sum of one output value is the one ss_conv_nhwc forms for the whole windows: the same MFMA sequence over k = (dt, dh, dw, ci),
 * cut at the same K tiles when `seg_tiles` is that launch's cut, the partial sums added in the same order.  The skipped products are
 * zeros, so the frames computed here equal the full computation's bit for bit.
 *
 * Compact activations [frames][63][128]: window 0 holds frames 0..6, every window k >= 1 the frames first..6 only, windows back to
 * back: frame f of window k >= 1 is compact frame 7 + (k - 1) * (7 - first) + (f - first).  first = 0 is the plain [nw][7][63][128].
 *
 * Every function that launches returns SST_OK, SST_ERR_ARG (refused before any launch) or SST_ERR_LAUNCH.  `stream` is a hipStream_t
 * (NULL: the default stream).  Nothing here allocates or synchronises. */
#ifndef STABSTITCH_SMOOTHTAIL_H
#define STABSTITCH_SMOOTHTAIL_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SST_API __declspec(dllexport)
#else
#define SST_API __attribute__((visibility("default")))
#endif

#define SST_OK 0
#define SST_ERR_ARG -1
#define SST_ERR_LAUNCH -2

#define SST_MAX_WINDOWS 2048         /* windows of one call (smooth_network.WINDOW_CHUNK) */
#define SST_K_TILES 180              /* K = 5 * 3 * 3 * 128 walked 32 at a time */

SST_API int sst_version(void);

/* Compact frames of `nw` windows whose later windows start at frame `first`: 7 + (nw - 1) * (7 - first). */
SST_API long long sst_compact_frames(int nw, int first);

/* One ragged layer: out = relu(conv3d(in) + bias) at frames 0..6 of window 0 and first_out..6 of every later window.
 * in: compact activations with first = first_in; out: compact with first = first_out; first_in <= max(first_out - 2, 0).
 * wgt [128][5][3][3][128] (cout, dt, dh, dw, cin); bias [128] or NULL.
 * seg_tiles in 1..SST_K_TILES: the K tiles of one partial sum.  With seg_tiles < SST_K_TILES the layer is two launches (partial sums,
 * then their sum in the order of the segments) and ws must hold ceil(SST_K_TILES / seg_tiles) * frames_out * 63 * 128 floats. */
SST_API int sst_conv3d_layer(const float* in, const float* wgt, const float* bias, float* out, float* ws, long long ws_floats, int nw,
                             int first_in, int first_out, int seg_tiles, void* stream);

/* Linear(128, 4) on compact rows (first as above), written to delta[((k * 7 + f) * 63 + v) * 4 + o], the [nw][7][63][4] layout
 * ss_smooth_stitch reads; entries of frames that are not in the compact set stay unwritten.  w [4][128]; b [4] or NULL. */
SST_API int sst_decode_scatter(const float* hid, const float* w, const float* b, float* delta, int nw, int first, void* stream);

#ifdef __cplusplus
}
#endif
#endif
