/* C ABI of libstabstitch_resample.so: a rectangle of stitched frames resampled, with a prefilter, to a fixed output size -- fp32
 * planes, packed BGR bytes or NV12.  gfx950 only.  DESIGN.md section 7m has the definition, the kernel and what was measured;
 * tests/resample_ref.py states the same definition in numpy float64.
 *
 * Rectangle.  (y0, x0, h, w) is intersected with the Hc x Wc frame; call the result R.  An empty R gives black everywhere: 0.0f,
 * bytes 0, or Y = 16 and U = V = 128.
 *
 * Window: the part of R that is resampled, in double, one operation after the other, no contraction.
 *   aspect SSR_ASPECT_STRETCH: the window is R.
 *   aspect SSR_ASPECT_FILL: the centred part of R with the output's aspect (h, w are R's):
 *     w * Hout > h * Wout:  fw = h * Wout / Hout,  fx = x0 + (w - fw) / 2,  rows unchanged;
 *     w * Hout < h * Wout:  fh = w * Hout / Wout,  fy = y0 + (h - fh) / 2,  columns unchanged;   else the window is R.
 *   The window may be fractional.
 *
 * Per axis, for the window [o, o + len) over n_out outputs and R's integer range [lo, hi) on that axis -- the separable triangle
 * filter of PIL and of interpolate(mode='bilinear', antialias=True, align_corners=False):
 *   scale = len / n_out,  support = max(scale, 1),  c_i = o + scale * (i + 0.5);
 *   taps j in [max(lo, floor(c_i - support + 0.5)), min(hi, floor(c_i + support + 0.5)));
 *   weight max(0, 1 - |j + 0.5 - c_i| / support), divided by the sum over the taps kept (added in ascending j).
 * Taps clamp to R, not to the frame: no pixel outside the rectangle leaks in.  All of this is double; a weight is rounded to fp32
 * once.  Accumulation is fp32 fmaf in a fixed order, the two passes of the separable form: per tap row in ascending order the
 * horizontal sum hrow = fmaf(wx_k, pixel_k, hrow) over ascending k from 0, then acc = fmaf(wy_j, hrow, acc) from 0.
 *
 * Outputs: fp32 planes unrounded; bytes floor(v + 0.5) saturated to 0 .. 255; NV12 is the BT.601 conversion of those bytes that
 * ss_bgr_to_nv12 (include/stabstitch_hip.h) does, byte for byte, without the BGR frame being written.
 *
 * The rectangle comes either from the device -- rect_dev, int32 [4] = (y0, x0, h, w) as ssc_covered_rect (include/stabstitch_cover.h)
 * leaves it, read inside the kernel: the host never sees it, any four values give a defined result -- or, with rect_dev NULL, as the
 * four ints y0, x0, h, w, none negative.
 *
 * Every launching function is ONE launch whatever n and returns SSR_OK, SSR_ERR_ARG (refused before the launch) or SSR_ERR_LAUNCH.
 * `stream` is a hipStream_t (NULL: the default stream).  Nothing here allocates, synchronises or copies to the host.
 * Refused: a null pointer other than rect_dev; n <= 0 or n > SSR_MAX_FRAMES; a size < 1; a frame of 2^31 pixels or more, in or out;
 * Hout > 16 * 65535 or Wout > 64 * 65535; an aspect that is neither; a negative member of a host rectangle. */
#ifndef STABSTITCH_RESAMPLE_H
#define STABSTITCH_RESAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSR_API __declspec(dllexport)
#else
#define SSR_API __attribute__((visibility("default")))
#endif

#define SSR_OK 0
#define SSR_ERR_ARG -1
#define SSR_ERR_LAUNCH -2

#define SSR_ASPECT_STRETCH 0
#define SSR_ASPECT_FILL 1
#define SSR_MAX_FRAMES 65535         /* the frames of a call are the grid's z dimension */

SSR_API int ssr_version(void);

/* Host only, no launch: out[4] = (fy, fx, fh, fw), the window of rect = (y0, x0, h, w) (no member negative) on a Hc x Wc frame for
 * an output of Hout x Wout, by the rule above -- the same function the kernels run; zeros for an empty R. */
SSR_API int ssr_source_window(const int rect[4], int Hc, int Wc, int Hout, int Wout, int aspect, double out[4]);

/* in fp32 [n][3][Hc][Wc] -> out fp32 [n][3][Hout][Wout], both dense. */
SSR_API int ssr_resample_f32(const float* in, float* out, int n, int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev,
                             int y0, int x0, int h, int w, void* stream);

/* in uint8 [n][Hc][Wc][3] dense -> out uint8 [n][Hout][Wout][3], frame i at out + i * out_frame_stride bytes
 * (out_frame_stride >= 3 * Hout * Wout). */
SSR_API int ssr_resample_u8(const unsigned char* in, unsigned char* out, long long out_frame_stride, int n, int Hc, int Wc, int Hout,
                            int Wout, int aspect, const int* rect_dev, int y0, int x0, int h, int w, void* stream);

/* in uint8 [n][Hc][Wc][3] dense -> NV12: Y plane y and interleaved UV plane uv of frame 0, `pitch` bytes per row of both, frame i
 * at + i * frame_stride bytes.  Hout, Wout, pitch and frame_stride even, pitch >= Wout, uv 2-byte aligned,
 * frame_stride >= pitch * Hout * 3 / 2. */
SSR_API int ssr_resample_u8_nv12(const unsigned char* in, unsigned char* y, unsigned char* uv, int pitch, long long frame_stride, int n,
                                 int Hc, int Wc, int Hout, int Wout, int aspect, const int* rect_dev, int y0, int x0, int h, int w,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
