/* C ABI of libstabstitch_surfaces.so: decoded NV12 surfaces to packed BGR frames, a list of surfaces per launch.  gfx950 only.
 * DESIGN.md section 7i has the definition and the kernel.
 *
 * A hardware decoder hands out a POOL of surfaces: every frame has its own Y plane, its own interleaved UV plane and its own bytes
 * per row, which the frame stride of ss_ingest_nv12 (include/stabstitch_hip.h) cannot express.  One call here converts up to
 * SSF_MAX_SURFACES such surfaces -- k frames of every view of a push_many_nv12 -- into one tensor of uint8 video frames in a single
 * launch.  The colour statement is the NV12 routes' first one (csrc/nv12.h, tests/nv12_ref.py): BT.601 limited range in
 * 20-bit fixed point, the chroma pair of pixel (y, x) taken from (y >> 1, x >> 1) without interpolation.
 *
 * A function that launches returns SSF_OK, SSF_ERR_ARG (refused before any device work) or SSF_ERR_LAUNCH.  `stream` is a
 * hipStream_t (NULL: the default stream).  Nothing here allocates or synchronises; a call is one launch. */
#ifndef STABSTITCH_SURFACES_H
#define STABSTITCH_SURFACES_H

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define SSF_API __declspec(dllexport)
#else
#define SSF_API __attribute__((visibility("default")))
#endif

#define SSF_OK 0
#define SSF_ERR_ARG -1
#define SSF_ERR_LAUNCH -2

#define SSF_MAX_SURFACES 96          /* 32 frames x 3 views; the surfaces are the grid's z dimension and ride in the kernel arguments */

SSF_API int ssf_version(void);

/* y, uv, pitch: HOST arrays of `surfaces` entries, consumed during the call: surface s has its Y plane at y[s] (h rows), its
 * interleaved UV plane at uv[s] (h / 2 rows of w bytes: U, V, U, V ..) and pitch[s] bytes per row of BOTH planes; y[s] and uv[s] are
 * device pointers.  out [surfaces][h][w][3] uint8 in B, G, R order, frame s at out + s * out_stride (formed in 64 bits).
 * Refused: a null array, entry or out; surfaces outside 1..SSF_MAX_SURFACES; h or w odd or not positive; h * w >= 2^31; h above
 * 8 * 65535 (the row tiles are the grid's y dimension); a pitch that is odd or below w; a uv[s] that is not 2-byte aligned;
 * out_stride < 3 * h * w.
 * When w, every pitch and out_stride are multiples of 8 and every y[s], uv[s] and out are 8-byte aligned, a thread converts 8 x 2
 * pixels with 8-byte loads and stores; otherwise -- the choice is per call -- a thread converts one 2 x 2 block.  Same bytes. */
SSF_API int ssf_nv12_to_bgr(const unsigned char* const* y, const unsigned char* const* uv, const int* pitch, int surfaces, int h, int w,
                            unsigned char* out, long long out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
