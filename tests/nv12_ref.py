"""The two colour statements of the NV12 frame format ("Frame formats") in numpy: BT.601 limited range, 20-bit fixed
point, plain integer arithmetic with an arithmetic shift.  The library's NV12 routes are held to "convert with nv12_to_bgr, run the
packed-BGR route, convert with bgr_to_nv12" byte for byte (tests/test_gpu_nv12.py); tests/test_nv12_abi.py holds these statements
themselves to the real-valued BT.601 formulas."""
import numpy as np

HALF = 1 << 19


def yuv_to_bgr(Y, U, V):
    """Integer arrays of one shape (values 0..255) -> (B, G, R) uint8."""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    c = np.maximum(0, Y - 16) * 1220542
    u, v = U - 128, V - 128
    sat8 = lambda a: np.clip(a, 0, 255).astype(np.uint8)
    return (sat8((c + 2116026 * u + HALF) >> 20),
            sat8((c - 409993 * u - 852492 * v + HALF) >> 20),
            sat8((c + 1673527 * v + HALF) >> 20))


def bgr_to_y(B, G, R):
    B, G, R = (np.asarray(a).astype(np.int64) for a in (B, G, R))
    return (269484 * R + 528482 * G + 102760 * B + (16 << 20) + HALF) >> 20


def bgr_to_uv(B, G, R):
    """(B, G, R) of a 2 x 2 block's rounded mean colour -> (U, V), unclamped."""
    B, G, R = (np.asarray(a).astype(np.int64) for a in (B, G, R))
    return ((-155188 * R - 305135 * G + 460324 * B + (128 << 20) + HALF) >> 20,
            (460324 * R - 385875 * G - 74448 * B + (128 << 20) + HALF) >> 20)


def nv12_to_bgr(frame, h=None):
    """NV12 uint8 [h*3/2, w] (rows 0..h-1 Y, rows h.. interleaved UV; a wider array's leading w columns will do) -> uint8 [h,w,3] in
    B, G, R order; U and V of pixel (y, x) come from the pair at (y >> 1, x >> 1), no chroma interpolation."""
    frame = np.asarray(frame)
    if h is None:
        h = frame.shape[0] // 3 * 2
    w = frame.shape[1]
    assert frame.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0 and frame.shape[0] == h // 2 * 3
    Y = frame[:h]
    uv = frame[h:].reshape(h // 2, w // 2, 2)
    U = np.repeat(np.repeat(uv[..., 0], 2, 0), 2, 1)
    V = np.repeat(np.repeat(uv[..., 1], 2, 0), 2, 1)
    return np.stack(yuv_to_bgr(Y, U, V), -1)


def bgr_to_nv12(bgr):
    """uint8 [h,w,3] in B, G, R order, h and w even -> NV12 uint8 [h*3/2, w]."""
    bgr = np.asarray(bgr)
    h, w, _ = bgr.shape
    assert bgr.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0
    out = np.empty((h // 2 * 3, w), np.uint8)
    out[:h] = bgr_to_y(bgr[..., 0], bgr[..., 1], bgr[..., 2]).astype(np.uint8)
    mean = (bgr.astype(np.int64).reshape(h // 2, 2, w // 2, 2, 3).sum((1, 3)) + 2) >> 2
    U, V = bgr_to_uv(mean[..., 0], mean[..., 1], mean[..., 2])
    out[h:] = np.stack((U, V), -1).astype(np.uint8).reshape(h // 2, w)
    return out


def random_nv12(rng, h, w):
    """A frame of random bytes over the full 0..255 range in all three channels: luma below 16 and saturating chroma occur."""
    return rng.integers(0, 256, (h // 2 * 3, w), dtype=np.uint8)
