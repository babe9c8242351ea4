"""Coverage bitmaps and the largest covered rectangle in numpy (libstabstitch_cover.so): the word layout, the rectangle
by the stack algorithm, and a brute-force search over all rectangles with the same order of preference.  A plain helper module
(imported like multiband_ref): tests/test_cover_abi.py holds the two searches against each other, tests/test_gpu_cover.py the library
against the first.

Layout: [hc][ceil(wc / 64)] 64-bit words (int64, as torch holds them), bit i of word j = column 64 j + i.
Rectangle: (y0, x0, h, w), the covered rectangle of largest area; among those the smallest y0, then the smallest x0, then the
largest width; (0, 0, 0, 0) when nothing is covered.  even: afterwards h -= h & 1, w -= w & 1, same origin."""
import numpy as np


def words(wc):
    return (wc + 63) // 64


def pack(mask):
    """bool [..., hc, wc] -> int64 [..., hc, W64]; the bits of columns >= wc are 0."""
    mask = np.asarray(mask, dtype=bool)
    wc = mask.shape[-1]
    padded = np.zeros(mask.shape[:-1] + (words(wc) * 64,), dtype=np.uint64)
    padded[..., :wc] = mask
    bits = padded.reshape(mask.shape[:-1] + (words(wc), 64)) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=-1).view(np.int64)


def unpack(bitmap, wc, pad=False):
    """int64 [..., hc, W64] -> bool [..., hc, wc] (pad: all 64 W64 columns, the pad bits included)."""
    b = np.ascontiguousarray(bitmap).view(np.uint64)
    bits = (b[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    out = bits.reshape(b.shape[:-1] + (b.shape[-1] * 64,)).astype(bool)
    return out if pad else out[..., :wc]


def _key(r):
    y0, x0, h, w = r
    return (-h * w, y0, x0, -w)


def _even(r, even):
    y0, x0, h, w = r
    return (y0, x0, h - (h & 1), w - (w & 1)) if even else r


def rect(mask, even=False):
    """The stack algorithm (largest rectangle in a histogram, row by row): every candidate is a bottom row and a limiting column."""
    mask = np.asarray(mask, dtype=bool)
    hc, wc = mask.shape
    best = (0, 0, 0, 0)
    heights = np.zeros(wc, dtype=np.int64)
    for y in range(hc):
        heights = np.where(mask[y], heights + 1, 0)
        stack = []                                       # columns of increasing height
        for x in range(wc + 1):
            cur = int(heights[x]) if x < wc else -1
            while stack and int(heights[stack[-1]]) >= cur:
                h = int(heights[stack.pop()])
                left = stack[-1] + 1 if stack else 0
                if h > 0:
                    cand = (y - h + 1, left, h, x - left)
                    if _key(cand) < _key(best):
                        best = cand
            stack.append(x)
    return _even(best, even)


def rect_brute(mask, even=False):
    """Every rectangle, through a summed-area table."""
    mask = np.asarray(mask, dtype=bool)
    hc, wc = mask.shape
    sat = np.zeros((hc + 1, wc + 1), dtype=np.int64)
    sat[1:, 1:] = mask.cumsum(0).cumsum(1)
    best = (0, 0, 0, 0)
    for y0 in range(hc):
        for y1 in range(y0 + 1, hc + 1):
            for x0 in range(wc):
                inside = sat[y1, x0 + 1:] - sat[y0, x0 + 1:] - sat[y1, x0] + sat[y0, x0]
                full = inside == (y1 - y0) * np.arange(1, wc - x0 + 1)
                w = wc - x0 if full.all() else int(np.argmin(full))       # the widest covered rectangle from this corner
                if w > 0:
                    cand = (y0, x0, y1 - y0, w)
                    if _key(cand) < _key(best):
                        best = cand
    return _even(best, even)


def staircase(hc, wc):
    """Row y covered up to column y * wc / hc."""
    return np.arange(wc)[None, :] < (np.arange(hc)[:, None] * wc // hc)


def ties(hc=12, wc=70):
    """Constructed ties -> {name: (mask, expected rect)}: equal areas side by side (the left one: smaller x0), one above the other
    (the upper one: smaller y0), and a 2 x 6 against a 3 x 4 from one corner (the same y0 and x0: the wider one)."""
    out = {}
    m = np.zeros((hc, wc), dtype=bool)
    m[2:5, 3:8] = True
    m[2:5, 20:25] = True
    out['side_by_side'] = (m, (2, 3, 3, 5))
    m = np.zeros((hc, wc), dtype=bool)
    m[1:4, 10:15] = True
    m[6:9, 2:7] = True
    out['above'] = (m, (1, 10, 3, 5))
    m = np.zeros((hc, wc), dtype=bool)
    m[4:6, 62:68] = True
    m[4:7, 62:66] = True
    out['corner'] = (m, (4, 62, 2, 6))
    return out
