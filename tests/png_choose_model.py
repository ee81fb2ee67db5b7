"""Filter selection by the heuristic of the PNG specification (12.8 "Filter selection", libpng's
default), in plain integers over png_model.filter_rows: the referee for fdh_png_choose_filters_batch.

    for every row and every type t in 0..4: filter the row with t (png_model.filter_rows: raw
    neighbours, zeros above row 0), read every filtered byte v as signed -- its cost is
    v if v < 128 else 256 - v, so 128 costs 128 --, sum the costs of the row's row_bytes bytes (the
    type byte is not counted); the row's type is the one with the smallest sum, the LOWEST type
    number on equal sums.

Also the images the selection tests share (choose_images), built so that every type wins somewhere
and many rows have a tied minimum; tests/test_png_choose_model.py asserts that coverage.
"""
import numpy as np

import png_model

TYPES = (0, 1, 2, 3, 4)
ROWS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1, 70)   # tests/test_gpu_png.py's: band boundaries everywhere


def cost(v):
    """Cost of filtered bytes (any integer array of values 0..255)."""
    v = np.asarray(v).astype(np.int64)
    return np.where(v < 128, v, 256 - v)


def choose(pix, bpp):
    """pix: uint8 [rows, row_bytes] -> (types uint8 [rows], sums int64 [5, rows])."""
    pix = np.asarray(pix, dtype=np.uint8)
    rows = pix.shape[0]
    sums = np.zeros((5, rows), dtype=np.int64)
    if rows == 0:
        return np.zeros(0, dtype=np.uint8), sums
    for t in TYPES:
        filt = png_model.filter_rows(pix, bpp, [t] * rows)
        sums[t] = cost(filt[:, 1:]).sum(axis=1)
    types = np.zeros(rows, dtype=np.uint8)
    for r in range(rows):
        best = 0
        for t in TYPES[1:]:
            if int(sums[t, r]) < int(sums[best, r]):      # strictly smaller: a tie keeps the lower number
                best = t
        types[r] = best
    return types, sums


def tied(sums):
    """bool [rows]: the minimum is reached by more than one type."""
    return (sums == sums.min(axis=0)).sum(axis=0) > 1


# ---- the images the selection tests share ----

# png_model.DATA_KINDS, then images on which each type should win:
#   "noise"   small signed values around 0 (0, 1, 2, 254, 255 ...): None
#   "hramp"   every row its own ramp along x (own offset, own small slope): Sub
#   "vramp"   every column its own ramp down the rows: Up
#   "diag"    one gradient in x and y plus 0 / 1 noise: Average / Paeth
#   "from1" .. "from4"  the image whose type-t residuals are small noise (reconstructed from them)
KINDS = png_model.DATA_KINDS + ("noise", "hramp", "vramp", "diag", "uniform", "from1", "from2", "from3", "from4")


_BASE = {}


def _from_residuals(t, rows, rb, bpp):
    """Reconstruction of small residuals under type t, in numpy (row by row, pixel by pixel for the
    types that look left: short loops, no reference to any filter code but png_model.predictor).
    One fixed image per (t, rb, bpp), made once: its first `rows` rows."""
    if (t, rb, bpp) not in _BASE:
        _BASE[(t, rb, bpp)] = _reconstruct(np.random.default_rng(1000 * t + 10 * bpp + rb), t, max(ROWS), rb, bpp)
    return _BASE[(t, rb, bpp)][:rows]


def _reconstruct(r, t, rows, rb, bpp):
    res = r.integers(-2, 3, (rows, rb)).astype(np.int32)
    out = np.zeros((rows + 1, rb + bpp), dtype=np.int32)     # a zero row above, zero pixels to the left
    for y in range(rows):
        cur, up = out[y + 1], out[y]
        if t == 2:
            cur[bpp:] = (res[y] + up[bpp:]) & 0xFF
            continue
        for x in range(0, rb, bpp):                          # one pixel at a time: its bytes do not depend on each other
            w = min(bpp, rb - x)
            a, b, c = cur[x:x + w], up[bpp + x:bpp + x + w], up[x:x + w]
            cur[bpp + x:bpp + x + w] = (res[y, x:x + w] + png_model.predictor(t, a, b, c)) & 0xFF
    return out[1:, bpp:].astype(np.uint8)


def image(r, kind, rows, rb, bpp):
    """uint8 [rows, rb]."""
    if kind in png_model.DATA_KINDS:
        return png_model.pixels(r, kind, rows * rb).reshape(rows, rb)
    x = np.arange(rb, dtype=np.int64)[None, :] // bpp
    y = np.arange(rows, dtype=np.int64)[:, None]
    if kind == "noise":
        v = r.integers(-2, 3, (rows, rb))
    elif kind == "hramp":
        v = r.integers(0, 256, (rows, 1)) + r.integers(1, 4, (rows, 1)) * x
    elif kind == "vramp":
        v = r.integers(0, 256, (1, rb)) + r.integers(1, 4, (1, rb)) * y
    elif kind == "diag":
        v = 3 * x + 5 * y + r.integers(0, 2, (rows, rb))
    elif kind.startswith("from"):
        # the serial reconstruction is slow in Python: wide images repeat a 256-byte-wide one with a jump at every seam
        w = min(rb, 256 // bpp * bpp)
        assert rows <= max(ROWS)
        base = _from_residuals(int(kind[4:]), rows, w, bpp).astype(np.int64)
        reps = (rb + w - 1) // w
        v = np.concatenate([base + 16 * k for k in range(reps)], axis=1)[:, :rb] + int(r.integers(0, 256))
    else:
        raise ValueError(kind)
    return (v & 0xFF).astype(np.uint8).reshape(rows, rb)


def choose_images(r, rb, bpp, rows=ROWS, shift=0):
    """The shared input set at one width: image i of rows[i] rows and kind KINDS[(i + shift) % len(KINDS)]."""
    return [image(r, KINDS[(i + shift) % len(KINDS)], nr, rb, bpp) for i, nr in enumerate(rows)]
