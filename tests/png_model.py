"""The five PNG filter types (PNG specification, 9.2 "Filter types for filter method 0" and 9.4
"Filter type 4: Paeth") written out in plain integer arithmetic, straight from the text and
independent of the oracle's C and of the HIP kernels: a third statement of the same rules, cheap
enough in numpy to give 2^24 expected values at once.

    x  the byte being filtered          a  the byte bpp to its left (0 in the first pixel)
    b  the byte above (0 in row 0)      c  the byte above a (0 in either case)

    0 None     Filt(x) = Orig(x)
    1 Sub      Filt(x) = Orig(x) - Orig(a)
    2 Up       Filt(x) = Orig(x) - Orig(b)
    3 Average  Filt(x) = Orig(x) - floor((Orig(a) + Orig(b)) / 2)      (the sum is NOT taken modulo 256)
    4 Paeth    Filt(x) = Orig(x) - PaethPredictor(Orig(a), Orig(b), Orig(c))

all modulo 256; reconstruction adds the same predictor of the RECONSTRUCTED neighbours.
"""
import numpy as np


def paeth(a, b, c):
    """PaethPredictor of the specification, on int32 arrays (or ints): p = a + b - c, the neighbour
    nearest to p, ties broken in the order a, b, c."""
    a, b, c = (np.asarray(v, dtype=np.int32) for v in (a, b, c))
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def predictor(t, a, b, c):
    a, b, c = (np.asarray(v, dtype=np.int32) for v in (a, b, c))
    if t == 0:
        return np.zeros_like(a)
    if t == 1:
        return a
    if t == 2:
        return b
    if t == 3:
        return (a + b) // 2
    if t == 4:
        return paeth(a, b, c)
    raise ValueError("filter type %d" % t)


def filter_rows(pix, bpp, types):
    """pix: uint8 [..., rows, row_bytes] (any number of images with the same shape and the same
    per-row types) -> uint8 [..., rows, 1 + row_bytes]: the type byte and the filtered bytes of
    every row.  Filtering uses the raw neighbours: every byte at once."""
    x = np.asarray(pix, dtype=np.uint8).astype(np.int32)
    rows, rb = x.shape[-2], x.shape[-1]
    assert len(types) == rows
    a = np.zeros_like(x)
    a[..., bpp:] = x[..., :rb - bpp] if rb > bpp else 0
    b = np.zeros_like(x)
    b[..., 1:, :] = x[..., :-1, :]
    c = np.zeros_like(x)
    c[..., 1:, :] = a[..., :-1, :]
    out = np.empty(x.shape[:-1] + (rb + 1,), dtype=np.uint8)
    for r, t in enumerate(types):
        out[..., r, 0] = t
        out[..., r, 1:] = ((x[..., r, :] - predictor(int(t), a[..., r, :], b[..., r, :], c[..., r, :])) & 0xFF).astype(np.uint8)
    return out


def unfilter(filt, row_bytes, bpp):
    """One image: bytes of rows x (1 + row_bytes) -> pixel bytes.  Reconstruction is serial along a
    row for Sub / Average / Paeth: those rows are walked byte by byte in Python integers."""
    f = np.frombuffer(bytes(filt), dtype=np.uint8)
    assert f.size % (row_bytes + 1) == 0
    rows = f.size // (row_bytes + 1)
    f = f.reshape(rows, row_bytes + 1)
    out = np.zeros((rows, row_bytes), dtype=np.uint8)
    up = [0] * row_bytes
    for r in range(rows):
        t = int(f[r, 0])
        line = f[r, 1:].tolist()
        cur = [0] * row_bytes
        for x in range(row_bytes):
            a = cur[x - bpp] if x >= bpp else 0
            b = up[x]
            c = up[x - bpp] if x >= bpp else 0
            if t == 0:
                pr = 0
            elif t == 1:
                pr = a
            elif t == 2:
                pr = b
            elif t == 3:
                pr = (a + b) // 2
            elif t == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pr = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                raise ValueError("filter type %d" % t)
            cur[x] = (line[x] + pr) & 0xFF
        out[r] = cur
        up = cur
    return out.tobytes()


# ---- the test data the PNG tests share ----

DATA_KINDS = ("random", "uniform", "small", "extreme")


def pixels(r, kind, n):
    """n pixel bytes: random; one constant byte; 0..3 (ties in Paeth and Average at every byte);
    0x00 / 0xFF (the largest differences, wrap-around in every predictor)."""
    if kind == "random":
        return r.integers(0, 256, n, dtype=np.uint8)
    if kind == "uniform":
        return np.full(n, int(r.integers(0, 256)), dtype=np.uint8)
    if kind == "small":
        return r.integers(0, 4, n, dtype=np.uint8)
    if kind == "extreme":
        return (r.integers(0, 2, n, dtype=np.uint8) * 0xFF).astype(np.uint8)
    raise ValueError(kind)


TYPE_PATTERNS = (0, 1, 2, 3, 4, "random", "4/3")


def row_types(r, pattern, rows):
    """Per-row filter types: one type alone, random types, or alternating Paeth / Average."""
    if pattern == "random":
        return r.integers(0, 5, rows, dtype=np.uint8)
    if pattern == "4/3":
        return np.where(np.arange(rows) % 2 == 0, 4, 3).astype(np.uint8)
    return np.full(rows, pattern, dtype=np.uint8)
