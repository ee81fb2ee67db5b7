"""The oracle's PNG filters against an implementation that shares nothing with it: Pillow's PNG
decoder and encoder (C, libImaging), and against tests/png_model.py, the specification's formulas in
plain integers.  The GPU kernels are pinned bit-exact to the oracle (tests/test_gpu_png.py); a
misreading of the Paeth tie order or of the Average rounding that the oracle's filter and unfilter
shared would pass every round trip, and the kernels would then be bit-exact with a wrong reference.
"""
import io
import struct
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_model

Image = pytest.importorskip("PIL.Image")

# (name, PNG colour type, bit depth, bytes per pixel, Pillow mode after decoding)
MODES = (
    ("L8", 0, 8, 1, "L"),
    ("LA8", 4, 8, 2, "LA"),
    ("L16", 0, 16, 2, "I;16"),
    ("RGB8", 2, 8, 3, "RGB"),
    ("RGBA8", 6, 8, 4, "RGBA"),
    ("RGB16", 2, 16, 6, "RGB"),
    ("RGBA16", 6, 16, 8, "RGBA"),
)
ROWS = 6


def _widths(bpp):
    """Pixels per row: one pixel, a row below 16 bytes, rows either side of 1 KiB and of 4 KiB, the
    1366-pixel row of a laptop screen, and a row well above 4 KiB."""
    w = {1, max(1, 15 // bpp), 1024 // bpp, 1024 // bpp + 1, 4096 // bpp, 4096 // bpp + 1, 1366, 5760 // bpp + 1}
    return sorted(w)


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def _png(width, height, colour_type, depth, filtered):
    """A PNG file by hand: signature, IHDR, one IDAT holding the zlib stream of `filtered`, IEND."""
    ihdr = struct.pack(">IIBBBBB", width, height, depth, colour_type, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(filtered, 1)) + _chunk(b"IEND", b"")


def _pillow_pixels(png, mode):
    """Pillow's pixels in PNG byte order: every byte of an 8-bit or 16-bit grey image, the high byte
    of every sample of 16-bit RGB / RGBA (Pillow keeps no more of those)."""
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == mode, (im.mode, mode)
    raw = im.tobytes()
    if mode == "I;16":   # little-endian in Pillow, big-endian in the file
        raw = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 2)[:, ::-1].tobytes()
    return raw


def _cases(bpp):
    """(width, data kind or "filtered", type pattern).  Kind "filtered" draws the FILTERED bytes at
    random (any byte string with valid type bytes is a PNG image): reconstruction alone, on values no
    filter produced."""
    for width in _widths(bpp):
        for kind in png_model.DATA_KINDS + ("filtered",):
            for pattern in png_model.TYPE_PATTERNS:
                yield width, kind, pattern


N_DECODE_CASES = sum(len(list(_cases(m[3]))) for m in MODES)


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_oracle_unfilter_and_filter_against_pillow_decoder(mode):
    """Hand-assembled PNGs through Pillow's decoder.  For every case: the oracle's reconstruction
    equals Pillow's pixels; where the image was filtered by the oracle, Pillow gives the source
    pixels back (so the oracle's FILTER is right, not merely the inverse of its unfilter); and
    png_model agrees with the oracle in both directions.

    8-bit modes and 16-bit grey compare every byte.  Pillow reduces 16-bit RGB / RGBA to 8 bits per
    sample, the high byte: for bpp 6 and 8 every other byte (the even ones) is compared with Pillow,
    all of them with png_model."""
    name, colour_type, depth, bpp, pil_mode = mode
    r = np.random.default_rng(1000 + bpp * 16 + depth)
    stride = 2 if (depth == 16 and colour_type != 0) else 1
    ran = 0
    for width, kind, pattern in _cases(bpp):
        rb = width * bpp
        types = png_model.row_types(r, pattern, ROWS)
        what = (name, width, kind, pattern)
        if kind == "filtered":
            f = r.integers(0, 256, (ROWS, rb + 1), dtype=np.uint8)
            f[:, 0] = types
            filt, pix = f.tobytes(), None
        else:
            pix = png_model.pixels(r, kind, ROWS * rb).tobytes()
            st, filt = ob.png_filter(pix, rb, bpp, bytes(types))
            assert st == 0, what
            model = png_model.filter_rows(np.frombuffer(pix, dtype=np.uint8).reshape(ROWS, rb), bpp, types)
            assert model.tobytes() == filt, what
        st, got = ob.png_unfilter(filt, rb, bpp)
        assert st == 0, what
        if pix is not None:
            assert got == pix, what
        ref = _pillow_pixels(_png(width, ROWS, colour_type, depth, filt), pil_mode)
        assert len(ref) * stride == len(got), what
        assert got[::stride] == ref, what
        # the serial restatement: every byte, on the narrow rows and on one kind of the wide ones
        if rb <= 1100 or kind in ("small", "filtered"):
            assert png_model.unfilter(filt, rb, bpp) == got, what
        ran += 1
    assert ran == len(list(_cases(bpp)))


def test_decode_case_count():
    """The number the commit message reports."""
    assert N_DECODE_CASES == sum(len(_widths(m[3])) for m in MODES) * 5 * 7
    print("oracle vs Pillow decoder: %d cases" % N_DECODE_CASES)


def _idat(png):
    """The inflated IDAT data and (width, height, depth, colour type) of a PNG file."""
    pos, idat, ihdr = 8, b"", None
    while pos < len(png):
        n, tag = struct.unpack(">I4s", png[pos:pos + 8])
        body = png[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) & 0xFFFFFFFF == struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])[0]
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert ihdr[4:] == (0, 0, 0)   # deflate, filter method 0, not interlaced
    return zlib.decompress(idat), ihdr[:4]


def _pillow_sources():
    r = np.random.default_rng(77)
    x = np.arange(1366, dtype=np.int64)[None, :, None]
    y = np.arange(64, dtype=np.int64)[:, None, None]
    ch = np.arange(4, dtype=np.int64)[None, None, :]
    smooth = ((x * (ch + 1) + y * 3 + (x * y) // 64) & 0xFF).astype(np.uint8)          # gradients
    noise = r.integers(0, 256, (64, 1366, 4), dtype=np.uint8)
    mixed = smooth.copy()
    mixed[16:32] = noise[16:32]
    mixed[40:48] = (smooth[40:48] & 0xF0) | (noise[40:48] & 3)
    flat = np.zeros((64, 1366, 4), dtype=np.uint8)
    flat[::2] = smooth[::2]
    for name, a in (("smooth", smooth), ("noise", noise), ("mixed", mixed), ("flat", flat)):
        yield name + "-rgba", "RGBA", a
        yield name + "-rgb", "RGB", a[:, :, :3]
        yield name + "-rgb-narrow", "RGB", a[:, :341, :3]     # 1023-byte rows


def test_oracle_against_pillow_encoder():
    """PNGs written by Pillow (which chooses a filter per row): the oracle reconstructs the source
    pixels from Pillow's IDAT data, and the oracle's filter with the types Pillow chose gives
    Pillow's filtered bytes.  Between them the files use at least three filter types."""
    seen = set()
    n = 0
    for name, mode, a in _pillow_sources():
        a = np.ascontiguousarray(a)
        bpp = a.shape[2]
        assert len(mode) == bpp
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG", compress_level=1)
        filt, (w, h, depth, colour_type) = _idat(buf.getvalue())
        assert (w, h, depth) == (a.shape[1], a.shape[0], 8) and colour_type == {3: 2, 4: 6}[bpp], name
        rb = w * bpp
        assert len(filt) == h * (rb + 1), name
        types = filt[::rb + 1]
        seen |= set(types)
        assert ob.png_unfilter(filt, rb, bpp) == (0, a.tobytes()), name
        assert ob.png_filter(a.tobytes(), rb, bpp, types) == (0, filt), name
        assert png_model.filter_rows(a.reshape(h, rb), bpp, types).tobytes() == filt, name
        n += 1
    assert len(seen) >= 3 and all(t <= 4 for t in seen), sorted(seen)
    print("oracle vs Pillow encoder: %d files, filter types %s" % (n, sorted(seen)))
