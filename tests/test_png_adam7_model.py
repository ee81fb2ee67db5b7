"""tests/png_adam7_model.py -- the referee of fdh_png_adam7_size and fdh_png_unfilter_interlaced_batch and the writer
of the tests' interlaced files -- against references that share nothing with it: Pillow's reader, which decodes Adam7
files of all fifteen depth / colour pairs (it cannot write them: save(interlace=1) gives a progressive file), the
specification's 8 x 8 pass pattern and worked sizes as literals.  Also the host arithmetic of png_adam7_size and the
CPU-side check that the library declares and exports the new entry points.
"""
import io
import os
import re
import zlib

import numpy as np
import pytest

import png_adam7_model as am
import png_expand_model as em
import png_file_model as fm
from png_corpus import CLASSES, adam7_file, clear_padding, cycling_types, pillow_rgba, pre_chunks, random_case

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdh_png_adam7_size", "fdh_png_unfilter_interlaced_batch")
WIDTHS = tuple(range(1, 10)) + (17, 33)
HEIGHTS = tuple(range(1, 10))


@pytest.mark.parametrize("cls", CLASSES, ids=["depth%d-colour%d%s" % (d, c, "-trns" if k else "") for d, c, k in CLASSES])
def test_model_written_files_against_pillow(cls):
    """Model-written Adam7 files of the 22 classes on which Pillow follows the specification, every width of 1 .. 9, 17,
    33 at every height of 1 .. 9, the filter types cycling through all five from the first row of every pass on.
    Pillow reports interlace 1; its RGBA picture is the model's expansion of the model's own decode of the file; and
    where Pillow leaves the samples untouched (depth 8, palette indices, one-bit grey) they are the picture's samples
    one by one."""
    depth, colour, keyed = cls
    r = np.random.default_rng(8200 + 64 * colour + depth + (1000 if keyed else 0))
    ch = fm.CHANNELS[colour]
    shift = 0
    for width in WIDTHS:
        for height in HEIGHTS:
            pix, key, pal = random_case(r, width, height, depth, colour, keyed)
            pix = clear_padding(pix, width, height, depth, colour)
            shift += 1
            png = adam7_file(pix, width, height, depth, colour, cycling_types(width, height, shift), pre_chunks(colour, key, pal))
            im = Image.open(io.BytesIO(png))
            im.load()
            assert im.info.get("interlace") == 1 and im.size == (width, height), (cls, width, height)
            got = am.decode(png)
            assert got == (width, height, depth, colour, pix.tobytes()), (cls, width, height)
            rgba, st = em.expand(got[4], width, depth, colour, key, pal)
            assert st == 0 and rgba == pillow_rgba(png), (cls, width, height)
            if depth == 8 or colour == 3 or (depth, colour) == (1, 0):
                rb = fm.geometry(width, depth, colour)[0]
                want = [s for y in range(height) for s in em.samples(got[4][y * rb:(y + 1) * rb], width, depth, ch)]
                assert np.asarray(im).astype(np.int64).reshape(-1).tolist() == want, (cls, width, height)


def test_the_specifications_pass_pattern():
    """PNG specification 8.2, the 8 x 8 pattern of pass numbers, as a literal: a picture whose pixel values are the
    pass numbers interlaces to seven constant images."""
    pattern = [[1, 6, 4, 6, 2, 6, 4, 6],
               [7, 7, 7, 7, 7, 7, 7, 7],
               [5, 6, 5, 6, 5, 6, 5, 6],
               [7, 7, 7, 7, 7, 7, 7, 7],
               [3, 6, 4, 6, 3, 6, 4, 6],
               [7, 7, 7, 7, 7, 7, 7, 7],
               [5, 6, 5, 6, 5, 6, 5, 6],
               [7, 7, 7, 7, 7, 7, 7, 7]]
    for width, height in ((8, 8), (16, 24), (13, 11)):
        pix = bytes(pattern[y % 8][x % 8] for y in range(height) for x in range(width))
        images = am.interlace(pix, width, height, 8, 0)
        for p, (pw, ph) in enumerate(am.passes(width, height)):
            assert images[p] == bytes([p + 1]) * (pw * ph), (width, height, p)
    assert am.passes(8, 8) == [(1, 1), (1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4)]
    assert am.passes(1, 1) == [(1, 1)] + [(0, 0)] * 6
    assert am.passes(4, 9) == [(1, 2), (0, 0), (1, 1), (1, 3), (2, 2), (2, 5), (4, 4)]


def test_interlace_there_and_back_and_size():
    """deinterlace(interlace(x)) == x for every pair at widths and heights that empty every combination of passes, and
    size() is the length of what the writer filters."""
    r = np.random.default_rng(8300)
    for depth, colour in fm.PAIRS:
        for width in WIDTHS:
            for height in HEIGHTS + (17,):
                rb = fm.geometry(width, depth, colour)[0]
                pix = clear_padding(r.integers(0, 256, height * rb, dtype=np.uint8), width, height, depth, colour).tobytes()
                images = am.interlace(pix, width, height, depth, colour)
                assert am.deinterlace(images, width, height, depth, colour) == pix, (depth, colour, width, height)
                types = cycling_types(width, height, width + height)
                stream = am.filter_passes(images, width, height, depth, colour, types)
                assert len(stream) == am.size(width, height, depth, colour), (depth, colour, width, height)
                assert am.unfilter_passes(stream, width, height, depth, colour) == images


def test_worked_sizes():
    assert am.size(341, 64, 8, 2) == 65592 and 64 * (1 + 341 * 3) == 65536
    assert am.size(8, 8, 1, 0) == 30
    assert am.size(1, 9, 8, 0) == 18 == 9 * (1 + 1)
    assert am.size(0, 5, 8, 0) == 0 and am.size(5, 0, 8, 0) == 0 and am.size(5, 5, 4, 2) == 0 and am.size(5, 5, 16, 3) == 0


def test_the_first_row_of_a_pass_has_zeros_above_it():
    """A file whose every row is of type Up: a reader that took the last row of the pass before as "above" would add
    it; the model's decode and Pillow's do not."""
    width, height = 9, 9
    pix = np.arange(1, 1 + width * height, dtype=np.uint8)
    png = adam7_file(pix, width, height, 8, 0, [2] * am.pass_rows(width, height))
    assert am.decode(png)[4] == pix.tobytes()
    assert np.asarray(Image.open(io.BytesIO(png))).reshape(-1).tolist() == pix.tolist()


def test_scan_with_and_without_the_flag():
    pix = np.arange(35, dtype=np.uint8)
    png = adam7_file(pix, 7, 5, 8, 0, [0] * am.pass_rows(7, 5), pre=[(b"tEXt", b"a\0b")], idat_chunks=2)
    plain = fm.scan(am.write_file(am.stream_of(pix, 7, 5, 8, 0, [0] * am.pass_rows(7, 5)), 7, 5, 8, 0, [(b"tEXt", b"a\0b")], 2, zlib.crc32, method=0),
                    crc=zlib.crc32)
    off = am.scan(png, adam7=False, crc=zlib.crc32)
    assert off.status == fm.INTERLACED and off.chunks == 0 and off.interlace == 1
    on = am.scan(png, adam7=True, crc=zlib.crc32)
    assert on.status == 0 and on.interlace == 1
    assert on.fields()[1:5] + on.fields()[6:] == plain.fields()[1:5] + plain.fields()[6:] and plain.status == 0
    two = am.write_file(b"x", 7, 5, 8, 0, method=2, crc=zlib.crc32)
    assert am.scan(two, adam7=True, crc=zlib.crc32).status == fm.BAD_IHDR == am.scan(two, crc=zlib.crc32).status
    bad = bytearray(png)
    bad[40] ^= 1                                            # a byte of the tEXt behind the IHDR
    assert am.scan(bytes(bad), adam7=True, crc=zlib.crc32).status == fm.CRC_MISMATCH
    assert am.scan(bytes(bad), adam7=False, crc=zlib.crc32).status == fm.INTERLACED


# ---- the library ----

def test_png_adam7_size_is_the_models():
    """api.png_adam7_size -- host arithmetic, ints and numpy heights -- and the library's fdh_png_adam7_size equal the
    model over the widths and heights above, and give the three worked values."""
    import fdeflate_amd as fd
    from fdeflate_amd import _lib
    L = _lib.lib()
    heights = np.array(HEIGHTS + (17, 64, 513), dtype=np.int64)
    for depth, colour in fm.PAIRS:
        for width in WIDTHS + (341,):
            want = [am.size(width, int(h), depth, colour) for h in heights]
            got = fd.png_adam7_size(width, heights, depth, colour)
            assert isinstance(got, np.ndarray) and got.tolist() == want, (depth, colour, width)
            assert [fd.png_adam7_size(width, int(h), depth, colour) for h in heights] == want
            assert [L.fdh_png_adam7_size(width, int(h), depth, colour) for h in heights] == want
    for f in (fd.png_adam7_size, L.fdh_png_adam7_size):
        assert (f(341, 64, 8, 2), f(8, 8, 1, 0), f(1, 9, 8, 0)) == (65592, 30, 18)
        assert (f(0, 5, 8, 0), f(5, 0, 8, 0), f(5, 5, 4, 2), f(5, 5, 16, 3), f(5, 5, 8, 1)) == (0, 0, 0, 0, 0)
    assert fd.png_adam7_size(5, np.array([0, 3]), 8, 0).tolist() == [0, am.size(5, 3, 8, 0)]
    assert L.fdh_png_adam7_size(0x7FFFFFFF, 1 << 20, 16, 6) == am.size(0x7FFFFFFF, 1 << 20, 16, 6) > 1 << 53     # (64-bit arithmetic)


def test_header_declares_and_library_exports_the_adam7_calls():
    from fdeflate_amd import _lib
    import fdeflate_amd as fd
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    assert re.search(r"#define\s+FDH_PNG_FLAG_ADAM7\s+0x2u", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fdh_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "not declared: " + s
        assert hasattr(L, s), "not exported: " + s
        assert s in _lib.EXPORTED_SYMBOLS
    assert fd.PNG_FLAG_ADAM7 == 2 and fd.PNG_FLAG_IGNORE_CRC == 1
    for name in ("PNG_FLAG_ADAM7", "png_adam7_size", "png_unfilter_interlaced_batch"):
        assert name in fd.__all__ and hasattr(fd, name)
    assert "PNG_FLAG_ADAM7" in fd.png_decode_files_batch.__doc__ and "PNG_FLAG_ADAM7" in fd.png_decode_files_rgba_batch.__doc__


def test_the_new_call_refuses_bad_geometry_before_it_needs_a_device():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for width, depth, colour, word in ((0, 8, 2, b"width"), (1 << 31, 8, 2, b"width"), (5, 3, 0, b"fifteen"), (5, 16, 3, b"fifteen"),
                                      (5, 4, 2, b"fifteen"), (5, 8, 1, b"fifteen")):
        assert L.fdh_png_unfilter_interlaced_batch(None, None, None, None, None, None, None, None, 1, width, depth, colour, None) == 1
        assert word in L.fdh_last_error()
    for depth, colour in fm.PAIRS:
        assert L.fdh_png_unfilter_interlaced_batch(None, None, None, None, None, None, None, None, 1, 5, depth, colour, None) == 1
        assert b"null pointer" in L.fdh_last_error()
        assert L.fdh_png_unfilter_interlaced_batch(None, None, None, None, None, None, None, None, 0, 5, depth, colour, None) == 0
