"""tests/png_expand_model.py -- the referee of fdh_png_colour_batch and fdh_png_expand_batch -- against two references
that share nothing with it: Pillow's reader (Image.open(..).convert("RGBA")) and expected bytes written out by hand.
Also the CPU-side check that the library declares and exports the new entry points.  The cases (random_case,
status_files) come from tests/png_corpus.py, which the GPU tests share.

Pillow is compared on 22 classes: all fifteen depth / colour pairs without tRNS, and with tRNS the palette at depths
1, 2, 4 and 8, grey at depths 1 and 8 and RGB at depth 8.  Four classes are NOT compared with Pillow, because Pillow
12 departs from the specification there: a grey key at depths 2 and 4 (it compares after scaling the samples to eight
bits, so the key never matches the raw sample), a grey key at depth 16 (mode I;16: convert("RGBA") does not apply the
key at all) and an RGB key at depth 16 (it compares the truncated high bytes, so samples that differ from the key in
their low byte only become transparent).  The specification (11.3.2.1) compares the raw samples: those four classes are
checked against literal bytes below.
"""
import os
import re
import zlib

import numpy as np
import pytest

import png_expand_model as em
import png_file_model as fm
from png_corpus import CLASSES, LEFT_OUT, pillow_rgba, pre_chunks, random_case, status_files, stream_of

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdh_png_colour_batch", "fdh_png_expand_batch")
WIDTHS = (1, 3, 7, 8, 9, 33)


@pytest.mark.parametrize("cls", CLASSES, ids=["depth%d-colour%d%s" % (d, c, "-trns" if k else "") for d, c, k in CLASSES])
def test_model_against_pillow(cls):
    """The 22 classes on which Pillow follows the specification, at widths either side of a byte of 1-bit pixels and a
    lane's four pixels: the model's RGBA bytes are Pillow's."""
    depth, colour, keyed = cls
    assert not (keyed and (depth, colour) in LEFT_OUT)
    r = np.random.default_rng(7100 + 64 * colour + depth + (1000 if keyed else 0))
    for width in WIDTHS:
        height = 5
        pix, key, pal = random_case(r, width, height, depth, colour, keyed)
        rb = fm.geometry(width, depth, colour)[0]
        png = em.write_file(stream_of(pix, rb), width, height, depth, colour, pre_chunks(colour, key, pal), crc=zlib.crc32)
        info = fm.scan(png, crc=zlib.crc32)
        st, got_pal, got_key = em.read_colour(png, info, width, depth, colour)
        assert (st, got_pal, got_key) == (0, pal, key), (cls, width)
        rgba, status = em.expand(pix, width, depth, colour, key, pal)
        assert status == 0 and len(rgba) == width * height * 4
        assert rgba == pillow_rgba(png), (cls, width)
        if keyed:
            assert 0 in rgba[3::4] or colour == 3, (cls, width)


def test_left_out_classes_against_literal_bytes():
    """The four classes Pillow does not follow the specification on: the key is compared on the raw sample."""
    # 2-bit grey 0, 1, 2, 3 with key 2
    rgba, st = em.expand(bytes([0b00011011]), 4, 2, 0, key=(2,))
    assert st == 0 and rgba == bytes([0, 0, 0, 255, 85, 85, 85, 255, 170, 170, 170, 0, 255, 255, 255, 255])
    # 4-bit grey 0, 1, 2, 3 with key 2
    rgba, st = em.expand(bytes([0x01, 0x23]), 4, 4, 0, key=(2,))
    assert st == 0 and rgba == bytes([0, 0, 0, 255, 17, 17, 17, 255, 34, 34, 34, 0, 51, 51, 51, 255])
    # a key wider than the depth is masked (libpng writes 16-bit values whatever the depth)
    assert em.expand(bytes([0b00011011]), 4, 2, 0, key=(0xFF02,))[0][3::4] == bytes([255, 255, 0, 255])
    # 16-bit grey 0x1234, 0x1235 with key 0x1234
    rgba, st = em.expand(bytes([0x12, 0x34, 0x12, 0x35]), 2, 16, 0, key=(0x1234,))
    assert st == 0 and rgba == bytes([0x12, 0x12, 0x12, 0, 0x12, 0x12, 0x12, 255])
    # 16-bit RGB: the key, then the key with one sample differing in its low byte only, each sample in turn
    key = (0x0102, 0x0304, 0x0506)
    px = [key, (0x0103, 0x0304, 0x0506), (0x0102, 0x0305, 0x0506), (0x0102, 0x0304, 0x0507)]
    rgba, st = em.expand(b"".join(em.trns_body(p) for p in px), 4, 16, 2, key=key)
    assert st == 0 and rgba == bytes([1, 3, 5, 0, 1, 3, 5, 255, 1, 3, 5, 255, 1, 3, 5, 255])
    # padding bits behind the last pixel are ignored: width 3 at depth 2, the last two bits set
    assert em.expand(bytes([0b00011011]), 3, 2, 0)[0] == bytes([0, 0, 0, 255, 85, 85, 85, 255, 170, 170, 170, 255])


def test_reader_statuses():
    """One file per status of fdh_png_colour_batch, each way to get 10 and 11, and the tolerated cases; on the sound
    files the palette and the key are the chunks' own."""
    seen = set()
    for what, f, (width, depth, colour), want, pix in status_files():
        info = fm.scan(f, crc=zlib.crc32)
        assert (info.status != 0) == (want == 3), what
        st, pal, key = em.read_colour(f, info, width, depth, colour)
        assert st == want, (what, st)
        seen.add(st)
        if st == 0 and what == "sound palette":
            assert pal == [(0, 1, 2, 9), (3, 4, 5, 8), (6, 7, 8, 7), (9, 10, 11, 255)] and key is None
            assert em.pal_words(pal)[:5] == [0x09020100, 0x08050403, 0x07080706, 0xFF0B0A09, 0xFF000000]
            assert em.colour_words(4, None) == [4, 0, 0, 0]
        if what == "sound RGB key":
            assert key == (0x1234, 5, 0xFFFE) and em.colour_words(0, key) == [0, 1, 0x1234 | 5 << 16, 0xFFFE]
        if what.startswith("tolerated: tRNS") or what == "tolerated: PLTE with RGB":
            assert pal is None and key is None
        if what == "tolerated: PLTE with grey, behind its key":
            assert key == (0x21,)
        if st == 0 and colour != 3:
            assert pillow_rgba(f) == em.expand(pix, width, depth, colour, key, pal)[0] or (depth, colour) in LEFT_OUT, what
    assert seen == {0, 3, 7, 10, 11}


def test_index_outside_the_palette():
    """Status 9: the pixel is (0, 0, 0, 255), the image is written in full, and a palette of 2^depth entries cannot
    give it."""
    pal = em.palette(bytes(range(10, 19)), bytes([1, 2]))       # three entries
    rgba, st = em.expand(bytes([0b00011011, 0b11100100]), 8, 2, 3, pal=pal)
    assert st == 9
    assert rgba == bytes([10, 11, 12, 1, 13, 14, 15, 2, 16, 17, 18, 255, 0, 0, 0, 255,
                          0, 0, 0, 255, 16, 17, 18, 255, 13, 14, 15, 2, 10, 11, 12, 1])
    assert em.expand(bytes([0b00011010]), 4, 2, 3, pal=pal) == (bytes([10, 11, 12, 1, 13, 14, 15, 2, 16, 17, 18, 255, 16, 17, 18, 255]), 0)
    # the padding bits of a row do not count: width 3, the fourth field is 3
    assert em.expand(bytes([0b00011011]), 3, 2, 3, pal=pal)[1] == 0


# ---- the library ----

def test_header_declares_and_library_exports_the_expand_calls():
    from fdeflate_amd import _lib
    import fdeflate_amd as fd
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fdh_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "not declared: " + s
        assert hasattr(L, s), "not exported: " + s
        assert s in _lib.EXPORTED_SYMBOLS
    assert (fd.PNG_INDEX_OUTSIDE_PALETTE, fd.PNG_BAD_PLTE, fd.PNG_BAD_TRNS) == (9, 10, 11)
    assert callable(fd.png_decode_files_rgba_batch) and "png_decode_files_rgba_batch" in fd.png_decode_files_batch.__doc__


def test_expand_refuses_bad_geometry_before_it_needs_a_device():
    """An illegal pair or width: FDH_ERR_INVALID_ARGUMENT with a message, with or without a GPU; a legal pair gets as
    far as the null pointers."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for width, depth, colour, word in ((0, 8, 2, b"width"), (1 << 31, 8, 2, b"width"), (5, 3, 0, b"fifteen"), (5, 16, 3, b"fifteen"),
                                      (5, 4, 2, b"fifteen"), (5, 8, 1, b"fifteen")):
        assert L.fdh_png_expand_batch(None, None, None, None, None, None, None, None, 1, width, depth, colour, None) == 1
        assert word in L.fdh_last_error()
        assert L.fdh_png_colour_batch(None, None, None, None, None, None, 1, width, depth, colour, None) == 1
        assert word in L.fdh_last_error()
    for depth, colour in fm.PAIRS:
        assert L.fdh_png_expand_batch(None, None, None, None, None, None, None, None, 1, 5, depth, colour, None) == 1
        assert b"null pointer" in L.fdh_last_error()
        assert L.fdh_png_colour_batch(None, None, None, None, None, None, 1, 5, depth, colour, None) == 1
        assert b"null pointer" in L.fdh_last_error()
