"""CPU-side checks of the mixed encode batches: tests/png_encode_mixed_model.py against the library's host arithmetic
(fdh_png_encode_plan_one through ctypes: no device), against values written out by hand, and its files against Pillow's
reader, on the classes where tests/test_png_expand_model.py says Pillow follows the specification (no tRNS but the
palette's)."""
import ctypes as C
import io

import numpy as np
import pytest

import png_encode_mixed_model as em
import png_file_model as fm
import png_mixed_model as mm
from png_corpus import kinds, pillow_rgba

BIT = {0: 1, 2: 4, 3: 8, 4: 16, 6: 64}


def lib_plan(r, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    import fdeflate_amd as fd
    return fd.png_encode_plan_one(r, count, trns_len, summary, analyse_status, allowed)


def both(r, **kw):
    want = em.plan(r, **kw)
    assert lib_plan(r, **kw) == want, (r, kw)
    return want


def summary(opaque, grey, depth):
    return (1 if opaque else 0) | (2 if grey else 0) | depth << 8


def test_the_symbol_is_exported_and_takes_null():
    from fdeflate_amd import _lib
    L = _lib.lib()
    sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.fdh_png_encode_plan_one(None, None, None, 0, 0, 0, sizes) == 3 and list(sizes) == [0, 0, 0, 0]
    assert lib_plan(mm.record(5, 7, 8, 6)) == (0, 8, 6, 140, 7, 41, 41 + em.ultrafast_bound(7 * 21) + 16)


def test_by_hand():
    """Values worked out on paper.  3 x 2 opaque grey at depth 2: a row is one byte.  Grey: 2.  Palette of 4 colours at
    depth 2: 2 + 12 + 12 = 26.  Grey-alpha: 12, RGB: 18, RGBA: 24."""
    r = mm.record(3, 2, 0, 0)
    s = summary(True, True, 2)
    assert em.plan(r, 4, 0, s) == (0, 2, 0, 2, 2, 41, 41 + em.ultrafast_bound(4) + 16)
    assert em.plan(r, 4, 0, s, allowed=BIT[3]) == (0, 2, 3, 2, 2, 41 + 24, 41 + 24 + em.ultrafast_bound(4) + 16)
    assert em.plan(r, 4, 0, s, allowed=BIT[3] | BIT[6])[1:4] == (8, 6, 24)      # 26 for the palette: its chunks lose
    assert em.plan(r, 4, 2, s & ~1, allowed=BIT[3])[5] == 41 + 24 + 14
    assert em.plan(r, 4, 0, s, allowed=BIT[4] | BIT[2] | BIT[6])[1:4] == (8, 4, 12)
    assert em.plan(r, 4, 0, s, allowed=BIT[2] | BIT[6])[1:4] == (8, 2, 18)
    assert em.plan(r, 4, 0, s, allowed=BIT[6])[1:4] == (8, 6, 24)
    assert em.ultrafast_bound(0) == 60 and em.ultrafast_bound(65536) == 98364


def test_grey_alpha_against_rgb_by_hand():
    """An opaque grey picture may be written as grey-alpha (2 bytes a pixel) or RGB (3): grey-alpha is cheaper."""
    r = mm.record(3, 2, 0, 0)
    assert em.plan(r, None, None, summary(True, True, 8), allowed=BIT[4] | BIT[2])[1:4] == (8, 4, 12)
    assert both(r, summary=summary(True, True, 8), allowed=BIT[2])[1:4] == (8, 2, 18)


@pytest.mark.parametrize("opaque", (False, True))
@pytest.mark.parametrize("grey", (False, True))
def test_summary_bits_depths_counts_and_masks(opaque, grey):
    """Every combination of the two summary bits with depths 1, 2, 4, 8, counts either side of every palette depth and
    overflow, trns_len 0, 1 and count, at sizes where each candidate can win; then every mask that removes the winner,
    until nothing is left (13)."""
    seen = set()
    for depth in (1, 2, 4, 8):
        for width, height in ((1, 1), (2, 2), (3, 5), (16, 16), (341, 64)):
            r = mm.record(width, height, 0, 0)
            for count in (1, 2, 3, 4, 5, 16, 17, 256, None):
                a_status = em.TOO_MANY_COLOURS if count is None else 0
                for trns in ((None,) if count is None else sorted({0, 1, count})):
                    if count is not None and (trns == 0) != opaque:
                        continue                # (a palette whose entries are all opaque belongs to an opaque picture)
                    kw = dict(count=count, trns_len=trns, summary=summary(opaque, grey, depth), analyse_status=a_status)
                    allowed = 0
                    while True:
                        st, d, c, pix, types, prefix, size = both(r, allowed=allowed, **kw)
                        if st != 0:
                            assert st == em.NOT_REPRESENTABLE and (pix, types, prefix, size) == (0, 0, 0, 0)
                            break
                        seen.add((c, d))
                        assert types == height and pix == height * em.row_bytes(width, d, c)
                        assert prefix == (41 if c != 3 else 41 + 12 + 3 * count + (12 + trns if trns else 0))
                        assert size == prefix + em.ultrafast_bound(height * (em.row_bytes(width, d, c) + 1)) + 16
                        allowed = (allowed or em.ALL_TYPES) & ~BIT[c]          # remove the winner
                        if allowed == 0:
                            break
    if opaque and grey:
        assert {(0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4)} <= seen, seen
    if not opaque and not grey:
        assert {(3, 1), (3, 2), (3, 4), (3, 8), (6, 8)} <= seen, seen


def test_ties_and_palettes_that_lose():
    """Equal cost: the lower colour type.  A 1 x 1 or 2 x 2 picture of two colours costs 1 or 2 bytes as grey-1 and as
    palette-1, but the palette's PLTE makes it lose even to RGBA; without grey the palette loses to RGB and RGBA on 1 x 1
    (3 and 4 bytes against 1 + 15) and 2 x 2 (12 and 16 against 2 + 18)."""
    for side in (1, 2):
        r = mm.record(side, side, 0, 0)
        assert both(r, count=2, trns_len=0, summary=summary(True, True, 1))[1:3] == (1, 0)
        assert both(r, count=2, trns_len=0, summary=summary(True, False, 1))[1:3] == (8, 2)
        assert both(r, count=2, trns_len=1, summary=summary(False, False, 1))[1:3] == (8, 6)
        assert both(r, count=2, trns_len=1, summary=summary(False, True, 1))[1:3] == (8, 4)
    # grey-8 and palette-8 rows are equally long: the chunks decide; grey-alpha 8 and grey 16 do not compete
    r = mm.record(100, 100, 0, 0)
    assert both(r, count=200, trns_len=0, summary=summary(True, True, 8))[1:3] == (8, 0)
    # the tie itself: no palette ties a grey of its own depth (its chunks are at least 15 bytes); one of a smaller depth
    # ties where height * (grey row - palette row) == 12 + 3 count.  Four greys at depth 4 (multiples of 17 that are not
    # multiples of 85): grey-4 against palette-2 at width 8 is 4 against 2 bytes a row, and 12 + 3 * 4 = 24 = 12 rows * 2
    r = mm.record(8, 12, 0, 0)
    s = summary(True, True, 4)
    grey = em.candidates(r, 4, 0, s, 0, BIT[0])
    palette = em.candidates(r, 4, 0, s, 0, BIT[3])
    assert grey == [(48, 0, 4)] and palette == [(48, 3, 2)]
    assert both(r, count=4, trns_len=0, summary=s)[1:3] == (4, 0)               # the lower colour type
    assert both(mm.record(8, 13, 0, 0), count=4, trns_len=0, summary=s)[1:3] == (2, 3)
    assert both(mm.record(8, 11, 0, 0), count=4, trns_len=0, summary=s)[1:3] == (4, 0)
    # RGB against the palette: 341 x 64 with 256 colours, 65472 against 21824 + 780
    assert both(mm.record(341, 64, 0, 0), count=256, trns_len=0, summary=summary(True, False, 8))[1:3] == (8, 3)


def test_encodable_records_keep_their_pair():
    for depth, colour in fm.PAIRS:
        r = mm.record(33, 7, depth, colour)
        if colour != 3:
            st, d, c, pix, types, prefix, size = both(r, summary=summary(False, False, 8), analyse_status=em.TOO_MANY_COLOURS)
            assert (st, d, c, prefix) == (0, depth, colour, 41) and pix == 7 * em.row_bytes(33, depth, colour)
            continue
        top = 1 << depth
        assert both(r)[0] == em.BAD_PLTE                                         # no arrays
        assert both(r, count=0, trns_len=0)[0] == em.BAD_PLTE
        assert both(r, count=top + 1, trns_len=0)[0] == em.BAD_PLTE
        assert both(r, count=top, trns_len=top + 1)[0] == em.BAD_TRNS
        assert both(r, count=1, trns_len=2)[0] == em.BAD_TRNS
        assert both(r, count=top, trns_len=top)[5] == 41 + 12 + 3 * top + 12 + top
        assert both(r, count=top, trns_len=0)[:3] == (0, depth, 3)
        assert both(r, count=0, trns_len=0, analyse_status=em.TOO_MANY_COLOURS)[0] == em.BAD_PLTE


def test_analyse_status_passes_through():
    for r in (mm.record(4, 4, 0, 0), mm.record(4, 4, 8, 2)):
        assert both(r, analyse_status=2)[0] == 2
        assert both(r, analyse_status=3)[0] == 3
        assert both(r, analyse_status=77)[0] == 77
        assert both(r, analyse_status=em.TOO_MANY_COLOURS)[0] == 0


def test_the_two_size_limits():
    """row_bytes of 2^25 (the chooser's limit) and height * (row_bytes + 1) of 2^31 (the fused encoder's): one below,
    at and above; nothing wraps at the largest sides."""
    for rb, want in ((em.ROW_LIMIT - 1, 0), (em.ROW_LIMIT, 2), (em.ROW_LIMIT + 1, 2)):
        st, _, _, pix, types, prefix, size = both(mm.record(rb, 1, 8, 0))
        assert st == want and (pix == rb if want == 0 else (pix, types, prefix, size) == (0, 0, 0, 0))
    # rb + 1 = 2^16: height 2^15 is the limit
    for height, want in (((1 << 15) - 1, 0), (1 << 15, 2), ((1 << 15) + 1, 2)):
        assert both(mm.record((1 << 16) - 1, height, 8, 0))[0] == want
    # a dimension record: the winner's sizes count (RGBA: 4 bytes a pixel)
    for width, want in (((1 << 23) - 1, 0), (1 << 23, 2)):
        assert both(mm.record(width, 1, 0, 0), summary=0, analyse_status=em.TOO_MANY_COLOURS)[0] == want
    assert both(mm.record(1 << 23, 1, 0, 0), summary=summary(True, True, 1), analyse_status=em.TOO_MANY_COLOURS)[:3] == (0, 1, 0)
    big = 0x7FFFFFFF
    for r in (mm.record(big, big, 16, 6), mm.record(big, big, 0, 0), mm.record(big, 1, 1, 0), mm.record(1, big, 1, 0)):
        assert both(r, count=2, trns_len=0, summary=summary(True, True, 1))[0] == 2


def test_records_of_neither_kind():
    bad = [mm.record(0, 4, 8, 6), mm.record(4, 0, 8, 6), mm.record(1 << 31, 4, 8, 6), mm.record(4, 1 << 31, 0, 0),
           mm.record(4, 4, 8, 6, interlace=1), mm.record(4, 4, 0, 0, interlace=1), mm.record(4, 4, 8, 6, status=5),
           mm.record(4, 4, 0, 0, status=1), mm.record(4, 4, 0, 2), mm.record(4, 4, 8, 0, interlace=2), mm.record(4, 4, 3, 0),
           mm.record(4, 4, 16, 3), mm.record(4, 4, 8, 1), mm.record(4, 4, 0, 3), mm.record(4, 4, 0, 6)]
    for r in bad:
        assert not em.encodable(r) and not em.dimension(r)
        assert both(r, count=1, trns_len=0, summary=summary(True, True, 1)) == (3, r["bit_depth"], r["colour_type"], 0, 0, 0, 0)
    assert em.dimension(mm.record(4, 4, 0, 0)) and not em.encodable(mm.record(4, 4, 0, 0)) and em.encodable(mm.record(4, 4, 1, 0))


def test_the_models_files_open_in_pillow():
    """Each of the five kinds the plan chooses, at every depth: the model's file has the planned pair in its IHDR, an
    exact PLTE / tRNS, and Pillow's convert("RGBA") gives the picture back."""
    from PIL import Image
    r = np.random.default_rng(12100)
    for width, height in ((37, 29), (64, 17)):
        for name, px, depth, colour in kinds(r, width, height):
            st, f, d, c = em.encode(px.tobytes(), width, height)
            assert (st, d, c) == (0, depth, colour), (name, st, d, c)
            info = fm.scan(f)
            assert (info.status, info.width, info.height, info.bit_depth, info.colour_type) == (0, width, height, depth, colour), name
            assert pillow_rgba(f) == px.tobytes(), name
            im = Image.open(io.BytesIO(f))
            if colour == 3:
                count = len(set(px.view(np.uint32).tolist()))
                assert len(im.palette.palette) == 3 * count, name        # no padding entries
    # a forced pair, and a picture the forced pair cannot hold
    px = kinds(r, 9, 5)[0][1]
    st, f, d, c = em.encode(px.tobytes(), 9, 5, pair=(16, 6))
    assert (st, d, c) == (0, 16, 6) and pillow_rgba(f) == px.tobytes()
    assert em.encode(kinds(r, 9, 5)[10][1].tobytes(), 9, 5, pair=(8, 0))[0] == em.NOT_REPRESENTABLE
    assert em.encode(kinds(r, 40, 40)[10][1].tobytes(), 40, 40, pair=(8, 3))[0] == em.TOO_MANY_COLOURS
    assert em.encode(px.tobytes(), 9, 4)[0] == em.BAD_SIZES
