"""CPU-side checks of the RGBA16 mixed encode: tests/png16_encode_model.py against the expansion model (every pair packs
and expands back), against values worked out independently, against the library's host arithmetic
(fdh_png_encode16_plan_one through ctypes: no device), and its files against a route without device code (png_file_model,
zlib, png_model, png16_model.expand16) and against Pillow's reader."""
import numpy as np
import pytest

import png16_encode_cases as cases
import png16_encode_model as e16
import png16_model as m16
import png_encode_mixed_model as em
import png_file_model as fm
import png_mixed_model as mm
from png16_encode_cases import MASKS, check_in_pillow, host_route, plan_inputs, plan_records

BIT = {0: 1, 2: 4, 3: 8, 4: 16, 6: 64}


def pal_entries(pal, count):
    return [(w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24) for w in pal[:count]]


def expand_back(pix, width, depth, colour, pal=None, count=0):
    out, st = m16.expand16(pix, width, depth, colour, None, pal_entries(pal, count) if colour == 3 else None)
    assert st == 0
    return out


# ---- packing ----

@pytest.mark.parametrize("depth,colour", cases.PAIRS)
def test_every_pair_packs_and_expands_back(depth, colour):
    r = np.random.default_rng(16100 + 8 * depth + colour)
    for width, height in ((1, 1), (7, 3), (33, 2)):
        px, pal, count = cases.holds(r, width, height, depth, colour)
        pix, st = e16.pack16_any(px.tobytes(), width, depth, colour, pal, count)
        assert st == 0 and len(pix) == height * em.row_bytes(width, depth, colour)
        assert expand_back(pix, width, depth, colour, pal, count) == px.tobytes()


def test_every_reason_a_picture_is_not_representable():
    r = np.random.default_rng(16200)
    width, height = 9, 4
    for depth, colour in cases.NARROW_PAIRS:
        px, pal, count = cases.holds(r, width, height, depth, colour)
        for at in (0, 17, px.size - 1):                      # ONE sample whose bytes differ
            bad = px.copy()
            bad[at] ^= 0x0100
            assert e16.pack16_any(bad.tobytes(), width, depth, colour, pal, count) == (None, 13), (depth, colour, at)
    narrow_white = cases.widen(bytes([255] * (width * height * 4)))

    def status(px, depth, colour, pal=None, count=256):
        return e16.pack16_any(px.tobytes(), width, depth, colour, pal, count)[1]

    for depth in (8, 16):
        translucent = narrow_white.copy()
        translucent[4 * 5 + 3] = 0x7F7F                      # A != 65535, narrow: colour types 0 and 2 cannot hold it
        assert [status(translucent, depth, c) for c in (0, 2, 4, 6)] == [13, 13, 0, 0]
        coloured = narrow_white.copy()
        coloured[4 * 7 + 1] = 0x8080                         # G != R: colour types 0 and 4 cannot
        assert [status(coloured, depth, c) for c in (0, 2, 4, 6)] == [13, 0, 13, 0]
    low = narrow_white.copy()
    low[4 * 2:4 * 2 + 3] = 0xFE01                            # R == G == B, but the two bytes differ: 16 bits only
    assert [status(low, d, 0) for d in (1, 2, 4, 8, 16)] == [13, 13, 13, 13, 0]
    level = narrow_white.copy()
    level[4 * 3:4 * 3 + 3] = 257 * 0x33                      # a multiple of 17 that is not one of 85: depth 4, not 2 or 1
    assert [status(level, d, 0) for d in (1, 2, 4, 8, 16)] == [13, 13, 0, 0, 0]
    pal = [0xFFFFFFFF, 0xFF333333] + [0xFF000000] * 254
    assert status(level, 1, 3, pal, 2) == 0 and status(level, 1, 3, pal, 1) == 13          # a pixel outside the palette
    pal3 = [0xFF000000, 0xFF010101, 0xFF333333, 0xFFFFFFFF] + [0xFF000000] * 252
    assert status(level, 2, 3, pal3, 4) == 0 and status(level, 1, 3, pal3, 4) == 13        # an index depth 1 cannot hold


# ---- analysis ----

def test_depth_field_and_narrow_bit_at_every_sample_value():
    """The depth of a picture with R = G = B = s is the smallest d that has a d-bit sample which expands to s
    (png16_model.to16: the specification's exact scaling), and bit 2 is s % 257 == 0."""
    expands_to = {}
    for d in (16, 8, 4, 2, 1):
        for v in range(1 << d):
            expands_to[m16.to16(v, d)] = d              # (descending: the smallest depth is written last)
    for s in range(65536):
        summary = e16.summary16_of([(s, s, s, 65535)])
        assert summary >> 8 == expands_to[s], s
        assert bool(summary & e16.NARROW) == (s % 257 == 0), s
        assert summary & 3 == 3
    assert e16.summary16_of([]) == 7 | 1 << 8
    # the depth looks at R, G, B only, bits 0 and 1 at all 16 bits, bit 2 at alpha as well
    assert e16.summary16_of([(0, 0, 0, 0x1234)]) == e16.GREY | 1 << 8
    assert e16.summary16_of([(0xFFFF, 0xFFFF, 0xFFFE, 0xFFFF)]) == e16.OPAQUE | 16 << 8
    assert e16.summary16_of([(0x5555, 0xAAAA, 0, 0xFFFF)]) == e16.OPAQUE | e16.NARROW | 2 << 8
    assert e16.summary16_of([(0x1212, 0x1212, 0x1212, 0xFF00)]) == e16.GREY | 8 << 8


def test_analysis_of_narrow_pictures_is_the_high_bytes_analysis():
    import png_pack_model as pm
    r = np.random.default_rng(16300)
    for name, px, depth, colour in cases.kinds16(r, 23, 11):
        st, pal, count, trns, summary = e16.analyse16(px.tobytes(), 23)
        if depth == 16:
            assert (st, pal, count, trns) == (12, None, None, None) and not summary & e16.NARROW and summary >> 8 == 16, name
            assert summary & 3 == {0: 3, 2: 1, 4: 2, 6: 0}[colour], name
        else:
            assert (st, pal, count, trns, summary & ~e16.NARROW) == pm.analyse(e16.high_bytes(px.tobytes()), 23, 256) and summary & e16.NARROW, name
    assert e16.analyse16(bytes(8 * 5), 2)[0] == 2


# ---- the plan ----

def lib_plan16(r, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    from fdeflate_amd import png16_encode
    return png16_encode.png_encode16_plan_one(r, count, trns_len, summary, analyse_status, allowed)


def both(r, **kw):
    want = e16.plan16(r, **kw)
    assert lib_plan16(r, **kw) == want, (r, kw)
    return want


@pytest.mark.parametrize("allowed", MASKS)
def test_plan_against_the_library_over_records_summaries_counts_and_masks(allowed):
    seen = set()
    for r in plan_records():
        for summary, count, trns, a_status in plan_inputs():
            st, d, c = both(r, count=count, trns_len=trns, summary=summary, analyse_status=a_status, allowed=allowed)[:3]
            if st == 0:
                seen.add((d, c))
    if allowed == 0:
        assert seen == set(fm.PAIRS)


def test_plan_by_hand():
    """5 x 3, not narrow: grey-16 rows are 10 bytes, grey-alpha 20, RGB 30, RGBA 40; the analysis says 12 of every such
    picture, and that is no error.  The same summary with bit 2 is the RGBA8 plan's business."""
    r = mm.record(5, 3, 0, 0)
    size = lambda rb: 41 + em.ultrafast_bound(3 * (rb + 1)) + 16
    assert both(r, summary=3 | 16 << 8, analyse_status=12) == (0, 16, 0, 30, 3, 41, size(10))
    assert both(r, summary=2 | 16 << 8, analyse_status=12) == (0, 16, 4, 60, 3, 41, size(20))
    assert both(r, summary=1 | 16 << 8, analyse_status=12) == (0, 16, 2, 90, 3, 41, size(30))
    assert both(r, summary=0 | 16 << 8, analyse_status=12) == (0, 16, 6, 120, 3, 41, size(40))
    assert both(r, summary=3 | 8 << 8, analyse_status=12)[1:3] == (16, 0)          # (bit 2 decides, not the depth field)
    assert both(r, summary=3 | 16 << 8, analyse_status=12, allowed=BIT[2] | BIT[4])[1:3] == (16, 4)
    assert both(r, summary=3 | 16 << 8, analyse_status=12, allowed=BIT[2] | BIT[3])[1:3] == (16, 2)
    assert both(r, summary=1 | 16 << 8, analyse_status=12, allowed=BIT[0] | BIT[3] | BIT[4])[0] == 13
    assert both(r, summary=3 | 16 << 8, analyse_status=12, allowed=BIT[3])[0] == 13
    assert both(r, summary=3 | 16 << 8, analyse_status=2)[0] == 2 and both(r, summary=0, analyse_status=77)[0] == 77
    assert both(r, count=2, trns_len=0, summary=7 | 1 << 8) == em.plan(r, 2, 0, 3 | 1 << 8)
    assert both(r, count=2, trns_len=0, summary=7 | 1 << 8)[1:3] == (1, 0)
    assert both(mm.record(5, 3, 8, 3), count=0, trns_len=0, summary=16 << 8, analyse_status=12)[0] == 10   # a forced palette pair
    # the size limits are the winner's: RGBA16 rows reach 2^25 bytes at width 2^22, grey-16 rows at 2^24
    assert both(mm.record((1 << 22) - 1, 1, 0, 0), summary=16 << 8, analyse_status=12)[:3] == (0, 16, 6)
    assert both(mm.record(1 << 22, 1, 0, 0), summary=16 << 8, analyse_status=12) == (2, 0, 0, 0, 0, 0, 0)
    assert both(mm.record(1 << 22, 1, 0, 0), summary=3 | 16 << 8, analyse_status=12)[:3] == (0, 16, 0)
    assert both(mm.record(0x7FFFFFFF, 0x7FFFFFFF, 0, 0), summary=16 << 8, analyse_status=12)[0] == 2       # nothing wraps


def test_bad_allowed_bits_are_the_batch_calls_business_and_null_is_taken():
    import ctypes as C
    from fdeflate_amd import _lib
    L = _lib.lib()
    sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.fdh_png_encode16_plan_one(None, None, None, 0, 0, 0, sizes) == 3 and list(sizes) == [0, 0, 0, 0]


# ---- files ----

def test_model_files_through_the_host_route_and_pillow():
    """Every kind the plan chooses, every forced pair on a picture it holds: the file carries the pair, comes back
    exactly through png_file_model / zlib / png_model / png16_model, and opens in Pillow."""
    r = np.random.default_rng(16400)
    chosen = set()
    for width, height in ((37, 29), (64, 17)):
        for name, px, depth, colour in cases.kinds16(r, width, height):
            st, f, d, c = e16.encode16(px.tobytes(), width, height)
            assert (st, d, c) == (0, depth, colour), (name, st, d, c)
            assert host_route(f) == (px.tobytes(), depth, colour), name
            check_in_pillow(f, px, width, height, depth, colour)
            chosen.add((depth, colour))
    assert chosen == set(fm.PAIRS)                               # no class is skipped
    for depth, colour in cases.PAIRS:
        px, _, _ = cases.holds(r, 13, 6, depth, colour)
        st, f, d, c = e16.encode16(px.tobytes(), 13, 6, pair=(depth, colour))
        assert (st, d, c) == (0, depth, colour)
        assert host_route(f) == (px.tobytes(), depth, colour)
        check_in_pillow(f, px, 13, 6, depth, colour)
    wide = cases.wide_picture(r, 13, 6, 6)
    assert e16.encode16(wide.tobytes(), 13, 6, pair=(8, 6))[0] == 13
    assert e16.encode16(wide.tobytes(), 13, 6, pair=(8, 3))[0] == 12
    assert e16.encode16(wide.tobytes(), 13, 6, pair=(16, 2))[0] == 13
    assert e16.encode16(wide.tobytes(), 13, 5)[0] == 2
