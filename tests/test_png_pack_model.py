"""tests/png_pack_model.py -- the referee of fdh_png_analyse_batch, fdh_png_pack_batch and fdh_png_frame_palette_batch --
against references that share nothing with it: tests/png_expand_model.py (itself pinned to Pillow and to literal
bytes), Pillow's reader on the model's files, Pillow's writer, and expected values written out by hand.  Also the
CPU-side check that the library declares and exports the new entry points.  The pictures (representable,
palette_image) come from tests/png_corpus.py, which the GPU tests share.
"""
import io
import os
import re
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_expand_model as em
import png_file_model as fm
import png_pack_model as pm
from png_corpus import palette_image, pillow_rgba, random_case, representable, stream_of

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdh_png_analyse_batch", "fdh_png_pack_batch", "fdh_png_palette_file_prefix", "fdh_png_frame_palette_batch")
WIDTHS = tuple(range(1, 10)) + (31, 32, 33)
PALETTE_DEPTHS = (1, 2, 4, 8)
CLASSES = [(d, c, False) for d, c in fm.PAIRS] + [(d, 3, True) for d in PALETTE_DEPTHS]
IDS = ["depth%d-colour%d%s" % (d, c, "-trns" if k else "") for d, c, k in CLASSES]


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_expand_of_pack_is_the_identity(pair):
    """Every pair at every width: expand(pack(x)) == x through png_expand_model.expand, the padding bits of every row
    are zero, and at depths up to 8 the packed bytes are the very rows x was expanded from (padding cleared)."""
    depth, colour = pair
    r = np.random.default_rng(9100 + 64 * colour + depth)
    for width in WIDTHS:
        height = 3
        rb = fm.geometry(width, depth, colour)[0]
        if colour == 3:
            x = palette_image(r, width, height, 1 << depth, 1)
            st, pal, count, _, _ = pm.analyse(x, width, 256)
            assert st == 0
            pix, st = pm.pack(x, width, depth, colour, pal, count)
            back = em.expand(pix, width, depth, colour, None, em.palette(*_plte_trns(pal, count)))
        else:
            src, _, _ = random_case(r, width, height, depth, colour, False)
            x = np.frombuffer(em.expand(src, width, depth, colour)[0], dtype=np.uint8)
            pix, st = pm.pack(x, width, depth, colour)
            back = em.expand(pix, width, depth, colour)
            if depth <= 8:
                want = src.reshape(height, rb).copy()
                pad = rb * 8 - width * fm.CHANNELS[colour] * depth
                want[:, -1] &= (0xFF << pad) & 0xFF
                assert pix == want.tobytes(), (pair, width)
        assert st == 0 and len(pix) == height * rb
        assert back == (x.tobytes(), 0), (pair, width)
        pad = rb * 8 - width * fm.CHANNELS[colour] * depth
        assert all(pix[(k + 1) * rb - 1] & ((1 << pad) - 1) == 0 for k in range(height)), (pair, width)


def _plte_trns(pal, count):
    own = pal[:count]
    return b"".join(bytes([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF]) for w in own), bytes(w >> 24 for w in own)


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_pillow_reads_the_models_files(cls):
    """All fifteen pairs, and the palette with tRNS at depths 1, 2, 4 and 8, at widths 1 .. 9 and 31 .. 33: the file
    around the model's packed rows -- png_expand_model.write_file, or write_palette_file with a PLTE of 2^depth entries
    -- opens in Pillow as the same RGBA."""
    depth, colour, trns = cls
    r = np.random.default_rng(9200 + 64 * colour + depth + (1000 if trns else 0))
    for width in WIDTHS:
        height = 4
        rb = fm.geometry(width, depth, colour)[0]
        if colour == 3:
            entries = 1 << depth
            x = palette_image(r, width, height, entries, entries // 2 if trns else 0)
            st, pal, count, trns_len, _ = pm.analyse(x, width, entries)
            assert st == 0 and (trns_len > 0) == trns
            pix, st = pm.pack(x, width, depth, colour, pal, count)
            png = pm.write_palette_file(stream_of(pix, rb), width, height, depth, pal, count, entries, entries if trns else 0, zlib.crc32)
            info = fm.scan(png, crc=zlib.crc32)
            got = em.read_colour(png, info, width, depth, 3)
            assert info.status == 0 and got[0] == 0 and em.pal_words(got[1])[:count] == pal[:count]
        else:
            x = representable(r, width, height, depth, colour)
            pix, st = pm.pack(x, width, depth, colour)
            png = em.write_file(stream_of(pix, rb), width, height, depth, colour, crc=zlib.crc32)
        assert st == 0
        assert pillow_rgba(png) == x.tobytes(), (cls, width)


@pytest.mark.parametrize("mode", ("RGB", "L", "LA", "RGBA"))
def test_pillows_writer_gives_the_models_packed_bytes(mode):
    """Image.fromarray(..).save of an RGB / L / LA / RGBA image: the file's IDAT stream, decoded and unfiltered, is the
    model's packing of the image's RGBA view."""
    colour = {"RGB": 2, "L": 0, "LA": 4, "RGBA": 6}[mode]
    ch = fm.CHANNELS[colour]
    r = np.random.default_rng(9300 + colour)
    for width in (1, 5, 32, 33):
        height = 7
        a = r.integers(0, 256, (height, width, ch), dtype=np.uint8)
        im = Image.fromarray(a[:, :, 0] if ch == 1 else a, mode)
        buf = io.BytesIO()
        im.save(buf, format="PNG")
        info = fm.scan(buf.getvalue(), crc=zlib.crc32)
        assert info.status == 0 and (info.width, info.height, info.bit_depth, info.colour_type) == (width, height, 8, colour)
        rb, bpp = fm.geometry(width, 8, colour)
        st, rows = ob.png_unfilter(zlib.decompress(info.idat), rb, bpp)
        assert st == 0
        assert pm.pack(im.convert("RGBA").tobytes(), width, 8, colour) == (rows, 0), (mode, width)


def test_sorted_palette_and_trns_len_by_hand():
    """The palette is the distinct pixel words in ascending unsigned order: alpha is the top byte, so the entries with
    A < 255 come first and trns_len counts them; 0xFF000000 behind the count."""
    px = [(1, 2, 3, 255), (9, 9, 9, 0), (1, 2, 3, 255), (0, 0, 0, 255), (200, 0, 0, 254), (0, 0, 1, 255), (9, 9, 9, 0), (255, 255, 255, 255)]
    rgba = bytes(v for p in px for v in p)
    st, pal, count, trns_len, summary = pm.analyse(rgba, 4, 256)
    assert (st, count, trns_len) == (0, 6, 2)
    assert pal[:7] == [0x00090909, 0xFE0000C8, 0xFF000000, 0xFF010000, 0xFF030201, 0xFFFFFFFF, 0xFF000000] and pal[7:] == [0xFF000000] * 249
    assert summary == 8 << 8
    assert pm.analyse(rgba, 4, 6)[0] == 0 and pm.analyse(rgba, 4, 5) == (12, None, None, None, 8 << 8)
    assert pm.analyse(rgba, 3, 256) == (2, None, None, None, None) and pm.analyse(rgba, 8, 256)[0] == 0
    # the summary: opaque, grey and each depth
    assert pm.analyse(bytes([0, 0, 0, 255, 255, 255, 255, 255]), 2, 256)[4] == pm.OPAQUE | pm.GREY | 1 << 8
    assert pm.analyse(bytes([0, 0, 0, 255, 85, 85, 85, 255]), 2, 256)[4] == pm.OPAQUE | pm.GREY | 2 << 8
    assert pm.analyse(bytes([0, 0, 0, 255, 85, 85, 17, 255]), 2, 256)[4] == pm.OPAQUE | 4 << 8
    assert pm.analyse(bytes([0, 0, 0, 255, 85, 85, 16, 255]), 2, 256)[4] == pm.OPAQUE | 8 << 8
    assert pm.analyse(bytes([0, 0, 0, 254, 255, 255, 255, 255]), 2, 256)[4] == pm.GREY | 1 << 8          # (alpha does not count for the depth)
    assert pm.analyse(b"", 5, 1) == (0, [0xFF000000] * 256, 0, 0, pm.OPAQUE | pm.GREY | 1 << 8)


def test_every_reason_for_not_representable():
    """A literal case per reason, and the same pixels in a pair that holds them."""
    opaque, clear = bytes([7, 7, 7, 255]), bytes([7, 7, 7, 254])
    assert pm.pack(opaque + clear, 2, 8, 2)[1] == 13 and pm.pack(opaque + opaque, 2, 8, 2) == (bytes([7] * 6), 0)      # a translucent pixel
    assert pm.pack(clear, 1, 8, 0)[1] == 13 and pm.pack(clear, 1, 8, 4) == (bytes([7, 254]), 0)
    rg = bytes([7, 8, 7, 255])
    assert pm.pack(rg, 1, 8, 0)[1] == 13 and pm.pack(rg, 1, 8, 4)[1] == 13 and pm.pack(rg, 1, 8, 2) == (bytes([7, 8, 7]), 0)   # R != G
    gb = bytes([7, 7, 8, 255])
    assert pm.pack(gb, 1, 16, 0)[1] == 13 and pm.pack(gb, 1, 16, 4)[1] == 13
    x80 = bytes([0x80, 0x80, 0x80, 255])
    assert pm.pack(x80, 1, 4, 0)[1] == 13 and pm.pack(x80, 1, 8, 0) == (b"\x80", 0)                                     # 0x80 at depth 4
    assert pm.pack(bytes([0x88] * 3 + [255]), 1, 4, 0) == (b"\x80", 0) and pm.pack(bytes([0x88] * 3 + [255]), 1, 2, 0)[1] == 13
    assert pm.pack(bytes([0xAA] * 3 + [255, 0x55] * 1 + [0x55, 0x55, 255]), 2, 2, 0) == (bytes([0b10010000]), 0)
    pal = [0xFF000001, 0xFF000002, 0xFF000003, 0xFF000004, 0xFF000005]
    five = bytes([5, 0, 0, 255])
    assert pm.pack(bytes([6, 0, 0, 255]), 1, 8, 3, pal, 5)[1] == 13                                                     # a colour missing from the palette
    assert pm.pack(five, 1, 8, 3, pal, 4)[1] == 13 and pm.pack(five, 1, 8, 3, pal, 5) == (b"\x04", 0)                   # (behind the count)
    assert pm.pack(five, 1, 2, 3, pal, 5)[1] == 13 and pm.pack(five, 1, 4, 3, pal, 5) == (b"\x40", 0)                   # an index of 4 at depth 2
    # the lowest index of equal words
    assert pm.pack(five, 1, 8, 3, [0xFF000005, 0xFF000009, 0xFF000005], 3) == (b"\x00", 0)
    # 16 bits: the byte twice
    assert pm.pack(bytes([1, 2, 3, 4]), 1, 16, 6) == (bytes([1, 1, 2, 2, 3, 3, 4, 4]), 0)
    # most significant bits first, padding zero: 1-bit grey 1 0 1 1 0, then 1 1 1 at width 3
    bw = lambda bits: b"".join(bytes([255 * b] * 3 + [255]) for b in bits)
    assert pm.pack(bw([1, 0, 1, 1, 0]), 5, 1, 0) == (bytes([0b10110000]), 0)
    assert pm.pack(bw([1, 1, 1, 0, 0, 1]), 3, 1, 0) == (bytes([0b11100000, 0b00100000]), 0)


def test_palette_file_by_hand():
    """The prefix arithmetic, the layout of a small file chunk by chunk, and the statuses' order."""
    assert pm.palette_file_prefix(1, 0) == 56 and pm.palette_file_prefix(2, 2) == 73 and pm.palette_file_prefix(256, 256) == 1089
    pal = [0x80030201, 0xFF060504] + [0xFF000000] * 254
    f = pm.write_palette_file(b"STREAM", 5, 7, 2, pal, 2, 4, 3)
    assert len(f) == pm.palette_file_prefix(4, 3) + 6 + 16
    chunks = []
    pos = 8
    while pos < len(f):
        n = fm.rd32(f, pos)
        chunks.append((f[pos + 4:pos + 8], f[pos + 8:pos + 8 + n]))
        assert fm.rd32(f, pos + 8 + n) == zlib.crc32(f[pos + 4:pos + 8 + n])
        pos += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"]
    assert chunks[1][1] == bytes([1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 0, 0]) and chunks[2][1] == bytes([0x80, 255, 255]) and chunks[3][1] == b"STREAM"
    assert [c[0] for c in _chunks(pm.write_palette_file(b"S", 5, 7, 2, pal, 2, 4, 0))] == [b"IHDR", b"PLTE", b"IDAT", b"IEND"]
    ok = dict(idat_len=6, height=7, slot=1000, count=2, trns_len=1, entries=4, alphas=3)
    assert pm.frame_palette_status(**ok) == 0
    assert pm.frame_palette_status(**dict(ok, slot=pm.palette_file_prefix(4, 3) + 6 + 15, count=0, trns_len=4)) == 2
    assert pm.frame_palette_status(**dict(ok, idat_len=0)) == 2 and pm.frame_palette_status(**dict(ok, height=0)) == 2
    assert pm.frame_palette_status(**dict(ok, count=0, trns_len=4)) == 10 and pm.frame_palette_status(**dict(ok, count=5)) == 10
    assert pm.frame_palette_status(**dict(ok, trns_len=4)) == 11 and pm.frame_palette_status(**dict(ok, trns_len=3)) == 0


def _chunks(f):
    out, pos = [], 8
    while pos < len(f):
        n = fm.rd32(f, pos)
        out.append((f[pos + 4:pos + 8], f[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


# ---- the library ----

def test_header_declares_and_library_exports_the_pack_calls():
    from fdeflate_amd import _lib
    import fdeflate_amd as fd
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    assert "#define FDH_PNG_STATUS_TOO_MANY_COLOURS 12u" in text and "#define FDH_PNG_STATUS_NOT_REPRESENTABLE 13u" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fdh_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "not declared: " + s
        assert hasattr(L, s), "not exported: " + s
        assert s in _lib.EXPORTED_SYMBOLS
    assert (fd.PNG_TOO_MANY_COLOURS, fd.PNG_NOT_REPRESENTABLE) == (12, 13)
    assert callable(fd.png_encode_rgba_files_batch)
    for e, t in ((1, 0), (2, 2), (16, 5), (256, 0), (256, 256)):
        assert fd.png_palette_file_prefix(e, t) == pm.palette_file_prefix(e, t) == 41 + 12 + 3 * e + (12 + t if t else 0)
    for e, t in ((0, 0), (257, 0), (4, 5)):
        assert L.fdh_png_palette_file_prefix(e, t) == 0


def test_pack_calls_refuse_bad_arguments_before_they_need_a_device():
    """An illegal pair, width, max_colours or PLTE / tRNS size: FDH_ERR_INVALID_ARGUMENT with a message, with or without
    a GPU; legal arguments get as far as the null pointers."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for width, depth, colour, word in ((0, 8, 2, b"width"), (1 << 31, 8, 2, b"width"), (5, 3, 0, b"fifteen"), (5, 16, 3, b"fifteen")):
        assert L.fdh_png_pack_batch(None, None, None, None, None, None, None, None, 1, width, depth, colour, None) == 1
        assert word in L.fdh_last_error()
    for depth, colour in fm.PAIRS:
        assert L.fdh_png_pack_batch(None, None, None, None, None, None, None, None, 1, 5, depth, colour, None) == 1
        assert b"null pointer" in L.fdh_last_error()
    for width, maxc, word in ((0, 256, b"width"), (1 << 31, 1, b"width"), (5, 0, b"max_colours"), (5, 257, b"max_colours")):
        assert L.fdh_png_analyse_batch(None, None, None, None, None, None, None, 1, width, maxc, None) == 1
        assert word in L.fdh_last_error()
    assert L.fdh_png_analyse_batch(None, None, None, None, None, None, None, 1, 5, 256, None) == 1 and b"null pointer" in L.fdh_last_error()
    for width, depth, e, t, word in ((0, 8, 4, 0, b"width"), (5, 16, 4, 0, b"fifteen"), (5, 3, 4, 0, b"fifteen"), (5, 8, 0, 0, b"plte_entries"),
                                     (5, 8, 257, 0, b"plte_entries"), (5, 2, 5, 0, b"plte_entries"), (5, 1, 3, 0, b"plte_entries"),
                                     (5, 4, 16, 17, b"trns_entries"), (5, 8, 1, 2, b"trns_entries")):
        assert L.fdh_png_frame_palette_batch(None, None, None, None, None, None, None, None, None, 1, width, depth, e, t, None) == 1
        assert word in L.fdh_last_error(), (width, depth, e, t)
    assert L.fdh_png_frame_palette_batch(None, None, None, None, None, None, None, None, None, 1, 5, 2, 4, 4, None) == 1
    assert b"null pointer" in L.fdh_last_error()
