"""The expected files of PNG encode at a compression level, on the CPU alone: what tests/test_gpu_png_levels.py compares
the device's files with is png_encode_mixed_model.encode / png16_encode_model.encode16 around the streams of
level_model (levels 1-3), lazy_model (4-9) and the oracle's stored writer (0), with png_choose_model's filter types.
Here every such file is opened by Pillow, its IDAT is inflated by zlib to png_model.filter_rows of the chosen types, and
the size condition of the tiled picture is shown to hold for the models' bytes alone."""
import zlib

import numpy as np
import pytest

import png16_encode_cases as c16
import png16_encode_model as e16
import png_choose_model as cm
import png_corpus as pc
import png_file_model as fm
import png_levels_cases as lc
import png_model
import png_pack_model as pm


def test_the_cases_are_small_and_of_the_kinds_the_issue_names():
    names = [c[0] for c in lc.cases8()]
    assert len(set(names)) == len(names) and lc.TILED in names
    pairs = {}
    for (name, px, w, h, pair, want), (st, f, depth, colour) in zip(lc.cases8(), lc.expected8(1)):
        assert px.dtype == np.uint8 and px.size == w * h * 4
        assert st == want, name
        if st == 0:
            rb = fm.geometry(w, depth, colour)[0]
            assert h * (rb + 1) <= 6200, name
            pairs[name] = (depth, colour)
    assert pairs[lc.TILED] == (8, 2) and pairs["tiled-grey"] == (8, 0) and pairs["tiled-palette"][1] == 3
    assert pairs["one-bit"] == (1, 0) and pairs["tiled-rgb-as-rgba"] == (8, 6) and pairs["noise"] == (8, 6)
    assert [c[5] for c in lc.cases8()].count(12) == 1 and [c[5] for c in lc.cases8()].count(13) == 1
    wide = {c[0]: e for c, e in zip(lc.cases16(), lc.expected16(1))}
    assert wide["tiled-rgb16"][2:] == (16, 2) and wide["tiled-rgb16"][0] == 0


@pytest.mark.parametrize("level", lc.LEVELS)
def test_expected_rgba8_files_open_in_pillow_and_inflate_to_the_filtered_rows(level):
    for (name, px, w, h, pair, want), (st, f, depth, colour) in zip(lc.cases8(), lc.expected8(level)):
        assert st == want, (name, level)
        if st != 0:
            assert f is None
            continue
        scan = fm.scan(f, crc=zlib.crc32)
        assert (scan.status, scan.width, scan.height, scan.bit_depth, scan.colour_type) == (0, w, h, depth, colour), name
        assert pc.pillow_rgba(f) == px.tobytes(), (name, level)
        # the IDAT is the filtered rows of the packed scanlines under the chosen types
        a_status, pal, count, _, _ = pm.analyse(px.tobytes(), w, 256)
        pix, p_st = pm.pack(px.tobytes(), w, depth, colour, pal, count or 256)
        assert p_st == 0
        rb, bpp = fm.geometry(w, depth, colour)
        rows = np.frombuffer(pix, dtype=np.uint8).reshape(h, rb)
        types = cm.choose(rows, bpp)[0]
        assert zlib.decompress(lc.idat_of(f)) == png_model.filter_rows(rows, bpp, list(types)).tobytes(), (name, level)


@pytest.mark.parametrize("level", lc.LEVELS)
def test_expected_rgba16_files(level):
    """The narrow pictures get the RGBA8 files; the wide one is read back without device code and, as far as Pillow
    reads 16-bit files, there."""
    narrow = {c[0]: e for c, e in zip(lc.cases8(), lc.expected8(level))}
    for (name, px, w, h, pair, want), (st, f, depth, colour) in zip(lc.cases16(), lc.expected16(level)):
        assert st == want, (name, level)
        if name in narrow:
            assert (st, f, depth, colour) == narrow[name], (name, level)
        elif st == 0:
            back, d, c = c16.host_route(f)
            assert (d, c) == (depth, colour) == (16, 2) and bytes(back) == px.tobytes()
            c16.check_in_pillow(f, px, w, h, depth, colour)
            assert e16.analyse16(px.tobytes(), w)[0] == 12          # not narrow: no palette, and no error


def test_size_condition_on_the_models_bytes():
    """The tiled RGB picture: the stream at each of levels 1, 3, 6 and 9 is under one tenth of the ultra-fast stream of the
    same filtered rows, and so is the file (57 bytes of framing on either side); the stored stream is the filtered rows
    and eleven bytes."""
    k = [c[0] for c in lc.cases8()].index(lc.TILED)
    filtered = zlib.decompress(lc.idat_of(lc.expected8(0)[k][1]))
    assert len(filtered) == 40 * 145
    fast = lc.ultrafast_stream_size(filtered)
    assert fast > len(filtered)                                     # larger than its input: the rows are not mostly zero
    assert len(lc.idat_of(lc.expected8(0)[k][1])) == len(filtered) + 11
    for level in lc.SIZE_LEVELS:
        f = lc.expected8(level)[k][1]
        stream = len(lc.idat_of(f))
        print("level %d: stream %d bytes, file %d; ultra-fast stream %d, file %d" % (level, stream, len(f), fast, fast + 57))
        assert 10 * stream < fast and 10 * len(f) < fast + 57, level
