"""The plan of a mixed batch (tests/png_mixed_model.py) against the models it is built on and against files, and
fdh_png_plan_sizes -- host arithmetic, loads without a GPU -- against the plan; the exports of the section "PNG decode:
mixed batches"."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest

import png_adam7_model as am
import png_expand_model as em
import png_file_model as fm
import png_mixed_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdh_png_plan_sizes", "fdh_png_plan_batch", "fdh_png_gather_idat_mixed_batch", "fdh_png_colour_mixed_batch",
               "fdh_png_unfilter_mixed_batch", "fdh_png_expand_mixed_batch")


def test_plan_agrees_with_the_adam7_and_file_models():
    for r in mm.small_records():
        w, h, d, c = r["width"], r["height"], r["bit_depth"], r["colour_type"]
        rb = fm.geometry(w, d, c)[0]
        st, comp, filt, pix, rgba = mm.plan(r)
        assert st == 0 and comp == r["idat_bytes"] and pix == h * rb and rgba == h * w * 4
        assert filt == (am.size(w, h, d, c) if r["interlace"] else h * (rb + 1)), r
        assert filt > pix


def _model_files():
    r = np.random.default_rng(5)
    for d, c in fm.PAIRS:
        for method in (0, 1):
            w, h = int(r.integers(1, 40)), int(r.integers(1, 20))
            rb = fm.geometry(w, d, c)[0]
            pix = r.integers(0, 256, h * rb, dtype=np.uint8).tobytes()
            if method:
                idat = am.stream_of(pix, w, h, d, c, r.integers(0, 5, am.pass_rows(w, h)).tolist())
            else:
                rows = np.frombuffer(pix, dtype=np.uint8).reshape(h, rb)
                idat = zlib.compress(np.concatenate([np.zeros((h, 1), dtype=np.uint8), rows], axis=1).tobytes())
            yield am.write_file(idat, w, h, d, c, idat_chunks=1 + (w % 3), method=method)


def _pillow_files():
    Image = pytest.importorskip("PIL.Image")
    r = np.random.default_rng(6)
    for mode, ch in (("1", 1), ("L", 1), ("P", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4), ("I;16", 2)):
        w, h = int(r.integers(1, 70)), int(r.integers(1, 30))
        if mode == "I;16":
            im = Image.fromarray(r.integers(0, 65536, (h, w), dtype=np.uint16))
        elif mode == "1":
            im = Image.fromarray(r.integers(0, 2, (h, w), dtype=np.uint8) * 255).convert("1")
        else:
            a = r.integers(0, 256, (h, w, ch) if ch > 1 else (h, w), dtype=np.uint8)
            im = Image.fromarray(a, "L" if mode == "P" else mode)
            if mode == "P":
                im.putpalette(r.integers(0, 256, 768, dtype=np.uint8).tobytes())
        b = io.BytesIO()
        im.save(b, "PNG")
        yield b.getvalue()


@pytest.mark.parametrize("files", [_model_files, _pillow_files], ids=["models", "pillow"])
def test_plan_agrees_with_what_files_decode_to(files):
    count = 0
    for f in files():
        info = am.scan(f, adam7=True, crc=zlib.crc32)
        assert info.status == 0
        st, comp, filt, pix, rgba = mm.plan(mm.of_info(info))
        assert st == 0 and comp == len(info.idat) and filt == len(zlib.decompress(info.idat))
        w, h, d, c, packed = am.decode(f)
        assert pix == len(packed) and rgba == 4 * w * h
        count += 1
    assert count >= 7


def test_undecodable_and_boundary_records():
    for r in mm.undecodable_records():
        assert mm.plan(r) == (3, 0, 0, 0, 0) and mm.plan(r, 1) == (3, 0, 0, 0, 0), r
    b = mm.boundary_records()
    assert mm.plan(*b[0]) == (0, 100, (1 << 32) - 1, 65535 * 65536, 65535 * 65536 * 4)
    assert mm.plan(*b[1]) == (2, 0, 0, 0, 0)
    assert mm.filtered_size(65535, 65536, 8, 0, 0) == 1 << 32
    for r, m in b[-60:]:
        assert r["width"] == r["height"] == 0x7FFFFFFF and mm.plan(r, m)[0] == 2


def _plan_sizes(L, r, max_bytes):
    words = (ctypes.c_uint32 * 8)(*mm.words(r))
    sizes = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    st = L.fdh_png_plan_sizes(words, max_bytes, sizes)
    return (st,) + tuple(sizes)


def test_plan_sizes_of_the_library_is_the_model():
    from fdeflate_amd import _lib
    L = _lib.lib()
    cases = mm.all_cases()
    assert len(cases) > 3700
    for r, m in cases:
        assert _plan_sizes(L, r, m) == mm.plan(r, m), (r, m)
    # a wrapped product would come back as a small size: 2^31-1 squared times 4 is 2^64 - 2^34 + 4
    for d, c in fm.PAIRS:
        assert _plan_sizes(L, mm.record(0x7FFFFFFF, 0x7FFFFFFF, d, c), 0) == (2, 0, 0, 0, 0)


def test_python_wrapper_of_plan_sizes():
    import fdeflate_amd as fd
    for r, m in mm.boundary_records() + [(r, 0) for r in mm.undecodable_records()]:
        assert fd.png_plan_sizes(r, m) == mm.plan(r, m)
    assert fd.png_plan_sizes({"width": 3, "height": 2, "bit_depth": 8, "colour_type": 6}) == (0, 0, 26, 24, 24)


def test_the_new_section_is_declared_exported_and_listed():
    from fdeflate_amd import _lib
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    assert "PNG decode: mixed batches" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s + " is not declared"
        assert hasattr(L, s), s + " is not exported"
        assert s in _lib.EXPORTED_SYMBOLS
    import fdeflate_amd as fd
    for name in ("png_plan_sizes", "png_plan_batch", "png_gather_idat_mixed_batch", "png_colour_mixed_batch", "png_unfilter_mixed_batch",
                 "png_expand_mixed_batch", "png_decode_mixed_files_batch", "png_decode_mixed_files_rgba_batch"):
        assert callable(getattr(fd, name))


def test_key_tells_geometries_apart():
    keys = {mm.key(r) for r in mm.small_records()}
    assert len(keys) == 15 * 2 * len(mm.SIDES)      # (the height is not part of a geometry)
    r = mm.record(341, 64, 8, 2)
    assert mm.key(r) == 341 | 8 << 32 | 2 << 40 and mm.key(mm.record(341, 9, 8, 2, 1)) == mm.key(r) | 1 << 48
    w = mm.words(r)
    assert (w[1] | (w[3] & 0xFFFFFF) << 32) == mm.key(r)     # how the pipeline builds it from the record's words
