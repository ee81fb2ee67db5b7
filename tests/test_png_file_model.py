"""tests/png_file_model.py -- the referee of the PNG-file kernels -- against implementations that share
nothing with it: zlib's crc32 and Pillow's PNG reader and writer.  Also the CPU-side check that the
library declares and exports the new entry points.  The files come from tests/png_corpus.py (pillow_corpus,
damaged_files), which the GPU tests share.
"""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_file_model as fm
from png_corpus import chunks_of, damaged_files, pillow_corpus, pillow_expected, pillow_view

Image = pytest.importorskip("PIL.Image")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fdh_crc32_batch", "fdh_png_frame_batch", "fdh_png_file_bound", "fdh_png_scan_files_batch", "fdh_png_gather_idat_batch")


# ---- CRC-32 and the combine ----

def test_crc_equals_zlib():
    """Every length 0 .. 300, three lengths up to 1 MiB, seeds 0 and random."""
    r = np.random.default_rng(5100)
    data = r.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    assert fm.crc32(b"123456789") == 0xCBF43926      # the check value of the CRC catalogue
    for n in range(301):
        at = int(r.integers(0, 1000))
        seed = int(r.integers(0, 1 << 32)) if n % 3 else 0
        assert fm.crc32(data[at:at + n], seed) == zlib.crc32(data[at:at + n], seed), (n, seed)
    for n in (65537, 100003, 1 << 20):
        seed = int(r.integers(0, 1 << 32))
        assert fm.crc32(data[:n], seed) == zlib.crc32(data[:n], seed), n


def test_combine_at_every_split():
    """crc(A || B) = crc(A) * x^(8 |B|) mod P xor crc(B) at every split of 300 bytes, the empty halves included; a seed
    is a CRC in front: crc(B, seed) = combine(seed, crc(B), |B|)."""
    r = np.random.default_rng(5101)
    buf = r.integers(0, 256, 300, dtype=np.uint8).tobytes()
    whole = zlib.crc32(buf)
    for k in range(301):
        a, b = buf[:k], buf[k:]
        assert fm.combine(zlib.crc32(a), zlib.crc32(b), len(b)) == whole, k
        assert fm.combine(fm.crc32(a), fm.crc32(b), len(b)) == whole, k
        seed = int(r.integers(0, 1 << 32))
        assert fm.combine(seed, zlib.crc32(b), len(b)) == zlib.crc32(b, seed), k
    # the order of x: exponents are taken modulo 2^32 - 1 (a 4 GiB range needs x^(2^35))
    assert fm.xpow(0xFFFFFFFF) == 0x80000000 and fm.xpow(0xFFFFFFFF + 77) == fm.xpow(77)
    assert fm.xpow(1) == 0x40000000 and fm.mulmod(fm.xpow(31), fm.xpow(1)) == fm.xpow(32) == fm.POLY


# ---- the writer ----


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_written_files_load_in_pillow(pair):
    """The 41 / 16 framing around zlib.compress(filtered, 1), filtered by the oracle with every type in turn, at a
    width of one pixel, an odd one and one of more than 4 KiB of row: Pillow loads the file and shows the pixels."""
    depth, colour = pair
    r = np.random.default_rng(5200 + 16 * colour + depth)
    for width in (1, 37, 4099):
        rb, bpp = fm.geometry(width, depth, colour)
        assert bpp in (1, 2, 3, 4, 6, 8) and rb == (width * fm.CHANNELS[colour] * depth + 7) // 8
        rows = 11
        pix = r.integers(0, 256, (rows, rb), dtype=np.uint8)
        types = bytes(k % 5 for k in range(rows))
        st, filt = ob.png_filter(pix.tobytes(), rb, bpp, types)
        assert st == 0
        f = fm.write_file(zlib.compress(filt, 1), width, rows, depth, colour)
        assert f[-12:] == bytes.fromhex("0000000049454E44AE426082") and f[:8] == b"\x89PNG\r\n\x1a\n"
        mode, size, shown = pillow_view(f)
        want_mode, want = pillow_expected(pix, width, depth, colour)
        assert (mode, size) == (want_mode, (width, rows)), (pair, width, mode)
        assert shown == want, (pair, width)
        info = fm.scan(f)
        assert info.fields() == (0, width, rows, depth, colour, 0, len(f) - 57, 1, 33, 3), (pair, width, info)


# ---- files written by Pillow (png_corpus.pillow_corpus) ----

def test_reader_on_pillow_files():
    """Status 0, Pillow's geometry, every chunk counted, and the concatenated IDAT bodies inflate (zlib) to the
    filtered image that the oracle reconstructs to the pixels Pillow shows."""
    tags = set()
    for name, png, width, height, depth, colour, pixels in pillow_corpus():
        info = fm.scan(png)
        ch = chunks_of(png)
        tags |= {t for t, _ in ch}
        n_idat = sum(1 for t, _ in ch if t == b"IDAT")
        assert n_idat >= 3, (name, n_idat)
        first = 8 + sum(12 + len(b) for t, b in ch[:[t for t, _ in ch].index(b"IDAT")])
        idat = b"".join(b for t, b in ch if t == b"IDAT")
        assert info.fields() == (0, width, height, depth, colour, 0, len(idat), n_idat, first, len(ch)), (name, info)
        assert info.idat == idat
        rb, bpp = fm.geometry(width, depth, colour)
        filt = zlib.decompress(info.idat)
        assert len(filt) == height * (rb + 1), name
        assert ob.png_unfilter(filt, rb, bpp) == (0, pixels), name
    assert {b"IHDR", b"PLTE", b"tEXt", b"pHYs", b"IDAT", b"IEND"} <= tags, tags


def test_reader_on_damaged_files():
    """Every status code 1 .. 6, several ways each, from one Pillow file.  Pillow is the referee only where it does
    refuse a file (a damaged signature, a damaged IHDR CRC field, a file cut inside IDAT or IHDR): there it must raise.
    It does not check the CRC field of an IDAT, a tEXt or IEND and does not need IEND, so for status 6 on those and for
    the missing IEND the referees are zlib.crc32 (the damaged chunk's stored CRC differs from zlib's of its bytes,
    every other chunk's agrees) and the specification (5.3: every chunk has a CRC; 5.6: IEND must be there).  With CRC
    checking off, a file whose only fault is a CRC field reads like the sound one."""
    name, png = pillow_corpus()[1][:2]
    sound = fm.scan(png)
    assert sound.status == 0
    seen = set()
    for what, f, status, status_ignoring, pillow_refuses in damaged_files(png):
        got = fm.scan(f)
        assert got.status == status, (what, got)
        assert fm.scan(f, ignore_crc=True).status == status_ignoring, what
        seen.add(status)
        if pillow_refuses:
            with pytest.raises(Exception):
                pillow_view(f)
        if status == 6:
            # zlib as referee: walk the (structurally sound) file, exactly one chunk's CRC differs
            pos, differing = 8, 0
            while pos < len(f):
                n = fm.rd32(f, pos)
                differing += zlib.crc32(f[pos + 4:pos + 8 + n]) != fm.rd32(f, pos + 8 + n)
                pos += 12 + n
            assert differing == 1, what
            if "CRC field" in what:
                ignoring = fm.scan(f, ignore_crc=True)
                assert ignoring.fields() == sound.fields() and ignoring.idat == sound.idat, what
    assert seen == {1, 2, 3, 4, 5, 6}
    # bytes behind IEND are ignored
    assert fm.scan(png + b"trailing bytes").fields() == sound.fields()


# ---- the library ----

def test_header_declares_and_library_exports_the_png_file_calls():
    from fdeflate_amd import _lib
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(fdh_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "not declared: " + s
        assert hasattr(L, s), "not exported: " + s
        assert s in _lib.EXPORTED_SYMBOLS
    assert "FDH_PNG_FILE_PREFIX 41u" in text and "FDH_PNG_FILE_SUFFIX 16u" in text
    assert L.fdh_png_file_bound(64, 1023) == L.fdh_ultrafast_bound(64 * 1024) + 57
    assert L.fdh_png_file_bound(0, 5) == L.fdh_ultrafast_bound(0) + 57 == 117
    assert ctypes.sizeof(ctypes.c_uint32) * 8 == 32      # fdh_png_info: eight 32-bit words


def test_frame_refuses_bad_geometry_before_it_needs_a_device():
    """width 0 or above 2^31 - 1 and a depth / colour pair outside the fifteen: FDH_ERR_INVALID_ARGUMENT with a message,
    with or without a GPU (the check comes first)."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for width, depth, colour, word in ((0, 8, 2, b"width"), (1 << 31, 8, 2, b"width"), (5, 3, 0, b"fifteen"), (5, 16, 3, b"fifteen"),
                                      (5, 4, 2, b"fifteen"), (5, 8, 1, b"fifteen"), (5, 8, 5, b"fifteen"), (5, 0, 0, b"fifteen")):
        assert L.fdh_png_frame_batch(None, None, None, None, None, None, 1, width, depth, colour, None) == 1
        assert word in L.fdh_last_error(), (width, depth, colour, L.fdh_last_error())
        assert L.fdh_png_gather_idat_batch(None, None, None, None, None, None, None, 1, width, depth, colour, None) == 1
    for depth, colour in fm.PAIRS:      # a legal pair gets as far as the null pointers
        assert L.fdh_png_frame_batch(None, None, None, None, None, None, 1, 5, depth, colour, None) == 1
        assert b"null pointer" in L.fdh_last_error()
