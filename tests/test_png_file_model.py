"""tests/png_file_model.py -- the referee of the PNG-file kernels -- against implementations that share
nothing with it: zlib's crc32 and Pillow's PNG reader and writer.  Also the files the GPU tests share
(pillow_corpus, damaged_files) and the CPU-side check that the library declares and exports the new
entry points.
"""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_file_model as fm

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

def pillow_view(png):
    """What Pillow makes of a PNG file, as (mode, size, bytes)."""
    im = Image.open(io.BytesIO(png))
    im.load()
    return im.mode, im.size, im.tobytes()


def pillow_expected(pix, width, bit_depth, colour_type):
    """What Pillow shows of packed scanlines `pix` (uint8 [rows, row_bytes]) -> (mode, bytes): samples below 8 bits
    unpacked (grey ones scaled to 0 .. 255, palette indices as they are), 8-bit samples as they are, 16-bit grey
    little-endian, of any other 16-bit sample the high byte (grey + alpha shown as RGBA)."""
    h = pix.shape[0]
    if bit_depth < 8:
        bits = np.unpackbits(pix, axis=1)[:, :width * bit_depth].reshape(h, width, bit_depth)
        v = np.zeros((h, width), dtype=np.uint8)
        for k in range(bit_depth):
            v = (v << 1) | bits[:, :, k]
        if colour_type == 3:
            return "P", v.tobytes()
        if bit_depth == 1:
            return "1", np.packbits(v, axis=1).tobytes()
        return "L", (v * (255 // ((1 << bit_depth) - 1))).astype(np.uint8).tobytes()
    if bit_depth == 8:
        return {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}[colour_type], pix.tobytes()
    if colour_type == 0:
        return "I;16", pix.reshape(h, width, 2)[:, :, ::-1].tobytes()
    high = pix.reshape(h, width, -1)[:, :, ::2]
    if colour_type == 4:
        return "RGBA", high[:, :, [0, 0, 0, 1]].tobytes()
    return {2: "RGB", 6: "RGBA"}[colour_type], high.tobytes()


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


# ---- files written by Pillow: the corpus the GPU tests share ----

# (name, Pillow mode, colour type, bit depth, width, height): about 200 KiB of mostly random samples each, so that a
# level-6 stream fills three or more of Pillow's 64 KiB IDAT chunks
CORPUS = (
    ("bilevel", "1", 0, 1, 1301, 1264),
    ("grey", "L", 0, 8, 501, 420),
    ("palette", "P", 3, 8, 499, 421),
    ("grey-alpha", "LA", 4, 8, 331, 320),
    ("rgb", "RGB", 2, 8, 301, 240),
    ("rgba", "RGBA", 6, 8, 251, 220),
    ("grey16", "I;16", 0, 16, 333, 320),
)


def _corpus_image(r, mode, width, height):
    ch = {"1": 1, "L": 1, "P": 1, "LA": 2, "RGB": 3, "RGBA": 4, "I;16": 1}[mode]
    x = np.arange(width, dtype=np.int64)[None, :, None]
    y = np.arange(height, dtype=np.int64)[:, None, None]
    k = np.arange(ch, dtype=np.int64)[None, None, :]
    a = r.integers(0, 256, (height, width, ch))
    a[height // 3:height // 2] = ((x * (k + 1) + 3 * y) & 0xFF)[height // 3:height // 2]     # a smooth band: other filter types
    if mode == "1":
        return Image.fromarray((a[:, :, 0] & 1).astype(bool))
    if mode == "I;16":
        return Image.fromarray((a[:, :, 0] * 257 ^ r.integers(0, 256, (height, width))).astype(np.uint16))
    if mode == "P":
        im = Image.fromarray(a[:, :, 0].astype(np.uint8), "P")
        im.putpalette(r.integers(0, 256, 768, dtype=np.uint8).tobytes())
        return im
    a = a.astype(np.uint8)
    return Image.fromarray(a[:, :, 0] if ch == 1 else a, mode)


def packed_scanlines(im):
    """The PNG's own packed scanlines of an image Pillow holds: its bytes, 16-bit grey made big-endian."""
    raw = im.tobytes()
    if im.mode == "I;16":
        raw = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 2)[:, ::-1].tobytes()
    return raw


_corpus = []


def pillow_corpus():
    """[(name, file bytes, width, height, bit depth, colour type, packed scanlines)]: written by Pillow at its default
    level 6, with two tEXt chunks and a pHYs (and a PLTE in the palette file)."""
    from PIL import PngImagePlugin
    if not _corpus:
        r = np.random.default_rng(5300)
        for name, mode, colour, depth, width, height in CORPUS:
            im = _corpus_image(r, mode, width, height)
            meta = PngImagePlugin.PngInfo()
            meta.add_text("Title", "fdeflate test file " + name)
            meta.add_text("Comment", "x" * 300)
            buf = io.BytesIO()
            im.save(buf, format="PNG", pnginfo=meta, dpi=(144, 144))
            back = Image.open(io.BytesIO(buf.getvalue()))
            back.load()
            assert back.mode == mode and back.size == (width, height)
            _corpus.append((name, buf.getvalue(), width, height, depth, colour, packed_scanlines(back)))
    return _corpus


def chunks_of(png):
    """[(tag, body)] of a sound file; every CRC is checked with zlib on the way."""
    out, pos = [], 8
    while pos < len(png):
        n, tag = fm.rd32(png, pos), png[pos + 4:pos + 8]
        body = png[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) == fm.rd32(png, pos + 8 + n)
        out.append((tag, body))
        pos += 12 + n
    return out


def build(chunks):
    """A file of the given chunks, their CRCs by zlib."""
    out = fm.SIGNATURE
    for tag, body in chunks:
        out += fm.be32(len(body)) + tag + body + fm.be32(zlib.crc32(tag + body))
    return out


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


def _patched_ihdr(ch, at, value):
    body = bytearray(ch[0][1])
    body[at] = value
    return [(b"IHDR", bytes(body))] + ch[1:]


def damaged_files(png):
    """[(what, file, status, status with FDH_PNG_FLAG_IGNORE_CRC, True if Pillow must refuse it)] from one sound file
    with three or more IDAT chunks and ancillary chunks in front of them."""
    ch = chunks_of(png)
    tags = [t for t, _ in ch]
    i0 = tags.index(b"IDAT")
    assert tags.count(b"IDAT") >= 3 and tags[-1] == b"IEND" and i0 >= 2
    at_idat = 8 + sum(12 + len(b) for _, b in ch[:i0])
    text = (b"tEXt", b"Comment\0between")
    out = []

    def crc_field(k):
        """The file with bit 0 of the last byte of chunk k's CRC field flipped."""
        end = 8 + sum(12 + len(b) for _, b in ch[:k + 1])
        return png[:end - 1] + bytes([png[end - 1] ^ 1]) + png[end:]

    out.append(("signature", b"\x89PNG\r\n\x1a\r" + png[8:], 1, 1, True))
    out.append(("empty file", b"", 1, 1, True))
    out.append(("cut inside the second IDAT", png[:at_idat + 12 + len(ch[i0][1]) + 100], 2, 2, True))
    out.append(("IEND cut off", png[:-12], 2, 2, False))
    out.append(("cut inside IHDR", png[:20], 2, 2, True))
    out.append(("depth 3", build(_patched_ihdr(ch, 8, 3)), 3, 3, False))
    out.append(("width 0", build([(b"IHDR", b"\0\0\0\0" + ch[0][1][4:])] + ch[1:]), 3, 3, False))
    out.append(("filter method 1", build(_patched_ihdr(ch, 11, 1)), 3, 3, False))
    out.append(("IHDR not first", build([ch[1], ch[0]] + ch[2:]), 3, 3, False))
    out.append(("IHDR of 14 bytes", build([(b"IHDR", ch[0][1] + b"\0")] + ch[1:]), 3, 3, False))
    out.append(("Adam7", build(_patched_ihdr(ch, 12, 1)), 4, 4, False))
    out.append(("no IDAT", build([c for c in ch if c[0] != b"IDAT"]), 5, 5, False))
    out.append(("IDAT chunks apart", build(ch[:i0 + 1] + [text] + ch[i0 + 1:]), 5, 5, False))
    out.append(("PLTE behind IDAT", build(ch[:-1] + [(b"PLTE", bytes(range(30)))] + ch[-1:]), 5, 5, False))
    out.append(("unknown critical chunk", build(ch[:1] + [(b"ABCD", b"1234")] + ch[1:]), 5, 5, False))
    out.append(("CRC field of IHDR", crc_field(0), 6, 0, True))
    out.append(("CRC field of a tEXt", crc_field(tags.index(b"tEXt")), 6, 0, False))
    out.append(("CRC field of the second IDAT", crc_field(i0 + 1), 6, 0, False))
    out.append(("CRC field of IEND", crc_field(len(ch) - 1), 6, 0, False))
    body_at = at_idat + 12 + len(ch[i0][1]) + 8 + 5000       # a byte inside the second IDAT's body
    out.append(("a data byte of the second IDAT", png[:body_at] + bytes([png[body_at] ^ 0x10]) + png[body_at + 1:], 6, 0, False))
    # structure comes before CRC: both faults in one file
    apart = build(ch[:i0 + 1] + [text] + ch[i0 + 1:])
    out.append(("IHDR CRC and IDAT chunks apart", apart[:32] + bytes([apart[32] ^ 1]) + apart[33:], 5, 5, True))
    return out


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
