"""The inputs that the PNG model tests and the PNG GPU tests share: random packed rows, model-written and Pillow-written
files, damaged files, RGBA pictures of every kind.  A plain module (no tests): each test_png_*_model.py pins the model it
names against references of its own, and the GPU tests draw on the same builders, so seeds, signatures and defaults
here are part of what those tests assert.

Every user needs Pillow for some of its cases; without it the importing test module is skipped as a whole.
"""
import io
import zlib

import numpy as np
import pytest

import png_adam7_model as am
import png_expand_model as em
import png_file_model as fm

Image = pytest.importorskip("PIL.Image")


# ---- packed rows, their chunks and files (pinned by test_png_expand_model.py) ----


KEYED = ((1, 3), (2, 3), (4, 3), (8, 3), (1, 0), (8, 0), (8, 2))      # (depth, colour) with tRNS that Pillow follows


CLASSES = [(d, c, False) for d, c in fm.PAIRS] + [(d, c, True) for d, c in KEYED]


LEFT_OUT = ((2, 0), (4, 0), (16, 0), (16, 2))


def stream_of(pix, row_bytes):
    """The zlib stream of packed rows, every row with filter type 0."""
    pix = bytes(pix)
    rows = len(pix) // row_bytes
    return zlib.compress(b"".join(b"\0" + pix[r * row_bytes:(r + 1) * row_bytes] for r in range(rows)), 6)


def random_case(r, width, height, depth, colour, keyed, entries=None):
    """(pix uint8 [height * row_bytes], key or None, pal or None) of random rows.  A key is the first pixel's samples
    (so it is hit at least once), and at depth 16 some pixels differ from it in their low bytes only.  A palette has
    `entries` entries (2^depth by default) and with `keyed` a tRNS that is shorter than the PLTE when that has more than
    two entries."""
    rb = fm.geometry(width, depth, colour)[0]
    ch = fm.CHANNELS[colour]
    pix = r.integers(0, 256, (height, rb), dtype=np.uint8)
    key = pal = None
    if colour == 3:
        n = entries if entries is not None else 1 << depth
        alpha = r.integers(0, 256, n - 1 if n > 2 else n, dtype=np.uint8).tolist() if keyed else []
        pal = em.palette(r.integers(0, 256, 3 * n, dtype=np.uint8).tobytes(), bytes(alpha))
    elif keyed and colour in (0, 2):
        key = tuple(em.samples(pix[0].tobytes(), 1, depth, ch))
        if depth >= 8:       # more hits, and near misses in the low byte
            bpp = ch * depth // 8
            first = pix[0, :bpp].copy()
            for x in range(2, width, 3):
                pix[height // 2, x * bpp:(x + 1) * bpp] = first
                if depth == 16 and x % 2:
                    pix[height // 2, (x + 1) * bpp - 1] ^= 1
    return pix.reshape(-1), key, pal


def pre_chunks(colour, key, pal, text=False):
    pre = [(b"tEXt", b"Comment\0in front")] if text else []
    if pal is not None:
        pre.append((b"PLTE", em.plte_body(pal)))
        alpha = [e[3] for e in pal]
        while alpha and alpha[-1] == 255:
            alpha.pop()
        if alpha:
            pre.append((b"tRNS", bytes(alpha)))
    if key is not None:
        pre.append((b"tRNS", em.trns_body(key)))
    return pre


def pillow_rgba(png):
    """Pillow's RGBA8 bytes of a file; 16-bit grey (mode I;16) is the array >> 8 with alpha 255."""
    im = Image.open(io.BytesIO(png))
    im.load()
    if im.mode == "I;16":
        g = (np.asarray(im).astype(np.uint16) >> 8).astype(np.uint8)
        return np.stack([g, g, g, np.full_like(g, 255)], axis=-1).tobytes()
    return im.convert("RGBA").tobytes()


def status_files(width=5, height=3, crc=zlib.crc32):
    """[(what, file, (width, depth, colour) of the CALL, expected status)]: one file per way to get 10 and 11, the two
    tolerated cases, a file the scan refuses (3), another geometry (7) and sound files in between."""
    r = np.random.default_rng(7300)
    out = []

    def add(what, depth, colour, pre, want, call=None):
        rb = fm.geometry(width, depth, colour)[0]
        pix = r.integers(0, 256, height * rb, dtype=np.uint8)
        if colour == 3:
            pix &= 3                     # indices 0 .. 3
        out.append((what, em.write_file(stream_of(pix, rb), width, height, depth, colour, pre, 2, crc), call or (width, depth, colour), want, pix))

    plte4 = (b"PLTE", bytes(range(12)))
    text = (b"tEXt", b"Title\0x")
    add("sound palette", 8, 3, [text, plte4, (b"tRNS", bytes([9, 8, 7]))], 0)
    add("no PLTE", 8, 3, [text], 10)
    add("PLTE of no bytes", 8, 3, [(b"PLTE", b"")], 10)
    add("PLTE of 13 bytes", 8, 3, [(b"PLTE", bytes(13))], 10)
    add("PLTE of 771 bytes", 8, 3, [(b"PLTE", bytes(771))], 10)
    add("two PLTE", 8, 3, [plte4, plte4], 10)
    add("sound palette of 256", 8, 3, [(b"PLTE", bytes(768)), (b"tRNS", bytes(256))], 0)
    add("grey tRNS of 1 byte", 8, 0, [(b"tRNS", b"\0")], 11)
    add("grey tRNS of 4 bytes", 4, 0, [(b"tRNS", bytes(4))], 11)
    add("RGB tRNS of 2 bytes", 8, 2, [(b"tRNS", bytes(2))], 11)
    add("sound grey key", 8, 0, [(b"tRNS", b"\0\x07"), text], 0)
    add("palette tRNS longer than PLTE", 8, 3, [plte4, (b"tRNS", bytes(5))], 11)
    add("palette tRNS in front of PLTE", 8, 3, [(b"tRNS", bytes(2)), plte4], 11)
    add("palette tRNS and no PLTE", 8, 3, [(b"tRNS", bytes(2))], 11)
    add("two tRNS, grey", 8, 0, [(b"tRNS", bytes(2)), (b"tRNS", bytes(2))], 11)
    add("two tRNS, RGB", 16, 2, [(b"tRNS", bytes(6)), text, (b"tRNS", bytes(6))], 11)
    add("two tRNS, palette", 2, 3, [plte4, (b"tRNS", bytes(2)), (b"tRNS", bytes(2))], 11)
    add("sound RGB key", 16, 2, [(b"tRNS", bytes([0x12, 0x34, 0, 5, 0xFF, 0xFE]))], 0)
    add("tolerated: tRNS with grey + alpha", 8, 4, [(b"tRNS", bytes(2)), (b"tRNS", bytes(7))], 0)
    add("tolerated: tRNS with RGBA", 8, 6, [(b"tRNS", bytes(1))], 0)
    add("tolerated: PLTE with RGB", 8, 2, [(b"PLTE", bytes(5)), (b"PLTE", b"")], 0)
    add("tolerated: PLTE with grey, behind its key", 8, 0, [(b"tRNS", b"\0\x21"), plte4], 0)
    add("another geometry", 8, 0, [], 7, call=(width, 8, 3))
    add("another width", 8, 3, [plte4], 7, call=(width + 1, 8, 3))
    what, f, call, _, pix = out[0]
    out.append(("refused by the scan", f[:40], call, 3, pix))
    return out


# ---- Pillow's view, Pillow-written files, damaged files (pinned by test_png_file_model.py) ----


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


def corpus_image(r, mode, width, height):
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
            im = corpus_image(r, mode, width, height)
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


# ---- RGBA8 pictures for the packers (pinned by test_png_pack_model.py) ----


def representable(r, width, height, depth, colour):
    """Random RGBA8 rows (uint8 [height * width * 4]) that the pair holds without loss: random packed rows, expanded."""
    assert colour != 3
    pix, _, _ = random_case(r, width, height, depth, colour, False)
    rgba, st = em.expand(pix, width, depth, colour)
    assert st == 0
    return np.frombuffer(rgba, dtype=np.uint8).copy()


def palette_image(r, width, height, colours, translucent):
    """Random RGBA8 rows of exactly min(colours, width * height) distinct pixels, `translucent` of them (at most) with
    A < 255; every colour occurs."""
    colours = min(colours, width * height)
    words = set()
    while len(words) < colours:
        a = int(r.integers(0, 255)) if len(words) < translucent else 255
        words.add(int(r.integers(0, 1 << 24)) | a << 24)
    words = np.array(sorted(words), dtype=np.uint32)
    idx = r.integers(0, colours, width * height)
    idx[r.permutation(width * height)[:colours]] = np.arange(colours)
    return words[idx].view(np.uint8).copy()


# ---- interlaced files (pinned by test_png_adam7_model.py) ----


def cycling_types(width, height, shift):
    """All five filter types in turn from the first row of every pass on; `shift` moves the start, so that over five
    files every pass has begun with every type."""
    return [(r + p + shift) % 5 for p, (_, ph) in enumerate(am.passes(width, height)) for r in range(ph)]


def adam7_file(pix, width, height, depth, colour, types, pre=(), idat_chunks=1, level=6):
    return am.write_file(am.stream_of(pix, width, height, depth, colour, types, level), width, height, depth, colour, pre,
                         idat_chunks, zlib.crc32)


def clear_padding(pix, width, height, depth, colour):
    """The picture with the padding bits of every row zero (what deinterlacing gives)."""
    bits = fm.CHANNELS[colour] * depth
    rb = fm.geometry(width, depth, colour)[0]
    a = np.array(np.frombuffer(bytes(pix), dtype=np.uint8)).reshape(height, rb)
    spare = rb * 8 - width * bits
    if spare:
        a[:, -1] &= (0xFF << spare) & 0xFF
    return a.reshape(-1)


# ---- pictures of every kind the encode plan chooses (pinned by test_png_encode_mixed_model.py) ----


def kinds(r, width, height):
    """RGBA8 pictures (uint8 [height * width * 4]) that are by construction grey-1 / 2 / 4 / 8, palette-1 / 2 / 4 / 8,
    grey-alpha, RGB and RGBA when the plan chooses -> [(name, picture, depth, colour)].  The palette pictures are coloured
    and large enough for the palette's chunks to pay."""
    n = width * height
    out = []
    for d in (1, 2, 4, 8):
        g = r.integers(0, 1 << d, n).astype(np.uint32)
        g[:min(n, 1 << d)] = np.arange(min(n, 1 << d))                 # every level occurs where there is room
        g = g * (255 // ((1 << d) - 1))
        out.append(("grey%d" % d, (g * 0x010101 | 0xFF000000).astype(np.uint32).view(np.uint8), d, 0))
    for d, colours, clear in ((1, 2, 0), (2, 4, 1), (4, 16, 16), (8, 200, 3)):
        out.append(("palette%d" % d, palette_image(r, width, height, colours, clear).reshape(-1), d, 3))
    g = r.integers(0, 256, n).astype(np.uint32)
    a = r.integers(0, 256, n).astype(np.uint32)
    a[0] = 7
    out.append(("grey-alpha", (g * 0x010101 | a << 24).astype(np.uint32).view(np.uint8), 8, 4))
    rgb = r.integers(0, 1 << 24, n).astype(np.uint32)
    rgb[0] = 0x010203
    out.append(("rgb", (rgb | 0xFF000000).astype(np.uint32).view(np.uint8), 8, 2))
    out.append(("rgba", (rgb | a << 24).astype(np.uint32).view(np.uint8), 8, 6))
    return out
