"""PNG encode from RGBA8 in plain Python integers, one pixel at a time, straight from the PNG specification (7.2
scanline packing, 11.2.3 PLTE, 11.3.2.1 tRNS, 13.12 sample depth scaling) and independent of the HIP kernels: the
referee for fdh_png_analyse_batch, fdh_png_pack_batch and fdh_png_frame_palette_batch.

    analyse(rgba, width, max_colours)   -> (status, pal words or None, count, trns_len, summary)
    pack(rgba, width, depth, colour, pal, count)   RGBA8 rows -> (packed rows, status 0 or 13)
    palette_file_prefix(E, T)           41 + 12 + 3 E + (T ? 12 + T : 0)
    write_palette_file(...)             signature, IHDR, PLTE of E entries, tRNS of T bytes, ONE IDAT, IEND
    frame_palette_status(...)           2, 10, 11 or 0, the first that applies
"""
from png_expand_model import plte_body
from png_file_model import CHANNELS, IEND, PREFIX, SIGNATURE, SUFFIX, be32, chunk, crc32, geometry

OK, BAD_SIZES, BAD_PLTE, BAD_TRNS, TOO_MANY_COLOURS, NOT_REPRESENTABLE = 0, 2, 10, 11, 12, 13
OPAQUE, GREY = 1, 2
UNIT = {1: 255, 2: 85, 4: 17, 8: 1}


def words(rgba):
    """The pixel words R | G << 8 | B << 16 | A << 24 of RGBA8 bytes."""
    rgba = bytes(rgba)
    return [rgba[k] | rgba[k + 1] << 8 | rgba[k + 2] << 16 | rgba[k + 3] << 24 for k in range(0, len(rgba), 4)]


def summary_of(px):
    """Bit 0: every A is 255; bit 1: every pixel is grey; bits 8 .. 15: the smallest depth of 1, 2, 4, 8 whose unit
    255 / (2^d - 1) divides every R, G and B.  No pixels: both bits, depth 1."""
    opaque = all(w >> 24 == 255 for w in px)
    grey = all(w & 0xFF == (w >> 8) & 0xFF == (w >> 16) & 0xFF for w in px)
    depth = 8
    for d in (1, 2, 4):
        if all(((w >> s) & 0xFF) % UNIT[d] == 0 for w in px for s in (0, 8, 16)):
            depth = d
            break
    return (OPAQUE if opaque else 0) | (GREY if grey else 0) | depth << 8


def analyse(rgba, width, max_colours):
    """fdh_png_analyse_batch on one image -> (status, pal, count, trns_len, summary).  Status 2: everything else is
    None (nothing is written).  Status 12: pal, count and trns_len are None (not specified), the summary is valid.
    pal: the 256 words, the distinct pixels in ascending order, then 0xFF000000."""
    rgba = bytes(rgba)
    if len(rgba) % (4 * width):
        return BAD_SIZES, None, None, None, None
    px = words(rgba)
    summary = summary_of(px)
    distinct = sorted(set(px))
    if len(distinct) > max_colours:
        return TOO_MANY_COLOURS, None, None, None, summary
    trns_len = sum(1 for w in distinct if w >> 24 < 255)
    return OK, distinct + [0xFF000000] * (256 - len(distinct)), len(distinct), trns_len, summary


def pixel_samples(w, depth, colour, pal, count):
    """The raw samples of the pixel word w in the pair, or None where it has no lossless representation."""
    r, g, b, a = w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24
    if colour == 3:
        for k in range(min(count, len(pal))):
            if pal[k] == w:
                return [k] if k < 1 << depth else None
        return None
    if colour in (0, 2) and a != 255:
        return None
    if colour in (0, 4) and not r == g == b:
        return None
    if colour == 0:
        if depth < 8:
            if r % UNIT[depth]:
                return None
            return [r // UNIT[depth]]
        s = [r]
    elif colour == 2:
        s = [r, g, b]
    elif colour == 4:
        s = [r, a]
    else:
        s = [r, g, b, a]
    return [v * 257 for v in s] if depth == 16 else s


def pack(rgba, width, depth, colour, pal=None, count=256):
    """Whole RGBA8 rows -> (packed rows, status).  Status 13: some pixel cannot be held; the bytes are then not
    specified (here: that pixel's samples are zeros).  pal: the palette's words (colour type 3), `count` of them in use."""
    rgba = bytes(rgba)
    assert len(rgba) % (4 * width) == 0
    rb = geometry(width, depth, colour)[0]
    ch = CHANNELS[colour]
    px = words(rgba)
    known = {}          # (a pixel word's samples are worked out once)
    out, status = bytearray(), OK
    for r in range(len(px) // width):
        row = bytearray(rb)
        for x in range(width):
            w = px[r * width + x]
            if w not in known:
                known[w] = pixel_samples(w, depth, colour, pal, count)
            s = known[w]
            if s is None:
                status = NOT_REPRESENTABLE
                s = [0] * ch
            for c, v in enumerate(s):
                k = x * ch + c
                if depth == 16:
                    row[2 * k], row[2 * k + 1] = v >> 8, v & 0xFF
                elif depth == 8:
                    row[k] = v
                else:
                    bit = k * depth
                    row[bit >> 3] |= v << (8 - depth - (bit & 7))
        out += row
    return bytes(out), status


def palette_file_prefix(entries, alphas):
    return PREFIX + 12 + 3 * entries + (12 + alphas if alphas else 0)


def frame_palette_status(idat_len, height, slot, count, trns_len, entries, alphas):
    """fdh_png_frame_palette_batch's status: 2 on fdh_png_frame_batch's conditions, then 10, then 11."""
    if idat_len == 0 or idat_len > 0x7FFFFFFF or idat_len + palette_file_prefix(entries, alphas) + SUFFIX > slot or height == 0 or height > 0x7FFFFFFF:
        return BAD_SIZES
    if count == 0 or count > entries:
        return BAD_PLTE
    if trns_len > alphas:
        return BAD_TRNS
    return OK


def write_palette_file(idat, width, height, depth, pal, count, entries, alphas, crc=crc32):
    """The file fdh_png_frame_palette_batch makes around the zlib stream `idat`: a PLTE of `entries` entries, the first
    `count` words of `pal` and then 0, 0, 0; where alphas > 0 a tRNS of that many bytes, the entries' alphas and then 255."""
    own = [(w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24) for w in pal[:count]]
    filled = own + [(0, 0, 0, 255)] * (entries - count)
    ihdr = be32(width) + be32(height) + bytes([depth, 3, 0, 0, 0])
    f = SIGNATURE + chunk(b"IHDR", ihdr, crc) + chunk(b"PLTE", plte_body(filled[:entries]), crc)
    if alphas:
        f += chunk(b"tRNS", bytes(e[3] for e in filled[:alphas]), crc)
    f += be32(len(idat)) + b"IDAT"
    assert len(f) == palette_file_prefix(entries, alphas)
    return f + idat + be32(crc(b"IDAT" + idat) & 0xFFFFFFFF) + IEND
