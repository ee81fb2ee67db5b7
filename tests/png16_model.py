"""PNG decode to and encode from RGBA16 in plain Python integers, one pixel at a time, straight from the PNG
specification (13.12: sample depth scaling by the exact factors 65535 / (2^depth - 1)) and independent of the HIP
kernels: the referee for fdh_png_expand16_batch and fdh_png_pack16_batch.  It builds on png_expand_model: the raw
samples of a row, the PLTE / tRNS reader and the file writer are that model's.

    to16(s, depth)                      s, s * 257, s * 4369, s * 21845, s * 65535
    expand16(pix, width, depth, colour, key, pal)   packed rows -> (little-endian RGBA16 bytes, status 0 or 9)
    pack16(rgba16, width, colour)       little-endian RGBA16 bytes -> (packed rows of depth 16, status 0 or 13)
"""
from png_expand_model import INDEX_OUTSIDE_PALETTE, OK, read_colour, samples, write_file  # noqa: F401 (read_colour, write_file: for the tests)
from png_file_model import CHANNELS, geometry

NOT_REPRESENTABLE = 13
SCALE16 = {1: 65535, 2: 21845, 4: 4369, 8: 257, 16: 1}


def to16(s, depth):
    return s * SCALE16[depth]


def pixel16(s, depth, colour, key, pal):
    """(r, g, b, a, inside) of one pixel, 16 bits each, from its raw samples.  key: None or the tRNS values (one for
    grey, three for RGB), compared on the raw samples at the file's depth; pal: the list of (r, g, b, a) PLTE entries
    with tRNS applied, eight bits each."""
    mask = (1 << depth) - 1
    if colour == 3:
        if s[0] >= len(pal):
            return 0, 0, 0, 65535, False
        return tuple(v * 257 for v in pal[s[0]]) + (True,)
    if colour == 0:
        g = to16(s[0], depth)
        return g, g, g, 0 if key is not None and s[0] == (key[0] & mask) else 65535, True
    if colour == 2:
        hit = key is not None and all(s[c] == (key[c] & mask) for c in range(3))
        return to16(s[0], depth), to16(s[1], depth), to16(s[2], depth), 0 if hit else 65535, True
    if colour == 4:
        g = to16(s[0], depth)
        return g, g, g, to16(s[1], depth), True
    return to16(s[0], depth), to16(s[1], depth), to16(s[2], depth), to16(s[3], depth), True


def expand16(pix, width, depth, colour, key=None, pal=None):
    """Whole packed rows -> (RGBA16 bytes, each sample little-endian, status): 9 if a palette index lies at or above
    len(pal), else 0."""
    pix = bytes(pix)
    rb = geometry(width, depth, colour)[0]
    ch = CHANNELS[colour]
    assert len(pix) % rb == 0
    out, status = bytearray(), OK
    for r in range(len(pix) // rb):
        s = samples(pix[r * rb:(r + 1) * rb], width, depth, ch)
        for x in range(width):
            p = pixel16(s[x * ch:(x + 1) * ch], depth, colour, key, pal)
            for v in p[:4]:
                out += bytes((v & 0xFF, v >> 8))
            if not p[4]:
                status = INDEX_OUTSIDE_PALETTE
    return bytes(out), status


def pack16(rgba16, width, colour):
    """Little-endian RGBA16 bytes of whole rows -> (packed rows of depth 16, samples big-endian, status): 13 if colour
    type 0 or 4 meets a pixel with R, G, B not all equal, or colour type 0 or 2 one with A != 65535 (the bytes are then
    not specified: here the samples the colour type keeps), else 0.  No key is written."""
    rgba16 = bytes(rgba16)
    assert colour in (0, 2, 4, 6) and len(rgba16) % (width * 8) == 0
    out, status = bytearray(), OK
    for p in range(len(rgba16) // 8):
        r, g, b, a = (rgba16[8 * p + 2 * c] | rgba16[8 * p + 2 * c + 1] << 8 for c in range(4))
        if colour in (0, 4) and not r == g == b:
            status = NOT_REPRESENTABLE
        if colour in (0, 2) and a != 65535:
            status = NOT_REPRESENTABLE
        kept = {0: (r,), 2: (r, g, b), 4: (r, a), 6: (r, g, b, a)}[colour]
        for v in kept:
            out += bytes((v >> 8, v & 0xFF))
    return bytes(out), status
