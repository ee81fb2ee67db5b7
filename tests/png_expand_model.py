"""PNG decode to RGBA8 in plain Python integers, one pixel at a time, straight from the PNG specification
(7.2 scanline packing, 11.2.3 PLTE, 11.3.2.1 tRNS, 13.12 sample depth scaling by the exact factors) and
independent of the HIP kernels: the referee for fdh_png_colour_batch and fdh_png_expand_batch.

    to8(s, depth)                       s >> 8, s, s * 255, s * 85, s * 17
    samples(row, width, depth, ch)      the raw samples of one packed row: most significant bits first, 16 bits
                                        big-endian, padding bits ignored
    expand(pix, width, depth, colour, key, pal)   packed rows -> (RGBA bytes, status 0 or 9)
    read_colour(file, info, width, depth, colour) PLTE / tRNS between IHDR and the first IDAT -> (status, pal words,
                                        colour words), the first finding in file order
    write_file(...)                     a file with any chunks between IHDR and IDAT and the stream in several IDATs
"""
from png_file_model import CHANNELS, IEND, SIGNATURE, be32, chunk, crc32, geometry, rd32

OK, SKIPPED, OTHER_GEOMETRY, INDEX_OUTSIDE_PALETTE, BAD_PLTE, BAD_TRNS = 0, 3, 7, 9, 10, 11
SCALE = {1: 255, 2: 85, 4: 17}


def to8(s, depth):
    if depth == 16:
        return s >> 8
    if depth == 8:
        return s
    return s * SCALE[depth]


def samples(row, width, depth, channels):
    """The width * channels raw samples of one packed row."""
    out = []
    if depth == 16:
        for k in range(width * channels):
            out.append((row[2 * k] << 8) | row[2 * k + 1])
    elif depth == 8:
        out = list(row[:width * channels])
    else:
        mask = (1 << depth) - 1
        for k in range(width * channels):
            bit = k * depth
            out.append((row[bit >> 3] >> (8 - depth - (bit & 7))) & mask)
    return out


def pixel(s, depth, colour, key, pal):
    """(r, g, b, a, inside) of one pixel from its raw samples.  key: None or the tRNS values (one for grey, three for
    RGB); pal: the list of (r, g, b, a) PLTE entries with tRNS applied."""
    mask = (1 << depth) - 1
    if colour == 3:
        if s[0] >= len(pal):
            return 0, 0, 0, 255, False
        return pal[s[0]] + (True,)
    if colour == 0:
        g = to8(s[0], depth)
        return g, g, g, 0 if key is not None and s[0] == (key[0] & mask) else 255, True
    if colour == 2:
        hit = key is not None and all(s[c] == (key[c] & mask) for c in range(3))
        return to8(s[0], depth), to8(s[1], depth), to8(s[2], depth), 0 if hit else 255, True
    if colour == 4:
        g = to8(s[0], depth)
        return g, g, g, to8(s[1], depth), True
    return to8(s[0], depth), to8(s[1], depth), to8(s[2], depth), to8(s[3], depth), True


def expand(pix, width, depth, colour, key=None, pal=None):
    """Whole packed rows -> (RGBA8 bytes, status): 9 if a palette index lies at or above len(pal), else 0."""
    pix = bytes(pix)
    rb = geometry(width, depth, colour)[0]
    ch = CHANNELS[colour]
    assert len(pix) % rb == 0
    out, status = bytearray(), OK
    for r in range(len(pix) // rb):
        s = samples(pix[r * rb:(r + 1) * rb], width, depth, ch)
        for x in range(width):
            p = pixel(s[x * ch:(x + 1) * ch], depth, colour, key, pal)
            out += bytes(p[:4])
            if not p[4]:
                status = INDEX_OUTSIDE_PALETTE
    return bytes(out), status


def palette(plte, trns=b""):
    """[(r, g, b, a)] from the bodies of a PLTE and a tRNS chunk."""
    return [(plte[3 * k], plte[3 * k + 1], plte[3 * k + 2], trns[k] if k < len(trns) else 255) for k in range(len(plte) // 3)]


def pal_words(pal):
    """The 256 words fdh_png_colour_batch writes: R | G << 8 | B << 16 | A << 24, 0xFF000000 behind the entries."""
    return [r | g << 8 | b << 16 | a << 24 for r, g, b, a in pal] + [0xFF000000] * (256 - len(pal))


def colour_words(count, key):
    """The four words: count, key present, R or grey | G << 16, B."""
    k = list(key or ()) + [0, 0, 0]
    return [count, 1 if key else 0, k[0] | k[1] << 16, k[2]]


def read_colour(f, info, width, depth, colour):
    """fdh_png_colour_batch on one file whose scan record is `info` (png_file_model.Info)
    -> (status, pal or None, key or None): the first finding in file order."""
    f = bytes(f)
    if info.status != 0:
        return SKIPPED, None, None
    if (info.width, info.bit_depth, info.colour_type) != (width, depth, colour):
        return OTHER_GEOMETRY, None, None
    pos, plte, trns = 8, None, None
    while pos < info.first_idat:
        n, tag = rd32(f, pos), f[pos + 4:pos + 8]
        body = f[pos + 8:pos + 8 + n]
        if tag == b"PLTE" and colour == 3:
            if plte is not None or n == 0 or n % 3 or n > 768:
                return BAD_PLTE, None, None
            plte = body
        elif tag == b"tRNS" and colour in (0, 2, 3):
            if trns is not None or (colour == 0 and n != 2) or (colour == 2 and n != 6):
                return BAD_TRNS, None, None
            if colour == 3 and (plte is None or n > len(plte) // 3):
                return BAD_TRNS, None, None
            trns = body
        pos += 12 + n
    if colour == 3:
        if plte is None:
            return BAD_PLTE, None, None
        return OK, palette(plte, trns or b""), None
    key = None
    if trns is not None:
        key = tuple((trns[2 * c] << 8) | trns[2 * c + 1] for c in range(len(trns) // 2))
    return OK, None, key


def trns_body(key):
    return b"".join(bytes([(v >> 8) & 0xFF, v & 0xFF]) for v in key)


def plte_body(pal):
    return b"".join(bytes(e[:3]) for e in pal)


def write_file(idat, width, height, depth, colour, pre=(), idat_chunks=1, crc=crc32):
    """Signature, IHDR, the chunks `pre` ((tag, body) pairs: PLTE, tRNS, tEXt .. in the given order), the zlib stream
    `idat` cut into `idat_chunks` IDAT chunks, IEND."""
    ihdr = be32(width) + be32(height) + bytes([depth, colour, 0, 0, 0])
    f = SIGNATURE + chunk(b"IHDR", ihdr, crc)
    for tag, body in pre:
        f += chunk(tag, bytes(body), crc)
    cut = [len(idat) * k // idat_chunks for k in range(idat_chunks + 1)]
    for a, b in zip(cut[:-1], cut[1:]):
        f += chunk(b"IDAT", idat[a:b], crc)
    return f + IEND
