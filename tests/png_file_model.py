"""The PNG container in plain Python integers, straight from the PNG specification (5.2 signature,
5.3 chunk layout, 5.5 / annex D CRC, 5.6 chunk ordering, 11.2.2 IHDR) and independent of the HIP
kernels: the referee for fdh_crc32_batch, fdh_png_frame_batch, fdh_png_scan_files_batch and
fdh_png_gather_idat_batch.  No compiled code, no zlib, no struct.

    crc32(data, seed)          one bit at a time: polynomial 0xEDB88320, reflected, register preset to
                               all ones and complemented at the end (a seed is the CRC of what came before)
    combine(crc_a, crc_b, n)   crc(A || B) from crc(A), crc(B) and n = |B|:  crc(A) * x^(8 n) mod P  xor  crc(B)
    write_file(...)            signature, IHDR, ONE IDAT, IEND: 41 bytes in front of the stream, 16 behind
    scan(file)                 the fields of fdh_png_info and its status codes, by the stated precedence
"""
POLY = 0xEDB88320
SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
PREFIX, SUFFIX = 41, 16
IEND = bytes([0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82])

# status codes of fdh_png_info.status
OK, NO_SIGNATURE, TRUNCATED, BAD_IHDR, INTERLACED, CHUNK_STRUCTURE, CRC_MISMATCH = range(7)
# png_status of fdh_png_gather_idat_batch
SKIPPED, OTHER_GEOMETRY, SLOT_TOO_SMALL = 3, 7, 8

# the fifteen pairs of the specification's table 11.1: colour type -> allowed bit depths
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
PAIRS = tuple((d, c) for c in sorted(DEPTHS) for d in DEPTHS[c])
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def crc32(data, seed=0):
    c = (seed ^ 0xFFFFFFFF) & 0xFFFFFFFF
    for v in bytes(data):
        c ^= v
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def mulmod(a, b):
    """a * b mod P on reflected 32-bit polynomials (bit 31 is x^0)."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow(n):
    """x^n mod P from the 32 constants x^(2^k); the order of x divides 2^32 - 1."""
    n %= 0xFFFFFFFF
    p, sq, k = 0x80000000, 0x40000000, 0
    while n >> k:
        if (n >> k) & 1:
            p = mulmod(p, sq)
        sq = mulmod(sq, sq)
        k += 1
    return p


def combine(crc_a, crc_b, len_b):
    return mulmod(crc_a, xpow(8 * len_b)) ^ crc_b


def be32(v):
    return bytes([(v >> 24) & 0xFF, (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF])


def rd32(b, at):
    return (b[at] << 24) | (b[at + 1] << 16) | (b[at + 2] << 8) | b[at + 3]


def chunk(tag, body, crc=crc32):
    return be32(len(body)) + tag + body + be32(crc(tag + body) & 0xFFFFFFFF)


def geometry(width, bit_depth, colour_type):
    """(row_bytes, bpp) of packed scanlines: row_bytes = ceil(width * channels * depth / 8),
    bpp = max(1, channels * depth / 8)."""
    bits = CHANNELS[colour_type] * bit_depth
    return (width * bits + 7) // 8, max(1, bits // 8)


def write_file(idat, width, height, bit_depth, colour_type, crc=crc32):
    """The file fdh_png_frame_batch makes around the zlib stream `idat`.  `crc`: another CRC-32 function of the same
    signature (tests with many large files pass zlib's, which tests/test_png_file_model.py pins to the one above)."""
    ihdr = be32(width) + be32(height) + bytes([bit_depth, colour_type, 0, 0, 0])
    f = SIGNATURE + chunk(b"IHDR", ihdr, crc) + be32(len(idat)) + b"IDAT"
    assert len(f) == PREFIX
    f += idat + be32(crc(b"IDAT" + idat) & 0xFFFFFFFF) + IEND
    assert len(f) == len(idat) + PREFIX + SUFFIX
    return f


class Info:
    FIELDS = ("status", "width", "height", "bit_depth", "colour_type", "interlace", "idat_bytes", "idat_chunks", "first_idat", "chunks")

    def __init__(self):
        for k in self.FIELDS:
            setattr(self, k, 0)
        self.idat = b""    # the concatenated IDAT bodies (not a field of fdh_png_info)

    def fields(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def __repr__(self):
        return "Info(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k in self.FIELDS)


def scan(f, ignore_crc=False, crc=crc32):
    """fdh_png_scan_files_batch on one file: the first structural finding in file order ends the walk
    (the counts then hold what came before it); with none, CRC_MISMATCH if any chunk's CRC differs.
    `crc` as for write_file."""
    f = bytes(f)
    r = Info()
    if len(f) < 8 or f[:8] != SIGNATURE:
        r.status = NO_SIGNATURE
        return r
    pos, seen_idat, idat_over, crc_ok = 8, False, False, True
    while True:
        if pos + 12 > len(f):
            r.status = TRUNCATED      # also: the file ended and there was no IEND
            return r
        n, tag = rd32(f, pos), f[pos + 4:pos + 8]
        if r.chunks == 0 and (tag != b"IHDR" or n != 13):
            r.status = BAD_IHDR
            return r
        if pos + 12 + n > len(f):
            r.status = TRUNCATED
            return r
        body = f[pos + 8:pos + 8 + n]
        if r.chunks == 0:
            r.width, r.height = rd32(body, 0), rd32(body, 4)
            r.bit_depth, r.colour_type, r.interlace = body[8], body[9], body[12]
            if (r.width == 0 or r.height == 0 or r.width >> 31 or r.height >> 31 or (body[8], body[9]) not in PAIRS
                    or body[10] != 0 or body[11] != 0 or body[12] > 1):
                r.status = BAD_IHDR
                return r
            if body[12] == 1:
                r.status = INTERLACED
                return r
        elif tag == b"IDAT":
            if idat_over:
                r.status = CHUNK_STRUCTURE
                return r
            if not seen_idat:
                r.first_idat = pos
            seen_idat = True
            r.idat_bytes += n
            r.idat_chunks += 1
            r.idat += body
        else:
            if seen_idat:
                idat_over = True
            if tag == b"IEND":
                bad = not seen_idat
            elif tag == b"PLTE":
                bad = seen_idat
            else:
                bad = not (tag[0] & 0x20)     # an upper-case first letter: a critical chunk, and none known here
            if bad:
                r.status = CHUNK_STRUCTURE
                return r
        crc_ok = crc_ok and (ignore_crc or crc(tag + body) & 0xFFFFFFFF == rd32(f, pos + 8 + n))
        r.chunks += 1
        pos += 12 + n
        if tag == b"IEND":
            break
    if not crc_ok and not ignore_crc:
        r.status = CRC_MISMATCH
    return r
