"""Adam7 interlacing (PNG specification 8.2 "Interlace methods", 9.2 filtering of the reduced images) in plain Python
integers, one pixel at a time and independent of the HIP kernels: the referee for fdh_png_adam7_size and
fdh_png_unfilter_interlaced_batch, and the writer of the interlaced files the tests read (Pillow reads Adam7 files
but cannot write them).  Built on png_model (the filters), png_file_model (chunks, geometry) and png_expand_model
(samples, the file writer's chunk order).

    X0, Y0, DX, DY             the pass tables
    passes(width, height)      [(pw, ph)] of the seven reduced images, (0, 0) for an empty one
    size(width, height, depth, colour)   bytes of the decoded IDAT stream
    interlace(pix, ...)        packed picture -> the seven reduced images, packed (b"" for an empty one)
    deinterlace(images, ...)   and back; padding bits of the picture's rows are zero
    filter_passes(images, ..., types)    the IDAT stream's bytes: every pass filtered as an image of its own, one
                               type per pass row, the row above a pass's first row zeros
    unfilter_passes(stream, ...)         and back -> the reduced images
    write_file(...)            an Adam7 file: IHDR with interlace method 1 (or any other value), chunks in front, the
                               stream in any number of IDAT chunks
    decode(file)               file -> packed pixels of the picture, whichever the interlace method
"""
import zlib

import numpy as np

import png_file_model as fm
import png_model as pm

X0 = (0, 4, 0, 2, 0, 1, 0)
Y0 = (0, 0, 4, 0, 2, 0, 1)
DX = (8, 8, 4, 4, 2, 2, 1)
DY = (8, 8, 8, 4, 4, 2, 2)


def passes(width, height):
    out = []
    for p in range(7):
        pw = max(0, -((X0[p] - width) // DX[p]))      # ceil((width - x0) / dx)
        ph = max(0, -((Y0[p] - height) // DY[p]))
        out.append((pw, ph) if pw and ph else (0, 0))
    return out


def size(width, height, depth, colour):
    if (depth, colour) not in fm.PAIRS or width <= 0 or height <= 0:
        return 0
    bits = fm.CHANNELS[colour] * depth
    return sum(ph * (1 + (pw * bits + 7) // 8) for pw, ph in passes(width, height))


def _get(row, x, bits):
    """Pixel x of a packed row as an integer of `bits` bits."""
    if bits >= 8:
        n = bits // 8
        return int.from_bytes(row[x * n:(x + 1) * n], "big")
    bit = x * bits
    return (row[bit >> 3] >> (8 - bits - (bit & 7))) & ((1 << bits) - 1)


def _put(row, x, bits, v):
    if bits >= 8:
        n = bits // 8
        row[x * n:(x + 1) * n] = v.to_bytes(n, "big")
    else:
        bit = x * bits
        row[bit >> 3] |= v << (8 - bits - (bit & 7))


def interlace(pix, width, height, depth, colour):
    """Packed rows of the picture -> the seven reduced images as packed rows (padding bits zero)."""
    pix = bytes(pix)
    bits = fm.CHANNELS[colour] * depth
    rb = (width * bits + 7) // 8
    assert len(pix) == height * rb
    out = []
    for p, (pw, ph) in enumerate(passes(width, height)):
        prb = (pw * bits + 7) // 8
        img = bytearray(ph * prb)
        for r in range(ph):
            src = pix[(Y0[p] + r * DY[p]) * rb:(Y0[p] + r * DY[p] + 1) * rb]
            row = bytearray(prb)
            for j in range(pw):
                _put(row, j, bits, _get(src, X0[p] + j * DX[p], bits))
            img[r * prb:(r + 1) * prb] = row
        out.append(bytes(img))
    return out


def deinterlace(images, width, height, depth, colour):
    """The seven reduced images -> packed rows of the picture; padding bits of every row zero."""
    bits = fm.CHANNELS[colour] * depth
    rb = (width * bits + 7) // 8
    rows = [bytearray(rb) for _ in range(height)]
    for p, (pw, ph) in enumerate(passes(width, height)):
        prb = (pw * bits + 7) // 8
        assert len(images[p]) == ph * prb
        for r in range(ph):
            src = images[p][r * prb:(r + 1) * prb]
            for j in range(pw):
                _put(rows[Y0[p] + r * DY[p]], X0[p] + j * DX[p], bits, _get(src, j, bits))
    return b"".join(bytes(r) for r in rows)


def pass_rows(width, height):
    """Rows of all passes together: the number of filter types a file has."""
    return sum(ph for _, ph in passes(width, height))


def filter_passes(images, width, height, depth, colour, types):
    """The decoded IDAT stream of an interlaced image: pass after pass, every row of a pass with its type byte, filtered
    with the pixel size of the full image, the row above a pass's first row zeros.  `types`: one per pass row, in
    stream order."""
    bits = fm.CHANNELS[colour] * depth
    bpp = max(1, bits // 8)
    out, at = b"", 0
    for p, (pw, ph) in enumerate(passes(width, height)):
        if not ph:
            continue
        prb = (pw * bits + 7) // 8
        img = np.frombuffer(images[p], dtype=np.uint8).reshape(ph, prb)
        out += pm.filter_rows(img, bpp, list(types[at:at + ph])).tobytes()
        at += ph
    assert at == len(types)
    return out


def unfilter_passes(stream, width, height, depth, colour):
    """The inverse: the stream's bytes -> the seven reduced images (ValueError on a filter type above 4)."""
    bits = fm.CHANNELS[colour] * depth
    bpp = max(1, bits // 8)
    stream = bytes(stream)
    assert len(stream) == size(width, height, depth, colour)
    out, at = [], 0
    for pw, ph in passes(width, height):
        prb = (pw * bits + 7) // 8
        n = ph * (prb + 1) if ph else 0
        out.append(pm.unfilter(stream[at:at + n], prb, bpp) if n else b"")
        at += n
    return out


def stream_of(pix, width, height, depth, colour, types, level=6):
    """The zlib stream of the interlaced picture."""
    return zlib.compress(filter_passes(interlace(pix, width, height, depth, colour), width, height, depth, colour, types), level)


def write_file(idat, width, height, depth, colour, pre=(), idat_chunks=1, crc=fm.crc32, method=1):
    """Signature, IHDR with the given interlace method, the chunks `pre` ((tag, body) pairs), the zlib stream `idat` cut
    into `idat_chunks` IDAT chunks, IEND."""
    ihdr = fm.be32(width) + fm.be32(height) + bytes([depth, colour, 0, 0, method])
    f = fm.SIGNATURE + fm.chunk(b"IHDR", ihdr, crc)
    for tag, body in pre:
        f += fm.chunk(tag, bytes(body), crc)
    cut = [len(idat) * k // idat_chunks for k in range(idat_chunks + 1)]
    for a, b in zip(cut[:-1], cut[1:]):
        f += fm.chunk(b"IDAT", idat[a:b], crc)
    return f + fm.IEND


def scan(f, adam7=False, ignore_crc=False, crc=fm.crc32):
    """fdh_png_scan_files_batch with or without FDH_PNG_FLAG_ADAM7: with the flag a file of interlace method 1 is
    walked like the same file with method 0 (the IHDR's CRC is checked over the bytes as they are), and `interlace`
    says 1; without it, png_file_model.scan as it is."""
    f = bytes(f)
    plain = fm.scan(f, ignore_crc, crc)
    if not adam7 or plain.status != fm.INTERLACED:
        return plain
    g = bytearray(f)
    g[28] = 0                                              # the interlace byte of the IHDR
    g[29:33] = fm.be32(crc(bytes(g[12:29])) & 0xFFFFFFFF)
    r = fm.scan(bytes(g), ignore_crc, crc)
    r.interlace = 1
    if r.status == fm.OK and not ignore_crc and crc(f[12:29]) & 0xFFFFFFFF != fm.rd32(f, 29):
        r.status = fm.CRC_MISMATCH                         # (the IHDR's own CRC is judged on the file's bytes)
    return r


def decode(f, crc=zlib.crc32):
    """A sound file -> (width, height, depth, colour, packed pixels of the picture)."""
    info = scan(f, adam7=True, crc=crc)
    assert info.status == 0, info
    w, h, d, c = info.width, info.height, info.bit_depth, info.colour_type
    raw = zlib.decompress(info.idat)
    rb, bpp = fm.geometry(w, d, c)
    if info.interlace == 0:
        return w, h, d, c, pm.unfilter(raw, rb, bpp)
    return w, h, d, c, deinterlace(unfilter_passes(raw, w, h, d, c), w, h, d, c)
