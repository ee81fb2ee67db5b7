"""PNG encode of mixed batches of RGBA16 pictures in plain Python integers, independent of the HIP code: the referee for
fdh_png_analyse16_mixed_batch, fdh_png_encode16_plan_one / _batch and fdh_png_pack16_mixed_batch
(include/fdeflate_hip_png16_encode.h).  It builds on the models of the RGBA8 pipeline and of depth 16: a picture whose
samples are all narrow (both bytes equal) is the RGBA8 picture of its high bytes.

    pixels16(rgba16)                  [(r, g, b, a)] of little-endian RGBA16 bytes
    narrow(px) / high_bytes(rgba16)   every sample is 257 * its high byte / the RGBA8 picture of the high bytes
    summary16_of(px)                  bits 0, 1, 2 and the depth 1, 2, 4, 8 or 16 in bits 8 .. 15
    analyse16(rgba16, width, max_colours)   -> (status, pal words or None, count, trns_len, summary)
    plan16(r, count, trns_len, summary, analyse_status, allowed)
                                      -> (status, depth, colour, packed, types, prefix, file), over png_encode_mixed_model.plan
    pack16_any(rgba16, width, depth, colour, pal, count)   -> (packed rows, status 0 or 13), any of the fifteen pairs
    encode16(rgba16, width, height, ...)    analyse16 -> plan16 -> pack16_any -> filter -> compress -> write_file
"""
import zlib

import numpy as np

import png16_model as m16
import png_encode_mixed_model as em
import png_file_model as fm
import png_mixed_model as mm
import png_model
import png_pack_model as pm

OK, BAD_SIZES, TOO_MANY_COLOURS, NOT_REPRESENTABLE = 0, 2, 12, 13
OPAQUE, GREY, NARROW = 1, 2, 4
UNIT16 = m16.SCALE16                     # 65535 / (2^d - 1)
WIDE_PAIRS = ((0, 16), (2, 16), (4, 16), (6, 16))      # (colour, depth), ascending colour types


def pixels16(rgba16):
    rgba16 = bytes(rgba16)
    s = [rgba16[k] | rgba16[k + 1] << 8 for k in range(0, len(rgba16), 2)]
    return [tuple(s[k:k + 4]) for k in range(0, len(s), 4)]


def narrow(px):
    return all(v == 257 * (v >> 8) for p in px for v in p)


def high_bytes(rgba16):
    """The RGBA8 picture of the high bytes (little-endian samples: every second byte)."""
    return bytes(rgba16)[1::2]


def summary16_of(px):
    """Bit 0: every A is 65535; bit 1: R == G == B on all 16 bits; bit 2: every sample is narrow; bits 8 .. 15: the
    smallest depth of 1, 2, 4, 8, 16 whose unit 65535 / (2^d - 1) divides every R, G and B.  No pixels: all three, depth 1."""
    opaque = all(p[3] == 65535 for p in px)
    grey = all(p[0] == p[1] == p[2] for p in px)
    depth = next(d for d in (1, 2, 4, 8, 16) if all(v % UNIT16[d] == 0 for p in px for v in p[:3]))
    return (OPAQUE if opaque else 0) | (GREY if grey else 0) | (NARROW if narrow(px) else 0) | depth << 8


def analyse16(rgba16, width, max_colours=256):
    """fdh_png_analyse16_mixed_batch on one picture -> (status, pal, count, trns_len, summary).  Status 2: everything
    else is None.  Status 12 (a sample that is not narrow, or too many colours): pal, count, trns_len are None, the
    summary is valid.  Else they are png_pack_model.analyse's for the high bytes."""
    rgba16 = bytes(rgba16)
    if len(rgba16) % (8 * width):
        return BAD_SIZES, None, None, None, None
    px = pixels16(rgba16)
    summary = summary16_of(px)
    if not summary & NARROW:
        return TOO_MANY_COLOURS, None, None, None, summary
    status, pal, count, trns_len, s8 = pm.analyse(high_bytes(rgba16), width, max_colours)
    assert s8 == summary & ~NARROW                     # the high bytes' summary is this one's
    return status, pal, count, trns_len, summary


def plan16(r, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    """fdh_png_encode16_plan_one -> (status, depth, colour, packed, types, prefix, file)."""
    if not em.dimension(r) or summary & NARROW:
        return em.plan(r, count, trns_len, summary & ~NARROW, analyse_status, allowed)
    fail = lambda st: (st, 0, 0, 0, 0, 0, 0)
    if analyse_status not in (0, TOO_MANY_COLOURS):
        return fail(analyse_status)
    opaque, grey = bool(summary & OPAQUE), bool(summary & GREY)
    ok = {0: opaque and grey, 2: opaque, 4: grey, 6: True}
    mask = allowed or em.ALL_TYPES
    costed = [(r["height"] * em.row_bytes(r["width"], depth, colour), colour, depth)
              for colour, depth in WIDE_PAIRS if ok[colour] and mask >> colour & 1]
    if not costed:
        return fail(NOT_REPRESENTABLE)
    _, colour, depth = min(costed)                     # the smallest cost, then the lower colour type
    st, _, _, packed, types, prefix, size = em.plan(mm.record(r["width"], r["height"], depth, colour))
    return (st, depth, colour, packed, types, prefix, size) if st == OK else fail(st)


def pack16_any(rgba16, width, depth, colour, pal=None, count=256):
    """fdh_png_pack16_mixed_batch on one picture -> (packed rows, status).  Depth 16: png16_model.pack16.  Below: 13
    where a sample is not narrow (the bytes are then not specified: here None), else png_pack_model.pack of the high bytes."""
    if depth == 16:
        return m16.pack16(rgba16, width, colour)
    if not narrow(pixels16(rgba16)):
        return None, NOT_REPRESENTABLE
    return pm.pack(high_bytes(rgba16), width, depth, colour, pal, count)


def encode16(rgba16, width, height, allowed=0, pair=None, compress=zlib.compress, choose=None, crc=zlib.crc32):
    """One RGBA16 picture (bytes, height * width * 8) to a file -> (status, file or None, depth, colour), as
    png_encode_mixed_model.encode."""
    rgba16 = bytes(rgba16)
    depth, colour = pair or (0, 0)
    r = mm.record(width, height, depth, colour)
    if len(rgba16) != height * width * 8:
        return BAD_SIZES, None, depth, colour
    a_status, pal, count, trns_len, summary = analyse16(rgba16, width, 256)
    st, depth, colour, packed, _, prefix, _ = plan16(r, count, trns_len, summary, a_status, allowed)
    if st != OK:
        if pair and colour == 3 and a_status == TOO_MANY_COLOURS:
            st = TOO_MANY_COLOURS
        return st, None, depth, colour
    pix, st = pack16_any(rgba16, width, depth, colour, pal, count or 256)
    if st != OK:
        return st, None, depth, colour
    assert len(pix) == packed
    rb, bpp = fm.geometry(width, depth, colour)
    rows = np.frombuffer(pix, dtype=np.uint8).reshape(height, rb)
    types = choose(rows, bpp) if choose else [0] * height
    idat = compress(png_model.filter_rows(rows, bpp, list(types)).tobytes())
    f = em.write_file(idat, width, height, depth, colour, pal, count or 0, trns_len or 0, crc)
    assert len(f) == prefix + len(idat) + 16
    return OK, f, depth, colour
