"""PNG encode of mixed batches in plain Python integers, independent of the HIP code: the referee for
fdh_png_encode_plan_one / fdh_png_encode_plan_batch and for the files fdh_png_frame_mixed_batch makes.

    encodable(r) / dimension(r)       the two kinds of record the encode steps take
    plan(r, count, trns_len, summary, analyse_status, allowed)
                                      -> (status, depth, colour, packed, types, prefix, file)
    write_file(...)                   an exact-palette file (a PLTE of `count` entries, a tRNS of `trns_len` bytes) or a
                                      plain one around a zlib stream, from png_pack_model and png_file_model
    encode(rgba, width, height, ...)  analyse -> plan -> pack -> filter -> compress -> write_file for one picture

Records are png_mixed_model's dictionaries.  The rules are those of include/fdeflate_hip.h, "PNG encode: mixed batches".
"""
import zlib

import numpy as np

import png_file_model as fm
import png_mixed_model as mm
import png_model
import png_pack_model as pm

OK, BAD_SIZES, SKIPPED, BAD_PLTE, BAD_TRNS, TOO_MANY_COLOURS, NOT_REPRESENTABLE = 0, 2, 3, 10, 11, 12, 13
ALL_TYPES = (1 << 0) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 6)
ROW_LIMIT, FILTERED_LIMIT = 1 << 25, 1 << 31     # the filter chooser's and the fused encoder's


def ultrafast_bound(n):
    return 53 + (5 + 12 * n + 12 + 7) // 8 + 4


def _sides_ok(r):
    return r["status"] == 0 and 1 <= r["width"] <= 0x7FFFFFFF and 1 <= r["height"] <= 0x7FFFFFFF and r["interlace"] == 0


def encodable(r):
    return _sides_ok(r) and (r["bit_depth"], r["colour_type"]) in fm.PAIRS


def dimension(r):
    return _sides_ok(r) and r["bit_depth"] == 0 and r["colour_type"] == 0


def row_bytes(width, depth, colour):
    return (width * fm.CHANNELS[colour] * depth + 7) // 8


def prefix_of(colour, count, trns_len):
    return 41 + (12 + 3 * count + (12 + trns_len if trns_len else 0) if colour == 3 else 0)


def candidates(r, count, trns_len, summary, analyse_status, allowed):
    """[(cost, colour, depth)] of a dimension record, in no order."""
    allowed = allowed or ALL_TYPES
    opaque, grey, sd = bool(summary & 1), bool(summary & 2), (summary >> 8) & 0xFF
    out = []
    if opaque and grey and sd in (1, 2, 4, 8):
        out.append((0, sd))
    if analyse_status == 0 and count is not None and trns_len is not None and 1 <= count <= 256 and trns_len <= count:
        out.append((3, next(p for p in (1, 2, 4, 8) if 1 << p >= count)))
    if grey:
        out.append((4, 8))
    if opaque:
        out.append((2, 8))
    out.append((6, 8))
    costed = []
    for colour, depth in out:
        if allowed >> colour & 1:
            cost = r["height"] * row_bytes(r["width"], depth, colour) + prefix_of(colour, count, trns_len) - 41
            costed.append((cost, colour, depth))
    return costed


def plan(r, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    """-> (status, depth, colour, packed, types, prefix, file); depth and colour are the record's unless the status is 0
    and the record was a dimension record; the sizes are 0 unless the status is 0."""
    depth, colour = r["bit_depth"], r["colour_type"]
    fail = lambda st: (st, r["bit_depth"], r["colour_type"], 0, 0, 0, 0)
    if not dimension(r) and not encodable(r):
        return fail(SKIPPED)
    if analyse_status not in (0, TOO_MANY_COLOURS):
        return fail(analyse_status)
    if dimension(r):
        c = candidates(r, count, trns_len, summary, analyse_status, allowed)
        if not c:
            return fail(NOT_REPRESENTABLE)
        _, colour, depth = min(c)            # the smallest cost, then the lower colour type
    elif colour == 3:
        if count is None or trns_len is None or not 1 <= count <= 1 << depth:
            return fail(BAD_PLTE)
        if trns_len > count:
            return fail(BAD_TRNS)
    rb = row_bytes(r["width"], depth, colour)
    if rb >= ROW_LIMIT or r["height"] * (rb + 1) >= FILTERED_LIMIT:
        return fail(BAD_SIZES)
    prefix = prefix_of(colour, count, trns_len)
    return OK, depth, colour, r["height"] * rb, r["height"], prefix, prefix + ultrafast_bound(r["height"] * (rb + 1)) + 16


def write_file(idat, width, height, depth, colour, pal=None, count=0, trns_len=0, crc=fm.crc32):
    """The file around the zlib stream `idat`: for colour type 3 with a PLTE of exactly `count` entries and, where
    trns_len > 0, a tRNS of exactly that many bytes."""
    if colour == 3:
        return pm.write_palette_file(idat, width, height, depth, pal, count, count, trns_len, crc)
    return fm.write_file(idat, width, height, depth, colour, crc)


def encode(rgba, width, height, allowed=0, pair=None, compress=zlib.compress, choose=None, crc=zlib.crc32):
    """One RGBA8 picture (bytes, height * width * 4) to a file -> (status, file or None, depth, colour).  pair: (depth,
    colour) to force, else the plan chooses.  choose(pix [rows, row_bytes], bpp) -> the rows' filter types (by default
    all 0); compress(filtered bytes) -> the zlib stream."""
    rgba = bytes(rgba)
    depth, colour = pair or (0, 0)
    r = mm.record(width, height, depth, colour)
    if len(rgba) != height * width * 4:
        return BAD_SIZES, None, depth, colour
    a_status, pal, count, trns_len, summary = pm.analyse(rgba, width, 256)
    st, depth, colour, packed, _, prefix, _ = plan(r, count, trns_len, summary, a_status, allowed)
    if st != OK:
        if pair and colour == 3 and a_status == TOO_MANY_COLOURS:
            st = TOO_MANY_COLOURS
        return st, None, depth, colour
    pix, st = pm.pack(rgba, width, depth, colour, pal, count or 256)
    if st != OK:
        return st, None, depth, colour
    rb, bpp = fm.geometry(width, depth, colour)
    rows = np.frombuffer(pix, dtype=np.uint8).reshape(height, rb)
    types = choose(rows, bpp) if choose else [0] * height
    idat = compress(png_model.filter_rows(rows, bpp, list(types)).tobytes())
    f = write_file(idat, width, height, depth, colour, pal, count or 0, trns_len or 0, crc)
    assert len(f) == prefix + len(idat) + 16
    return OK, f, depth, colour
