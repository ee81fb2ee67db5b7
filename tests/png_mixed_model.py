"""Mixed batches (include/fdeflate_hip.h, "PNG decode: mixed batches") in plain Python integers: what a pipeline that
takes every image's geometry from its own scan record has to allocate, and the records the tests feed to the plan.

    decodable(record)          the record is one the decode steps can work with
    plan(record, max_bytes)    -> (status, comp, filt, pix, rgba): fdh_png_plan_sizes
    record(...)                a scan record as the eight 32-bit words of fdh_png_info
    key(record)                width | depth << 32 | colour << 40 | interlace << 48: what tells a uniform batch
    all_cases()                (record, max_bytes) pairs: every pair and method at small sizes, every kind of record that
                               is not decodable, the boundaries at 2^32, at max_bytes and at 2^31-1 by 2^31-1

A record is a dict with the fields of fdh_png_info (png_file_model.Info carries the same names).  Python integers do
not wrap, so the model is the referee for the sizes near 2^32 and 2^64 as well.
"""
import png_adam7_model as am
import png_file_model as fm

OK, BAD_SIZES, SKIPPED = 0, 2, 3
FIELDS = ("status", "width", "height", "bit_depth", "colour_type", "interlace", "idat_bytes", "idat_chunks", "first_idat", "chunks")


def record(width, height, bit_depth, colour_type, interlace=0, status=0, idat_bytes=0, idat_chunks=1, first_idat=33, chunks=3):
    return dict(status=status, width=width, height=height, bit_depth=bit_depth, colour_type=colour_type, interlace=interlace,
                idat_bytes=idat_bytes, idat_chunks=idat_chunks, first_idat=first_idat, chunks=chunks)


def of_info(info):
    """png_file_model.Info -> record"""
    return {k: int(getattr(info, k)) for k in FIELDS}


def words(r):
    """The record as fdh_png_info's eight 32-bit words."""
    return [r["status"], r["width"], r["height"], r["bit_depth"] | r["colour_type"] << 8 | r["interlace"] << 16, r["idat_bytes"],
            r["idat_chunks"], r["first_idat"], r["chunks"]]


def decodable(r):
    return (r["status"] == 0 and 1 <= r["width"] <= 0x7FFFFFFF and 1 <= r["height"] <= 0x7FFFFFFF
            and (r["bit_depth"], r["colour_type"]) in fm.PAIRS and r["interlace"] <= 1)


def filtered_size(width, height, bit_depth, colour_type, interlace):
    """Bytes the IDAT stream decodes to: every row of every pass with its type byte."""
    bits = fm.CHANNELS[colour_type] * bit_depth
    if interlace == 0:
        return height * (1 + (width * bits + 7) // 8)
    total = 0
    for p in range(7):
        pw = max(0, (width - am.X0[p] + am.DX[p] - 1) // am.DX[p])
        ph = max(0, (height - am.Y0[p] + am.DY[p] - 1) // am.DY[p])
        if pw and ph:
            total += ph * (1 + (pw * bits + 7) // 8)
    return total


def plan(r, max_bytes=0):
    if not decodable(r):
        return SKIPPED, 0, 0, 0, 0
    w, h = r["width"], r["height"]
    bits = fm.CHANNELS[r["colour_type"]] * r["bit_depth"]
    comp = r["idat_bytes"]
    filt = filtered_size(w, h, r["bit_depth"], r["colour_type"], r["interlace"])
    pix = h * ((w * bits + 7) // 8)
    rgba = h * w * 4
    if filt >= 1 << 32 or (max_bytes != 0 and max(comp, filt, pix, rgba) > max_bytes):
        return BAD_SIZES, 0, 0, 0, 0
    return OK, comp, filt, pix, rgba


def key(r):
    return r["width"] | r["bit_depth"] << 32 | r["colour_type"] << 40 | r["interlace"] << 48


SIDES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 33)


def small_records():
    """Every pair, both methods, widths and heights 1 .. 9, 17, 33."""
    out = []
    for d, c in fm.PAIRS:
        for m in (0, 1):
            for w in SIDES:
                for h in SIDES:
                    out.append(record(w, h, d, c, m, idat_bytes=11 + 7 * w * h))
    return out


def undecodable_records():
    """Each scan status, a zero dimension, 2^31, depth 16 with colour type 3, colour type 1, interlace 2."""
    out = [record(5, 4, 8, 2, status=s, idat_bytes=30) for s in range(1, 7)]
    out += [record(0, 4, 8, 2), record(5, 0, 8, 2), record(1 << 31, 4, 8, 2), record(5, 1 << 31, 8, 2), record(0xFFFFFFFF, 1, 1, 0)]
    out += [record(5, 4, 16, 3), record(5, 4, 8, 1), record(5, 4, 3, 0), record(5, 4, 8, 2, interlace=2), record(5, 4, 8, 2, interlace=255)]
    return out


def boundary_records():
    """(record, max_bytes): a filtered size of exactly 2^32 - 1 and 2^32 (65535 * 65537 and 65536 * 65536, grey-8),
    max_bytes at the largest size, one below and one above it with the compressed, the filtered and the RGBA size the
    largest in turn (the packed size never is: the filtered one has the type bytes on top), and 2^31-1 by 2^31-1 at every pair and both methods."""
    out = [(record(65536, 65535, 8, 0, idat_bytes=100), 0), (record(65535, 65536, 8, 0, idat_bytes=100), 0),
           (record(65536, 65535, 8, 0, 1, idat_bytes=100), 0), (record(16385, 65536, 16, 6, 1, idat_bytes=100), 0),
           (record(0x7FFFFFFF, 1, 1, 0, idat_bytes=100), 0), (record(0x7FFFFFFF, 17, 1, 0, 1, idat_bytes=100), 0),
           (record(1, 0x7FFFFFFF, 8, 0, idat_bytes=100), 0), (record(1, 0x7FFFFFFF, 8, 0, 1, idat_bytes=100), 0),
           (record(1, 0x7FFFFFFF, 1, 0, idat_bytes=0xFFFFFFFF), 0)]
    for r in (record(33, 9, 8, 2, idat_bytes=0xFFFFFFFF), record(33, 9, 16, 6, 0, idat_bytes=5), record(33, 9, 16, 6, 1, idat_bytes=5),
              record(33, 9, 1, 0, idat_bytes=5), record(1, 9, 1, 3, 1, idat_bytes=5), record(3, 1, 16, 6, idat_bytes=5)):
        largest = max(plan(r)[1:])
        out += [(r, largest), (r, largest - 1), (r, largest + 1), (r, 1)]
    for d, c in fm.PAIRS:
        for m in (0, 1):
            out += [(record(0x7FFFFFFF, 0x7FFFFFFF, d, c, m, idat_bytes=27), 0), (record(0x7FFFFFFF, 0x7FFFFFFF, d, c, m, idat_bytes=27), 1 << 63)]
    return out


def all_cases():
    """(record, max_bytes) of everything above: what the host function and the device kernel are both checked on."""
    return [(r, 0) for r in small_records() + undecodable_records()] + boundary_records()
