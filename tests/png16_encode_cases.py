"""RGBA16 pictures that the tests of the RGBA16 mixed encode share (tests/test_png16_encode_model.py on the CPU,
tests/test_gpu_png16_encode.py on the GPU).  A plain module: no tests, no fixtures.

A picture is a numpy uint16 array [height * width * 4] in R, G, B, A order; .tobytes() (or .view(np.uint8)) is the
little-endian RGBA16 buffer the library takes.
"""
import io
import zlib

import numpy as np

import png16_encode_model as e16
import png16_model as m16
import png_encode_mixed_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_mixed_model as mm
import png_model
from png_corpus import LEFT_OUT, kinds, palette_image, pillow_rgba

MASKS = [0, 1 << 6, (1 << 3) | (1 << 6), (1 << 0) | (1 << 2), (1 << 4) | (1 << 2) | (1 << 3), 1 << 3]   # `allowed`, as test_gpu_png_encode_mixed.py


def widen(rgba8):
    """The RGBA16 picture whose samples are 257 * the samples of an RGBA8 picture (uint8 array or bytes): all narrow."""
    return np.frombuffer(bytes(rgba8), dtype=np.uint8).astype(np.uint16) * 257


def wide_picture(r, width, height, colour):
    """A random RGBA16 picture that (16, colour) holds and no cheaper pair does: R, G, B (and A where the colour type has
    one) use all 16 bits, the first pixel has samples whose bytes differ, and grey / opaque are exactly what the colour
    type needs."""
    n = width * height
    px = r.integers(0, 1 << 16, (n, 4)).astype(np.uint16)
    px[0] = (0x1234, 0x5678, 0x9ABC, 0x0DEF)
    if colour in (0, 4):
        px[:, 1] = px[:, 0]
        px[:, 2] = px[:, 0]
    if colour in (0, 2):
        px[:, 3] = 65535
    return px.reshape(-1)


def kinds16(r, width, height):
    """Pictures of every kind the RGBA16 plan chooses -> [(name, picture, depth, colour)]: the eleven kinds of
    png_corpus.kinds widened (the plan gives them their RGBA8 pair) and the four pairs of depth 16."""
    out = [(name, widen(px), depth, colour) for name, px, depth, colour in kinds(r, width, height)]
    for colour, name in ((0, "grey16"), (4, "grey-alpha16"), (2, "rgb16"), (6, "rgba16")):
        out.append((name, wide_picture(r, width, height, colour), 16, colour))
    return out


def holds(r, width, height, depth, colour):
    """A random RGBA16 picture that the pair holds without loss -> (picture, pal words or None, count): below depth 16 a
    widened RGBA8 picture (colour type 3: one of up to 2^depth colours, its palette the sorted distinct words)."""
    if depth == 16:
        return wide_picture(r, width, height, colour), None, 256
    if colour == 3:
        colours = int(r.integers(1, (1 << depth) + 1))
        px8 = palette_image(r, width, height, colours, int(r.integers(0, colours + 1)))
        words = sorted(set(px8.view(np.uint32).tolist()))
        return widen(px8), words + [0xFF000000] * (256 - len(words)), len(words)
    return widen(gh.random_rgba(r, width, height, depth, colour).view(np.uint8)), None, 256


PAIRS = fm.PAIRS
NARROW_PAIRS = tuple(p for p in fm.PAIRS if p[0] < 16)


# ---- what the plan is checked on ----

def plan_records():
    """The records of the RGBA8 plan's tests (tests/test_png_encode_mixed_model.py), the size limits included."""
    big = 0x7FFFFFFF
    out = [mm.record(w, h, 0, 0) for w, h in ((1, 1), (2, 2), (3, 5), (8, 12), (16, 16), (341, 64))]
    out += [mm.record(33, 7, d, c) for d, c in fm.PAIRS]
    out += [mm.record(rb, 1, 8, 0) for rb in (em.ROW_LIMIT - 1, em.ROW_LIMIT, em.ROW_LIMIT + 1)]
    out += [mm.record((1 << 16) - 1, h, 8, 0) for h in ((1 << 15) - 1, 1 << 15, (1 << 15) + 1)]
    out += [mm.record(w, 1, 0, 0) for w in ((1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24)]
    out += [mm.record(big, big, 16, 6), mm.record(big, big, 0, 0), mm.record(big, 1, 1, 0), mm.record(1, big, 1, 0), mm.record(1, big, 0, 0)]
    out += [mm.record(0, 4, 8, 6), mm.record(4, 0, 0, 0), mm.record(1 << 31, 4, 8, 6), mm.record(4, 4, 0, 0, interlace=1),
            mm.record(4, 4, 8, 6, status=5), mm.record(4, 4, 0, 0, status=1), mm.record(4, 4, 0, 2), mm.record(4, 4, 16, 3)]
    return out


def plan_inputs():
    """(summary, count, trns_len, analyse_status): every combination of summary bits 0 .. 2 with depths 1 .. 16 and the
    counts 0, 1, 2, 3, 16, 17, 256, and no palette at all."""
    out = []
    for bits in range(8):
        for depth in (1, 2, 4, 8, 16):
            summary = bits | depth << 8
            for count in (0, 1, 2, 3, 16, 17, 256):
                for trns in sorted({0, 1, count}):
                    if trns <= count:
                        out.append((summary, count, trns, 0))
            out.append((summary, None, None, 12))
            out.append((summary, 0, 0, 12))
    return out


# ---- files back to pictures without device code, and in Pillow ----

def host_route(f):
    """A file back to its RGBA16 picture without device code -> (picture bytes, depth, colour)."""
    info = fm.scan(f)
    assert info.status == 0
    depth, colour = info.bit_depth, info.colour_type
    idat = b"".join(f[at + 8:at + 8 + size] for tag, at, size in chunk_list(f) if tag == b"IDAT")
    rb, bpp = fm.geometry(info.width, depth, colour)
    pix = png_model.unfilter(zlib.decompress(idat), rb, bpp)
    pal = None
    if colour == 3:
        plte = next(f[at + 8:at + 8 + size] for tag, at, size in chunk_list(f) if tag == b"PLTE")
        trns = b"".join(f[at + 8:at + 8 + size] for tag, at, size in chunk_list(f) if tag == b"tRNS")
        pal = [(plte[3 * k], plte[3 * k + 1], plte[3 * k + 2], trns[k] if k < len(trns) else 255) for k in range(len(plte) // 3)]
    out, st = m16.expand16(pix, info.width, depth, colour, None, pal)
    assert st == 0
    return out, depth, colour


def chunk_list(f):
    out, at = [], 8
    while at < len(f):
        size = fm.rd32(f, at)
        out.append((f[at + 4:at + 8], at, size))
        at += 12 + size
    return out


def check_in_pillow(f, px, width, height, depth, colour):
    """Pixels for the pairs of depth 8 and below outside LEFT_OUT, grey-16 through I;16, the size for the rest."""
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.size == (width, height)
    if (depth, colour) == (16, 0):
        assert im.mode == "I;16" and np.array_equal(np.asarray(im).astype(np.uint16).reshape(-1), px.reshape(-1, 4)[:, 0])
    elif depth <= 8 and (depth, colour) not in LEFT_OUT:
        assert pillow_rgba(f) == e16.high_bytes(px.tobytes())
