"""Pictures and expected files that the tests of PNG encode at a compression level share (tests/test_png_levels_model.py
on the CPU, tests/test_gpu_png_levels.py on the GPU).  A plain module: no tests, no fixtures.

Every picture has at most about 6 KB of filtered bytes, so that the pure-Python encoders (level_model at levels 1-3,
lazy_model at 4-9) take milliseconds each.  A case is (name, picture, width, height, pair or None, expected status):
the picture a uint8 array of RGBA8 bytes -- for the RGBA16 cases a uint16 array of samples --, the pair forced on it
(None: the plan chooses).
"""
import functools
import zlib

import numpy as np

import lazy_model
import level_model
import oracle_binding as ob
import png16_encode_model as e16
import png_choose_model as cm
import png_encode_mixed_model as em
import png_file_model as fm

LEVELS = (0, 1, 3, 4, 6, 9)
SIZE_LEVELS = (1, 3, 6, 9)          # the size condition's
TILED = "tiled-rgb"                 # the picture of the size condition


def compressor(level):
    """bytes -> the reference's zlib stream at `level`: the oracle's stored writer, level_model, lazy_model."""
    if level == 0:
        return ob.compress_stored
    model = level_model if level <= 3 else lazy_model
    return lambda b: model.compress(b, level)


def choose(rows, bpp):
    return cm.choose(rows, bpp)[0].tolist()


def _tile(patch, width, height):
    """patch: uint32 words [ph, pw] -> the words of a width x height picture that repeats it."""
    ph, pw = patch.shape
    return np.tile(patch, ((height + ph - 1) // ph, (width + pw - 1) // pw))[:height, :width].reshape(-1)


def _bytes(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8).copy()


def cases8():
    """The RGBA8 pictures, in the order of the batch."""
    r = np.random.default_rng(14000)
    rgb = r.integers(0, 1 << 24, (5, 7)).astype(np.uint32) | 0xFF000000
    grey = r.integers(0, 256, (5, 7)).astype(np.uint32) * 0x010101 | 0xFF000000
    few = np.array([0xFF0000FF, 0xFF00FF00, 0x80FF0000, 0xFF123456, 0xFFFFFFFF], dtype=np.uint32)[r.integers(0, 5, (5, 7))]
    noise = r.integers(0, 1 << 32, 20 * 20, dtype=np.uint64).astype(np.uint32)
    bits = np.where(r.integers(0, 2, 33 * 9) == 1, 0xFFFFFFFF, 0xFF000000).astype(np.uint32)
    many = r.integers(0, 1 << 24, 20 * 20).astype(np.uint32) | 0xFF000000
    many[:300] = np.arange(300) * 0x010203 | 0xFF000000              # more than 256 colours for certain
    coloured = np.full(6 * 5, 0xFF808080, dtype=np.uint32)
    coloured[13] = 0xFF010203                                        # grey-8 cannot hold this one
    return [
        (TILED, _bytes(_tile(rgb, 48, 40)), 48, 40, (8, 2), 0),      # 5 800 filtered bytes (35 colours: left alone it is a palette picture)
        ("noise", _bytes(noise), 20, 20, None, 0),
        ("too-many-colours", _bytes(many), 20, 20, (8, 3), 12),
        ("tiled-grey", _bytes(_tile(grey, 96, 40)), 96, 40, None, 0),
        ("zero", np.zeros(16 * 16 * 4, dtype=np.uint8), 16, 16, None, 0),
        ("one-pixel", _bytes(np.array([0x7F112233])), 1, 1, None, 0),
        ("tiled-palette", _bytes(_tile(few, 96, 40)), 96, 40, None, 0),
        ("not-representable", _bytes(coloured), 6, 5, (8, 0), 13),
        ("one-bit", _bytes(bits), 33, 9, None, 0),
        ("tiled-rgb-as-rgba", _bytes(_tile(rgb, 30, 40)), 30, 40, (8, 6), 0),
    ]


def cases16():
    """The RGBA16 pictures: the RGBA8 ones widened (all narrow), and the tiled picture in 16-bit samples."""
    r = np.random.default_rng(14001)
    out = [(name, px.astype(np.uint16) * 257, w, h, pair, st) for name, px, w, h, pair, st in cases8()]
    patch = r.integers(0, 1 << 16, (5, 7, 4)).astype(np.uint16)
    patch[..., 3] = 65535
    patch[0, 0] = (0x1234, 0x5678, 0x9ABC, 65535)
    wide = np.tile(patch, (8, 4, 1))[:40, :24].reshape(-1)           # 24 x 40 as (16, 2): 144-byte rows
    out.insert(3, ("tiled-rgb16", wide, 24, 40, None, 0))
    return out


@functools.lru_cache(maxsize=None)
def expected8(level):
    """[(status, file or None, depth, colour)] of cases8() at `level`, computed once."""
    return [em.encode(px.tobytes(), w, h, pair=pair, compress=compressor(level), choose=choose)
            for _, px, w, h, pair, _ in cases8()]


@functools.lru_cache(maxsize=None)
def expected16(level):
    return [e16.encode16(px.tobytes(), w, h, pair=pair, compress=compressor(level), choose=choose)
            for _, px, w, h, pair, _ in cases16()]


def idat_of(f):
    """The bytes of a file's IDAT chunks."""
    out, at = b"", 8
    while at < len(f):
        size = fm.rd32(f, at)
        if f[at + 4:at + 8] == b"IDAT":
            out += f[at + 8:at + 8 + size]
        at += 12 + size
    return out


def ultrafast_stream_size(filtered):
    return len(ob.compress_ultra_fast(filtered))


def inflate(stream):
    return zlib.decompress(stream)
