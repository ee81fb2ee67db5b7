"""tests/png16_model.py against what is independent of it: the RGBA8 model (every sample value of depths 1 to 8),
numpy's big-endian view of 16-bit samples, Pillow on 16-bit grey (mode I;16, which it reads and writes exactly; it
reduces 16-bit colour files to eight bits, so it is a referee for grey only), and literal values."""
import io
import zlib

import numpy as np
import pytest

import png16_model as m16
import png_adam7_model as am
import png_expand_model as em
import png_file_model as fm
from png_corpus import random_case, stream_of

Image = pytest.importorskip("PIL.Image")


def u16(rgba16):
    return np.frombuffer(rgba16, dtype="<u2").reshape(-1, 4)


def every_value_case(r, depth, colour):
    """(pix, width, key, pal): rows in which every sample value of the depth occurs in every channel (depths 1 to 8),
    or 300 random pixels with the corner values among them (depth 16)."""
    ch = fm.CHANNELS[colour]
    width = 256 if depth <= 8 else 300
    if depth <= 8:
        v = (np.arange(width)[:, None] + 37 * np.arange(ch)[None, :]) % (1 << depth)          # [width, ch]
        bits = ((v.reshape(-1)[:, None] >> np.arange(depth - 1, -1, -1)[None, :]) & 1).astype(np.uint8).reshape(-1)
        rb = fm.geometry(width, depth, colour)[0]
        row = np.zeros(rb * 8, dtype=np.uint8)
        row[:bits.size] = bits
        pix = np.packbits(row)
        assert em.samples(pix.tobytes(), width, depth, ch) == v.reshape(-1).tolist()
    else:
        v = r.integers(0, 65536, (width, ch))
        v[:4] = np.array([0, 0xFFFF, 0x00FF, 0xFF00])[:, None]
        pix = v.astype(">u2").view(np.uint8).reshape(-1)
    pal = key = None
    if colour == 3:
        n = 1 << depth
        pal = em.palette(r.integers(0, 256, 3 * n, dtype=np.uint8).tobytes(), r.integers(0, 256, n, dtype=np.uint8).tobytes())
    elif colour in (0, 2):
        key = tuple(int(x) for x in v[width // 2])
    return pix, width, key, pal


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_expand16_against_the_rgba8_model(pair):
    """All fifteen pairs, keyed and not: the high bytes of expand16 are expand's bytes, and at depths 1 to 8 -- every
    sample value -- expand16 is expand times 257 (s * 65535 / max = (s * 255 / max) * 257)."""
    depth, colour = pair
    r = np.random.default_rng(16100 + 64 * colour + depth)
    pix, width, key, pal = every_value_case(r, depth, colour)
    for k in (None, key) if key is not None else (None,):
        wide, st16 = m16.expand16(pix, width, depth, colour, k, pal)
        narrow, st8 = em.expand(pix, width, depth, colour, k, pal)
        assert st16 == st8 == 0 and len(wide) == 2 * len(narrow)
        w, n = u16(wide), np.frombuffer(narrow, dtype=np.uint8).reshape(-1, 4).astype(np.uint16)
        assert np.array_equal(w >> 8, n)
        if depth <= 8:
            assert np.array_equal(w, n * 257)
        if k is not None:
            assert 0 in w[:, 3] and 65535 in w[:, 3]
    assert [m16.to16((1 << d) - 1, d) for d in (1, 2, 4, 8, 16)] == [65535] * 5
    assert [m16.to16(1, d) for d in (1, 2, 4, 8, 16)] == [65535, 21845, 4369, 257, 1]


@pytest.mark.parametrize("colour", (0, 2, 4, 6))
def test_depth_16_is_the_samples_themselves(colour):
    r = np.random.default_rng(16200 + colour)
    pix, width, _, _ = every_value_case(r, 16, colour)
    s = np.frombuffer(pix.tobytes(), dtype=">u2").reshape(width, -1)
    w = u16(m16.expand16(pix, width, 16, colour)[0])
    full = np.full(width, 65535)
    columns = {0: (0, 0, 0, None), 2: (0, 1, 2, None), 4: (0, 0, 0, 1), 6: (0, 1, 2, 3)}[colour]     # None: alpha 65535
    assert np.array_equal(w, np.stack([full if c is None else s[:, c] for c in columns], axis=1))


def test_grey_16_against_pillow_both_ways():
    """Model-written grey-16 files as Pillow reads them (mode I;16) are expand16's R plane; files Pillow writes from an
    I;16 image, decoded by the models, are the source."""
    r = np.random.default_rng(16300)
    for width, height in ((1, 1), (7, 5), (33, 9), (100, 3)):
        pix, _, _ = random_case(r, width, height, 16, 0, False)
        png = m16.write_file(stream_of(pix, 2 * width), width, height, 16, 0, crc=zlib.crc32)
        im = Image.open(io.BytesIO(png))
        im.load()
        assert im.mode == "I;16"
        w = u16(m16.expand16(pix, width, 16, 0)[0]).reshape(height, width, 4)
        assert np.array_equal(np.asarray(im).astype(np.uint16), w[..., 0])
        assert np.array_equal(w[..., 0], w[..., 1]) and np.array_equal(w[..., 0], w[..., 2]) and (w[..., 3] == 65535).all()
        source = r.integers(0, 65536, (height, width), dtype=np.uint16)
        b = io.BytesIO()
        Image.fromarray(source).save(b, "PNG")
        fw, fh, d, c, packed = am.decode(b.getvalue())
        assert (fw, fh, d, c) == (width, height, 16, 0)
        got = u16(m16.expand16(bytes(packed), width, 16, 0)[0]).reshape(height, width, 4)
        assert np.array_equal(got[..., 0], source)


def representable(r, n, colour):
    """n random RGBA16 pixels (uint16 [n, 4]) that the pair (16, colour) holds without loss."""
    p = r.integers(0, 65536, (n, 4)).astype(np.uint16)
    corners = (0, 0xFFFF, 0x00FF, 0xFF00, 0x0100)
    p[:min(n, 5), 0] = corners[:min(n, 5)]
    if colour in (0, 4):
        p[:, 1] = p[:, 2] = p[:, 0]
    if colour in (0, 2):
        p[:, 3] = 65535
    return p


@pytest.mark.parametrize("colour", (0, 2, 4, 6))
def test_pack16_there_and_back(colour):
    r = np.random.default_rng(16400 + colour)
    for width, height in ((1, 1), (5, 3), (33, 2)):
        x = representable(r, width * height, colour).astype("<u2").tobytes()
        packed, st = m16.pack16(x, width, colour)
        assert st == 0 and len(packed) == height * fm.geometry(width, 16, colour)[0]
        assert m16.expand16(packed, width, 16, colour) == (x, 0)
    # big-endian on the way out: R = 0x1234 is the bytes 0x12, 0x34
    one = np.array([[0x1234, 0x1234, 0x1234, 0xFFFF]], dtype="<u2").tobytes()
    assert m16.pack16(one, 1, 0) == (bytes([0x12, 0x34]), 0)


def test_every_reason_for_status_13():
    px = lambda r, g, b, a: np.array([[r, g, b, a]], dtype="<u2").tobytes()    # noqa: E731
    grey, opaque = px(7, 7, 7, 65535), px(1, 2, 3, 65535)
    for colour, bad in ((0, px(7, 8, 7, 65535)), (0, px(7, 7, 8, 65535)), (0, px(7, 7, 7, 65534)), (0, px(7, 7, 7, 0x00FF)),
                        (4, px(7, 8, 7, 9)), (4, px(8, 7, 7, 9)), (4, px(0x0107, 0x0007, 0x0107, 9)),
                        (2, px(1, 2, 3, 0)), (2, px(1, 2, 3, 0xFF00))):
        assert m16.pack16(grey + bad + grey, 3, colour)[1] == 13, (colour, bad)
        assert m16.pack16(grey + grey, 2, colour)[1] == 0
    assert m16.pack16(opaque, 1, 2)[1] == 0 and m16.pack16(opaque, 1, 6)[1] == 0 and m16.pack16(opaque, 1, 4)[1] == 13
    assert m16.pack16(px(1, 2, 3, 4), 1, 6) == (bytes([0, 1, 0, 2, 0, 3, 0, 4]), 0)


def test_a_key_that_matches_in_the_high_bytes_only_leaves_the_pixel_opaque():
    # grey: 0x1234 is the key, 0x1235 and 0x1334 are not (the RGBA8 model cannot tell the first two apart in its output)
    rgba, st = m16.expand16(bytes([0x12, 0x34, 0x12, 0x35, 0x13, 0x34]), 3, 16, 0, key=(0x1234,))
    assert st == 0 and u16(rgba).tolist() == [[0x1234] * 3 + [0], [0x1235] * 3 + [65535], [0x1334] * 3 + [65535]]
    key = (0x0102, 0x0304, 0x0506)
    px = [key, (0x0103, 0x0304, 0x0506), (0x0102, 0x0305, 0x0506), (0x0102, 0x0304, 0x0507)]
    rgba, st = m16.expand16(b"".join(em.trns_body(p) for p in px), 4, 16, 2, key=key)
    assert st == 0 and u16(rgba).tolist() == [list(p) + [0 if p == key else 65535] for p in px]
    # a key wider than the depth is masked, as in the RGBA8 model
    assert u16(m16.expand16(bytes([0b00011011]), 4, 2, 0, key=(0xFF02,))[0])[:, 3].tolist() == [65535, 65535, 0, 65535]
    # an index outside the palette: (0, 0, 0, 65535) and status 9
    rgba, st = m16.expand16(bytes([0, 2]), 2, 8, 3, pal=[(1, 2, 3, 4), (5, 6, 7, 255)])
    assert st == 9 and u16(rgba).tolist() == [[257, 514, 771, 1028], [0, 0, 0, 65535]]
