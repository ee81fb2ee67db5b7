"""-m gpu: PNG encode from RGBA8 -- fdh_png_analyse_batch, fdh_png_pack_batch, fdh_png_frame_palette_batch,
png_encode_rgba_files_batch.

Referee: tests/png_pack_model.py (plain integers, pinned to png_expand_model, to Pillow and to literal bytes by
tests/test_png_pack_model.py); the existing fdh_png_expand_batch, fdh_png_scan_files_batch and fdh_png_colour_batch on
the device, and Pillow's reader on the files.  Everything is bit-exact.

png_pack_kernel: grid(n, waves), a wavefront takes the bands b, b + waves, .. of 64 rows of its image and four pixels
per lane and step; FDH_PNG_PACK_WAVES forces the wavefronts per image.  png_analyse_kernel: one workgroup per image,
FDH_PNG_ANALYSE_WAVES (1 .. 16) forces its wavefronts.
"""
import zlib

import numpy as np
import pytest

import png_corpus as pc
import png_expand_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_pack_model as pm
from png_gpu_harness import GUARD, HEIGHTS, PASSED_ON

pytestmark = pytest.mark.gpu

GUARD_WORD = 0x5A5A5A5A


def random_palette(r, depth, duplicates=True):
    """2^depth palette words in no order, with A < 255 anywhere and (from four entries on) some words twice."""
    n = 1 << depth
    pal = r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pal[r.integers(0, n)] |= 0xFF000000
    if duplicates and n >= 4:
        for _ in range(n // 4):
            a, b = r.integers(0, n, 2)
            pal[a] = pal[b]
    return pal


def palette_pixels(r, pal, count, npix):
    """Pixel words drawn from the first `count` entries; every entry occurs where there is room."""
    idx = r.integers(0, count, npix)
    k = min(count, npix)
    idx[r.permutation(npix)[:k]] = np.arange(k)
    return pal[idx]


class Batch:
    """Images one behind the other from an odd byte of a buffer of guard bytes, and their packed slots with a slot of
    guard bytes between every two (an entry with no pixels that `upstream` marks as failed: its slot must stay as it
    is): 20 bytes behind the first image, 5 behind the others, so that packed slots start at every alignment."""

    def __init__(self, images, width, depth, colour, front=3, null_colour=False):
        """images: [(pixel words uint32, palette words or None, count)]"""
        self.geometry = (width, depth, colour)
        self.n = 2 * len(images)
        rb = fm.geometry(width, depth, colour)[0]
        s_off, p_off, self.want_status, self.unspecified = [front], [0], [], []
        for k, (px, pal, count) in enumerate(images):
            want, st = pm.pack(px.view(np.uint8), width, depth, colour, None if pal is None else pal.tolist(), count)
            assert len(want) == px.size // width * rb
            s_off += [s_off[-1] + 4 * px.size] * 2
            p_off += [p_off[-1] + len(want), p_off[-1] + len(want) + (20 if k == 0 else 5)]
            self.want_status += [st, PASSED_ON]
            self.unspecified.append(st != 0)
        self.s_off, self.p_off = np.asarray(s_off, dtype=np.int64), np.asarray(p_off, dtype=np.int64)
        self.rgba = np.full(int(s_off[-1]) + 7, GUARD, dtype=np.uint8)
        self.expect = np.full(int(p_off[-1]) + 64, GUARD, dtype=np.uint8)
        for k, (px, pal, count) in enumerate(images):
            self.rgba[s_off[2 * k]:s_off[2 * k + 1]] = px.view(np.uint8)
            want, _ = pm.pack(px.view(np.uint8), width, depth, colour, None if pal is None else pal.tolist(), count)
            self.expect[p_off[2 * k]:p_off[2 * k + 1]] = np.frombuffer(want, dtype=np.uint8)
        self.upstream = [0, PASSED_ON] * len(images)
        self.pal = self.colour = None
        if colour == 3:
            full = [np.concatenate([pal, np.full(256 - pal.size, 0xFF000000, dtype=np.uint32)]) for _, pal, _ in images]
            self.pal = [w for p in full for w in (p.tolist(), [0] * 256)]
            if not null_colour:
                self.colour = [w for _, _, count in images for w in ([count, 0, 0, 0], [0] * 4)]
        self.images = images

    def run(self, fd):
        """-> (packed buffer on the device, png_status) after one call; the input must not change."""
        import torch
        d_rgba = gh.dev(self.rgba)
        pix = torch.full((self.expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n + 16,), GUARD_WORD, dtype=torch.int32, device="cuda")
        fd.png_pack_batch(d_rgba, gh.dev(self.s_off), pix, gh.dev(self.p_off), *self.geometry,
                          pal=None if self.pal is None else gh.words(self.pal),
                          colour=None if self.colour is None else gh.words(self.colour),
                          upstream=gh.words(self.upstream), png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        assert np.array_equal(d_rgba.cpu().numpy(), self.rgba)
        st = st.cpu().numpy()
        assert (st[:8] == GUARD_WORD).all() and (st[8 + self.n:] == GUARD_WORD).all()
        return pix, st[8:8 + self.n].tolist()

    def check(self, fd, what, round_trip=True):
        import torch
        pix, st = self.run(fd)
        assert st == self.want_status, (what, st)
        got = pix.cpu().numpy()
        expect = self.expect.copy()
        for k, loose in enumerate(self.unspecified):        # status 13: the slot's contents are not specified
            if loose:
                expect[self.p_off[2 * k]:self.p_off[2 * k + 1]] = got[self.p_off[2 * k]:self.p_off[2 * k + 1]]
        if not np.array_equal(got, expect):
            at = int(np.nonzero(got != expect)[0][0])
            raise AssertionError("%r: byte %d of the output is %d, not %d (slots at %s)" % (what, at, got[at], expect[at], self.p_off.tolist()))
        if round_trip:      # the existing expansion on the device gives the input back
            sizes = np.diff(self.s_off)
            b_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            back = torch.full((int(b_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
            est = fd.png_expand_batch(pix, gh.dev(self.p_off), back, gh.dev(b_off), *self.geometry,
                                      pal=None if self.pal is None else gh.words(self.pal),
                                      colour=None if self.colour is None else gh.words(self.colour),
                                      upstream=gh.words(st))
            torch.cuda.synchronize()
            assert est.cpu().tolist() == st, what
            back = back.cpu().numpy()
            for k, (px, _, _) in enumerate(self.images):
                if st[2 * k] == 0:
                    assert np.array_equal(back[b_off[2 * k]:b_off[2 * k + 1]], px.view(np.uint8)), (what, k)


# ---- fdh_png_pack_batch ----

@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_pack_every_width_and_height(pair, monkeypatch):
    """Every width of gh.PACK_WIDTHS at heights 1, 2, 3 and one more than a band, four images a call: the packed buffer equals
    the model's byte for byte (padding bits zero), guard slots and the bytes behind the last slot included, the input is
    unchanged, every status is right, and fdh_png_expand_batch takes the packed rows back to the input on the device.
    Palettes are unsorted and hold duplicates.  Each batch runs with 1, 2 and 5 wavefronts per image and the default."""
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(9500 + 64 * colour + depth)
    for width in gh.PACK_WIDTHS:
        images = []
        for h in HEIGHTS:
            if colour == 3:
                pal = random_palette(r, depth)
                images.append((palette_pixels(r, pal, pal.size, width * h), pal, pal.size))
            else:
                images.append((gh.random_rgba(r, width, h, depth, colour), None, 256))
        b = Batch(images, width, depth, colour)
        assert b.want_status[0::2] == [0] * len(images)
        for waves in (1, 2, 5, None):
            gh.set_env(monkeypatch, FDH_PNG_PACK_WAVES=waves)
            b.check(fd, (pair, width, waves), round_trip=waves in (2, None))


def _spoil(px, at, word):
    out = px.copy()
    out[at] = word
    return out


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_not_representable_wherever_it_sits(pair):
    """Every reason the pair has for status 13, each in the first pixel, in a row's last short quad, in the last short
    quad of the image and in the very last pixel, one image per case between images that fit: 13 exactly there, the
    neighbours exact."""
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(9600 + 64 * colour + depth)
    width, height = 7, 2
    npix = width * height
    reasons = []                                    # (what, a word that cannot be held)
    if colour == 3:
        n = min(1 << depth, 254)
        pal = random_palette(r, depth, duplicates=False)[:n]
        pal = np.concatenate([pal, np.array([0x01020304, 0x05060708], dtype=np.uint32)])      # entries n (inside the count: 2^depth below depth 8) and n + 1 (behind it)
        count = n + 1
        missing = 0x0A0B0C0D
        assert missing not in pal.tolist()
        reasons = [("a colour missing from the palette", missing), ("a colour behind the count", 0x05060708)]
        if depth < 8:
            reasons.append(("an index of 2^depth", 0x01020304))
        base = lambda: (palette_pixels(r, pal[:n], n, npix), pal, count)
    else:
        pal, count = None, 256
        if colour in (0, 2):
            reasons.append(("a translucent pixel", 0xFE000000))
        if colour in (0, 4):
            reasons += [("R != G", 0xFF000011), ("G != B", 0xFF110000)]
        if colour == 0 and depth < 8:
            reasons.append(("not a multiple of the unit", {4: 0xFF808080, 2: 0xFF111111, 1: 0xFF555555}[depth]))
        base = lambda: (gh.random_rgba(r, width, height, depth, colour), None, 256)
    if not reasons:
        assert colour == 6                          # (RGBA holds everything)
        return
    images, want = [base()], [0]
    for what, word in reasons:
        for at in (0, 5, npix - 2, npix - 1):
            px, _, _ = base()
            images += [(_spoil(px, at, word), pal, count), base()]
            want += [13, 0]
    b = Batch(images, width, depth, colour)
    assert b.want_status[0::2] == want, pair
    b.check(fd, pair)


def test_palette_without_colour_words_and_the_lowest_index():
    """colour == NULL: all 256 words count.  A palette of 256 words in which every word occurs twice: the index is the
    lower one, and an image that uses words from the upper half alone still gets the lower indices."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9700)
    half = r.integers(0, 1 << 32, 128, dtype=np.uint64).astype(np.uint32)
    pal = np.concatenate([half, half[::-1]])
    width, height = 33, 5
    px = pal[r.integers(128, 256, width * height)]
    b = Batch([(px, pal, 256), (pal[r.integers(0, 256, width * height)], pal, 256)], width, 8, 3, null_colour=True)
    pix, st = b.run(fd)
    assert st == b.want_status == [0, PASSED_ON, 0, PASSED_ON]
    got = pix.cpu().numpy()
    assert np.array_equal(got, b.expect) and got[:width * height].max() < 128
    b.check(fd, "null colour")
    # with a count of 128 the same pixels are inside; with 100 some are not
    for count, want in ((128, 0), (100, 13)):
        c = Batch([(px, pal, count)], width, 8, 3)
        assert c.want_status[0] == want
        c.check(fd, count)


def test_pack_slots_that_do_not_fit_and_upstream():
    """An RGBA slot of rows and a half, a packed slot one byte short and one long: status 2 and no byte changes.
    upstream != 0: that value is the status and the slot is untouched.  Two empty slots: status 0.  The images in
    between are exact."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(9800)
    for (depth, colour), width in (((8, 2), 21), ((1, 0), 21), ((8, 3), 70), ((16, 6), 9), ((4, 3), 5)):
        rb = fm.geometry(width, depth, colour)[0]
        rows = 4
        full, out = rows * width * 4, rows * rb
        pal = random_palette(r, depth) if colour == 3 else None
        # (RGBA bytes, packed bytes, upstream, expected status)
        plan = [(full, out, 0, 0), (full + width * 2, out + rb, 0, 2), (full, out, 0, 0), (full, out - 1, 0, 2), (full, out + 1, 0, 2),
                (0, 0, 0, 0), (full, out, 5, 5), (full, out, 0, 0), (full, out, 0x80000003, 0x80000003), (0, 3, 0, 2),
                (width * 4, 0, 0, 2), (full, out, 0, 0)]
        s_off = np.concatenate([[1], 1 + np.cumsum([p[0] for p in plan])]).astype(np.int64)
        p_off = np.concatenate([[3], 3 + np.cumsum([p[1] for p in plan])]).astype(np.int64)
        rgba = np.full(int(s_off[-1]) + 3, GUARD, dtype=np.uint8)
        expect = np.full(int(p_off[-1]) + 32, GUARD, dtype=np.uint8)
        for k, (sb, pb, up, want) in enumerate(plan):
            px = palette_pixels(r, pal, pal.size, sb // 4) if colour == 3 else gh.random_rgba(r, sb // 4, 1, depth, colour)
            rgba[s_off[k]:s_off[k] + 4 * px.size] = px.view(np.uint8)
            if want == 0 and sb:
                packed, st = pm.pack(px.view(np.uint8), width, depth, colour, None if pal is None else pal.tolist(), 1 << depth)
                assert st == 0
                expect[p_off[k]:p_off[k + 1]] = np.frombuffer(packed, dtype=np.uint8)
        n = len(plan)
        pix = torch.full((expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        pal_words = None if pal is None else gh.words([np.concatenate([pal, np.zeros(256 - pal.size, dtype=np.uint32)]).tolist()] * n)
        st = fd.png_pack_batch(gh.dev(rgba), gh.dev(s_off), pix, gh.dev(p_off), width, depth, colour, pal=pal_words,
                               colour=None if pal is None else gh.words([[pal.size, 0, 0, 0]] * n), upstream=gh.words([p[2] for p in plan]))
        torch.cuda.synchronize()
        assert st.cpu().numpy().view(np.uint32).tolist() == [p[3] for p in plan], (depth, colour)
        assert np.array_equal(pix.cpu().numpy(), expect), (depth, colour)


def test_pack_more_images_than_wavefronts_fill():
    """5000 images of 3 x 7 two-bit palette pixels, of 2 x 5 sixteen-bit grey + alpha pixels and of 5 x 3 one-bit grey
    pixels in one call each (one wavefront per image; rows of a few pixels share a step), against the model."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(9900)
    n = 5000
    for (depth, colour), width, rows in (((2, 3), 7, 3), ((16, 4), 5, 2), ((1, 0), 3, 5)):
        rb = fm.geometry(width, depth, colour)[0]
        pal = random_palette(r, depth, duplicates=False) if colour == 3 else None
        px = palette_pixels(r, pal, pal.size, n * rows * width) if colour == 3 else gh.random_rgba(r, width, n * rows, depth, colour)
        want, st = pm.pack(px.view(np.uint8), width, depth, colour, None if pal is None else pal.tolist(), 4)     # (the images one below the other)
        assert st == 0
        s_off = 1 + np.arange(n + 1, dtype=np.int64) * (rows * width * 4)
        p_off = np.arange(n + 1, dtype=np.int64) * (rows * rb)
        rgba = np.concatenate([[GUARD], px.view(np.uint8)]).astype(np.uint8)
        pix = torch.full((int(p_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
        got_st = fd.png_pack_batch(gh.dev(rgba), gh.dev(s_off), pix, gh.dev(p_off), width, depth, colour,
                                   pal=None if pal is None else gh.words([np.concatenate([pal, np.zeros(252, dtype=np.uint32)]).tolist()] * n),
                                   colour=None if pal is None else gh.words([[4, 0, 0, 0]] * n))
        torch.cuda.synchronize()
        got = pix.cpu().numpy()
        assert int(got_st.abs().sum()) == 0
        assert got[:int(p_off[-1])].tobytes() == want and (got[int(p_off[-1]):] == GUARD).all()


# ---- fdh_png_analyse_batch ----

def _analyse(fd, images, width, max_colours, with_pal=True, front=5):
    """One call over `images` (uint32 pixel words each; a byte count instead gives a slot of that many guard bytes):
    -> per image (status, pal, count, trns_len, summary) as the model returns them, after the guard words around every
    output array and the input have been checked.  Outputs the call must not have written read as GUARD_WORD."""
    import torch
    sizes = [4 * im.size if isinstance(im, np.ndarray) else im for im in images]
    off = np.concatenate([[front], front + np.cumsum(sizes)]).astype(np.int64)
    rgba = np.full(int(off[-1]) + 9, GUARD, dtype=np.uint8)
    for k, im in enumerate(images):
        if isinstance(im, np.ndarray):
            rgba[off[k]:off[k + 1]] = im.view(np.uint8)
    n = len(images)
    d_rgba = gh.dev(rgba)
    pal = torch.full((n + 2, 256), GUARD_WORD, dtype=torch.int32, device="cuda")
    col = torch.full((n + 2, 4), GUARD_WORD, dtype=torch.int32, device="cuda")
    trns, summ, st = (torch.full((n + 2,), GUARD_WORD, dtype=torch.int32, device="cuda") for _ in range(3))
    fd.png_analyse_batch(d_rgba, gh.dev(off), width, max_colours, with_pal=with_pal, pal=pal[1:n + 1] if with_pal else None,
                         colour=col[1:n + 1], trns_len=trns[1:n + 1], summary=summ[1:n + 1], png_status=st[1:n + 1])
    torch.cuda.synchronize()
    assert np.array_equal(d_rgba.cpu().numpy(), rgba)
    pal, col, trns, summ, st = (t.cpu().numpy().view(np.uint32) for t in (pal, col, trns, summ, st))
    for t in (pal, col, trns, summ, st):
        assert (t[0] == GUARD_WORD).all() and (t[n + 1] == GUARD_WORD).all()
    if not with_pal:
        assert (pal == GUARD_WORD).all()
    return [(int(st[k]), pal[k].tolist(), col[k].tolist(), int(trns[k]), int(summ[k])) for k in range(1, n + 1)], rgba, off


def _check_analysis(got, rgba, off, width, max_colours, what, with_pal=True):
    for k, (st, pal, col, trns, summ) in enumerate(got):
        m_st, m_pal, m_count, m_trns, m_summ = pm.analyse(rgba[off[k]:off[k + 1]], width, max_colours)
        assert st == m_st, (what, k, st, m_st)
        if m_st == 2:           # nothing is written for the image
            assert pal == [GUARD_WORD] * 256 and col == [GUARD_WORD] * 4 and trns == GUARD_WORD and summ == GUARD_WORD, (what, k)
            continue
        assert summ == m_summ, (what, k, hex(summ), hex(m_summ))
        if m_st == 0:
            assert col == [m_count, 0, 0, 0] and trns == m_trns, (what, k, col, trns)
            if with_pal:
                assert pal == m_pal, (what, k)


COUNTS = (1, 2, 3, 16, 17, 255, 256, 257)


def _counted_images(r, width, height):
    """For every count of COUNTS three images of exactly that many distinct pixels: the colours spread at random, and
    one colour only in the very last pixel, and only in the very first."""
    npix = width * height
    images = []
    for c in COUNTS:
        spread = pc.palette_image(r, width, height, c, c // 3).view(np.uint32)
        assert len(set(spread.tolist())) == c
        images.append(spread)
        for at in (npix - 1, 0):
            extra = 0x80123456 if at else 0xFF654321
            if c == 1:
                im = np.full(npix, extra, dtype=np.uint32)
            else:       # the other c - 1 colours on the other pixels
                rest = pc.palette_image(r, npix - 1, 1, c - 1, c // 3).view(np.uint32)
                assert extra not in rest.tolist()
                im = np.insert(rest, at, extra)
            assert len(set(im.tolist())) == c
            images.append(im)
    return images


def test_analyse_counts_against_every_threshold(monkeypatch):
    """Images of 1, 2, 3, 16, 17, 255, 256 and 257 distinct colours (with the alpha mix that decides trns_len), the
    extra colour spread, only in the last pixel and only in the first, under max_colours at, under and over each count:
    status, sorted palette, count, trns_len and summary are the model's, at 1, 4 and 16 wavefronts and the default."""
    import fdeflate_amd as fd
    r = np.random.default_rng(10100)
    width, height = 23, 13
    images = _counted_images(r, width, height)
    limits = sorted({m for c in COUNTS for m in (c - 1, c, c + 1) if 1 <= m <= 256})
    assert limits == [1, 2, 3, 4, 15, 16, 17, 18, 254, 255, 256]
    seen = set()
    for max_colours in limits:
        for waves in (1, 4, 16, None) if max_colours in (1, 16, 256) else (None,):
            gh.set_env(monkeypatch, FDH_PNG_ANALYSE_WAVES=waves)
            got, rgba, off = _analyse(fd, images, width, max_colours)
            _check_analysis(got, rgba, off, width, max_colours, (max_colours, waves))
            seen |= {g[0] for g in got}
    assert seen == {0, 12}


def test_analyse_large_images_at_every_launch_shape(monkeypatch):
    """Three images of 301 x 299 pixels (more quads than a workgroup has lanes: every lane loops) of 200, 256 and 300
    colours in long runs and in noise, from an odd address: the same, exact answer at 1, 2, 4, 7 and 16 wavefronts."""
    import fdeflate_amd as fd
    r = np.random.default_rng(10200)
    width, height = 301, 299
    images = []
    for colours in (200, 256, 300):
        im = pc.palette_image(r, width, height, colours, 50).view(np.uint32)
        runs = np.repeat(im[:width * height // 8 + 1], 8)[:width * height]          # runs of eight equal pixels
        runs[-colours:] = np.unique(im)[:colours]                                 # (and every colour at the end)
        images += [im, runs.copy()]
    answers = []
    for waves in (1, 2, 4, 7, 16, None):
        gh.set_env(monkeypatch, FDH_PNG_ANALYSE_WAVES=waves)
        got, rgba, off = _analyse(fd, images, width, 256, front=1)
        _check_analysis(got, rgba, off, width, 256, waves)
        assert [g[0] for g in got] == [0, 0, 0, 0, 12, 12]
        answers.append([g for g in got if g[0] == 0])
    assert all(a == answers[0] for a in answers)


def test_analyse_colours_in_one_bucket():
    """Colours built to start probing at ONE slot of the kernel's table (the binding names the hash), at the table's
    last slot too, so that the probes wrap: 1 .. 256 of them, and one more than max_colours."""
    import fdeflate_amd as fd
    mul, bits = fd.PNG_ANALYSE_HASH_MUL, fd.PNG_ANALYSE_HASH_BITS
    inv = pow(mul, -1, 1 << 32)
    r = np.random.default_rng(10300)
    width = 16
    images = []
    for bucket in (0, 1000, (1 << bits) - 1):
        words = np.array([((bucket << (32 - bits)) + 7919 * j + 1) * inv % (1 << 32) for j in range(256)], dtype=np.uint32)
        assert {(int(w) * mul % (1 << 32)) >> (32 - bits) for w in words} == {bucket} and len(set(words.tolist())) == 256
        for colours in (2, 40, 256):
            images.append(words[:colours][r.integers(0, colours, width * 32)])
            images[-1][r.permutation(width * 32)[:colours]] = words[:colours]
    for max_colours in (256, 39):
        got, rgba, off = _analyse(fd, images, width, max_colours)
        _check_analysis(got, rgba, off, width, max_colours, max_colours)
        assert [g[0] for g in got] == [0, 0 if max_colours == 256 else 12, 0 if max_colours == 256 else 12] * 3


def test_analyse_summary_bits_switched_by_one_pixel():
    """An all-white image is opaque, grey and of depth 1; ONE pixel -- the first, one in the middle, the last -- switches
    each bit and each depth, through each of R, G and B."""
    import fdeflate_amd as fd
    width, height = 19, 11
    npix = width * height
    white = np.full(npix, 0xFFFFFFFF, dtype=np.uint32)
    OP, GR = pm.OPAQUE, pm.GREY
    cases = [(0xFFFFFFFF, OP | GR | 1 << 8), (0xFF000000, OP | GR | 1 << 8), (0xFEFFFFFF, GR | 1 << 8), (0x00FFFFFF, GR | 1 << 8),
             (0xFF0000FF, OP | 1 << 8), (0xFFFF00FF, OP | 1 << 8), (0xFF555555, OP | GR | 2 << 8), (0xFFAAAAAA, OP | GR | 2 << 8),
             (0xFF111111, OP | GR | 4 << 8), (0xFF101010, OP | GR | 8 << 8), (0xFF0000AA, OP | 2 << 8), (0xFF00AA00, OP | 2 << 8),
             (0xFFAA0000, OP | 2 << 8), (0xFF000022, OP | 4 << 8), (0xFF002200, OP | 4 << 8), (0xFF220000, OP | 4 << 8),
             (0xFF000001, OP | 8 << 8), (0xFF008000, OP | 8 << 8), (0xFF7F0000, OP | 8 << 8), (0x7F7F7F7F, GR | 8 << 8), (0x00010203, 8 << 8)]
    images, want = [], []
    for word, summary in cases:
        for at in (0, npix // 2, npix - 1):
            images.append(_spoil(white, at, word))
            want.append(summary)
    got, rgba, off = _analyse(fd, images, width, 256)
    assert [g[4] for g in got] == want
    _check_analysis(got, rgba, off, width, 256, "summary")
    # the summary is over the whole image also when the colours overflow
    got, rgba, off = _analyse(fd, images, width, 1)
    assert [g[4] for g in got] == want and [g[0] for g in got] == [0] * 3 + [12] * (len(images) - 3)


def test_analyse_without_palette_empty_images_and_bad_slots():
    """pal == NULL: the other outputs alone.  An image of no rows: status 0, no colours, opaque, grey, depth 1, a palette
    of 0xFF000000.  A slot that is not whole rows: status 2 and nothing written for that image."""
    import fdeflate_amd as fd
    r = np.random.default_rng(10400)
    width = 9
    images = [pc.palette_image(r, width, 4, 20, 5).view(np.uint32), 0, pc.palette_image(r, width, 3, 7, 7).view(np.uint32), 4 * width + 4,
              pc.palette_image(r, width, 1, 9, 0).view(np.uint32), 2, 0, pc.palette_image(r, width, 70, 256, 100).view(np.uint32)]
    for with_pal in (True, False):
        got, rgba, off = _analyse(fd, images, width, 256, with_pal=with_pal)
        _check_analysis(got, rgba, off, width, 256, with_pal, with_pal=with_pal)
        assert [g[0] for g in got] == [0, 0, 0, 2, 0, 2, 0, 0]
        assert got[1][2:] == ([0, 0, 0, 0], 0, pm.OPAQUE | pm.GREY | 1 << 8)
        if with_pal:
            assert got[1][1] == [0xFF000000] * 256 and got[2][3] == 7 and got[4][3] == 0


# ---- fdh_png_frame_palette_batch ----

FRAMES = ((1, 0, 1), (2, 2, 1), (16, 5, 4), (256, 0, 8), (256, 256, 8))          # (E, T, depth)


@pytest.mark.parametrize("shape", FRAMES, ids=["E%d-T%d" % s[:2] for s in FRAMES])
def test_frame_palette_files(shape):
    """Files with a PLTE of E entries and a tRNS of T bytes around streams that are already in place, of images with 1 ..
    E colours: byte-equal to write_palette_file; accepted by fdh_png_scan_files_batch (every CRC verified) and read back
    by fdh_png_colour_batch word for word; opened by Pillow as the image.  Every status (2 three ways, 10 two ways, 11)
    leaves its slot as it was with file_len 0, and no byte outside the files is written."""
    import torch
    import fdeflate_amd as fd
    entries, alphas, depth = shape
    r = np.random.default_rng(10500 + entries + alphas)
    width = 13
    rb = fm.geometry(width, depth, 3)[0]
    prefix = fd.png_palette_file_prefix(entries, alphas)
    assert prefix == pm.palette_file_prefix(entries, alphas)
    # (height, colours, translucent ones, what is wrong)
    plan = [(3, 1, min(1, alphas), None), (9, entries, alphas, None), (1, max(1, entries // 2), alphas // 2, None), (5, entries, 0, None),
            (4, 1, 0, "idat_len 0"), (4, 1, 0, "slot too small"), (4, 1, 0, "height 0"), (4, 1, 0, "count 0"), (4, 1, 0, "count above E"),
            (4, 1, 0, "trns_len above T"), (70, entries, alphas, None)]
    files, rows = [], []
    for height, colours, translucent, wrong in plan:
        x = pc.palette_image(r, width, height, colours, translucent)
        st, pal, count, trns_len, _ = pm.analyse(x, width, 256)
        pix, pst = pm.pack(x, width, depth, 3, pal, count)
        assert st == 0 and pst == 0 and count <= entries and trns_len <= alphas
        stream = pc.stream_of(pix, rb)
        idat_len, h, slot = len(stream), height, prefix + len(stream) + 16 + 3
        if wrong == "idat_len 0":
            idat_len = 0
        elif wrong == "slot too small":
            slot = prefix + len(stream) + 15
        elif wrong == "height 0":
            h = 0
        elif wrong == "count 0":
            count = 0
        elif wrong == "count above E":
            count = entries + 1
        elif wrong == "trns_len above T":
            trns_len = alphas + 1
        rows.append((x, stream, pal, count, trns_len, idat_len, h, slot))
        files.append(pm.write_palette_file(stream, width, height, depth, pal, count, entries, alphas, zlib.crc32) if wrong is None else None)
    n = len(plan)
    f_off = np.concatenate([[7], 7 + np.cumsum([row[7] for row in rows])]).astype(np.int64)
    host = np.full(int(f_off[-1]) + 32, GUARD, dtype=np.uint8)
    for k, row in enumerate(rows):
        room = min(len(row[1]), int(f_off[k + 1] - f_off[k]) - prefix)
        host[f_off[k] + prefix:f_off[k] + prefix + room] = np.frombuffer(row[1][:room], dtype=np.uint8)
    expect = host.copy()
    want_st, want_len = [], []
    for k, (row, f) in enumerate(zip(rows, files)):
        st = pm.frame_palette_status(row[5], row[6], row[7], row[3], row[4], entries, alphas)
        assert (st == 0) == (f is not None)
        want_st.append(st)
        want_len.append(len(f) if f else 0)
        if f:
            expect[f_off[k]:f_off[k] + len(f)] = np.frombuffer(f, dtype=np.uint8)
    assert sorted(set(want_st)) == [0, 2, 10, 11] and want_st.count(2) == 3 and want_st.count(10) == 2
    d_file = gh.dev(host)
    d_off = gh.dev(f_off)
    pal_words = gh.words([row[2] for row in rows])
    f_len = torch.full((n + 2,), GUARD_WORD, dtype=torch.int32, device="cuda")
    st = torch.full((n + 2,), GUARD_WORD, dtype=torch.int32, device="cuda")
    fd.png_frame_palette_batch(d_file, d_off, gh.words([row[5] for row in rows]), gh.words([row[6] for row in rows]), pal_words,
                               gh.words([[row[3], 0, 0, 0] for row in rows]), gh.words([row[4] for row in rows]), width, depth, entries,
                               alphas, file_len=f_len[1:n + 1], png_status=st[1:n + 1])
    torch.cuda.synchronize()
    got = d_file.cpu().numpy()
    f_len_h, st_h = f_len.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)
    assert st_h.tolist() == [GUARD_WORD] + want_st + [GUARD_WORD] and f_len_h.tolist() == [GUARD_WORD] + want_len + [GUARD_WORD]
    for k in range(n):          # (the bytes of a slot behind its file are not specified)
        if want_len[k]:
            got[f_off[k] + want_len[k]:f_off[k + 1]] = expect[f_off[k] + want_len[k]:f_off[k + 1]]
    if not np.array_equal(got, expect):
        at = int(np.nonzero(got != expect)[0][0])
        raise AssertionError("byte %d is %d, not %d (slots at %s)" % (at, got[at], expect[at], f_off.tolist()))
    # the device's own readers, and Pillow
    info = fd.png_scan_files_batch(d_file, d_off, f_len[1:n + 1])
    pal_back, colour_back, cst = fd.png_colour_batch(d_file, d_off, info, width, depth, 3)
    torch.cuda.synchronize()
    fields = fd.png_info_fields(info)
    pal_back, colour_back = pal_back.cpu().numpy().view(np.uint32), colour_back.cpu().numpy().view(np.uint32)
    for k, (row, f) in enumerate(zip(rows, files)):
        if f is None:
            assert fields["status"][k] != 0
            continue
        assert fields["status"][k] == 0 and cst[k].item() == 0, k
        assert (fields["width"][k], fields["height"][k], fields["bit_depth"][k], fields["colour_type"][k]) == (width, plan[k][0], depth, 3)
        assert fields["first_idat"][k] == prefix - 8 and fields["chunks"][k] == (5 if alphas else 4)
        model_pal = em.read_colour(f, fm.scan(f, crc=zlib.crc32), width, depth, 3)[1]
        assert colour_back[k].tolist() == [entries, 0, 0, 0] and pal_back[k].tolist() == em.pal_words(model_pal)
        assert pal_back[k].tolist()[:row[3]] == row[2][:row[3]]
        assert pc.pillow_rgba(got[f_off[k]:f_off[k] + want_len[k]].tobytes()) == row[0].tobytes(), k


def test_frame_palette_invalid_arguments():
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd._lib import FdeflateHipError
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    pal = torch.zeros(256, dtype=torch.int32, device="cuda")
    f = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    off = gh.dev(np.array([0, 4096], dtype=np.int64))
    for width, depth, e, t in ((0, 8, 4, 0), (5, 16, 4, 0), (5, 8, 0, 0), (5, 8, 257, 0), (5, 2, 5, 0), (5, 4, 16, 17)):
        with pytest.raises(FdeflateHipError):
            fd.png_frame_palette_batch(f, off, z[:1], z[:1], pal, z[:4], z[:1], width, depth, e, t)
    with pytest.raises(FdeflateHipError):
        fd.png_analyse_batch(f, off, 5, max_colours=257)
    with pytest.raises(FdeflateHipError):
        fd.png_analyse_batch(f, off, 5, max_colours=0)
    with pytest.raises(FdeflateHipError):
        fd.png_pack_batch(f, off, f, off, 5, 8, 3)          # colour type 3 needs a palette
    with pytest.raises(ValueError):
        fd.png_palette_file_prefix(4, 5)
    torch.cuda.synchronize()
    assert int(f.sum()) == 0


# ---- RGBA -> files -> RGBA ----

@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_rgba_to_files_and_back(pair):
    """png_encode_rgba_files_batch, then png_decode_files_rgba_batch: the pictures come back byte for byte, for every
    pair, at heights 1, 5 and 70; the files open in Pillow to the same RGBA; no byte outside the file slots changes."""
    import torch
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(10700 + 64 * colour + depth)
    width, heights = 37, (1, 5, 70)
    if colour == 3:
        images = [pc.palette_image(r, width, h, 1 << depth, (1 << depth) // 2).view(np.uint32) for h in heights]
    else:
        images = [gh.random_rgba(r, width, h, depth, colour) for h in heights]
    rgba = np.concatenate([[GUARD]] + [im.view(np.uint8) for im in images]).astype(np.uint8)
    r_off = np.concatenate([[1], 1 + np.cumsum([4 * im.size for im in images])]).astype(np.int64)
    extra = fd.png_palette_file_prefix(1 << depth, 1 << depth) - 41 if colour == 3 else 0
    f_off = gh.file_slots(fd, heights, width, depth, colour, extra)
    file = torch.full((int(f_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    d_rgba = gh.dev(rgba)
    file_len, st = fd.png_encode_rgba_files_batch(d_rgba, gh.dev(r_off), file, gh.dev(f_off), width, depth, colour)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, 0], pair
    assert np.array_equal(d_rgba.cpu().numpy(), rgba)
    host = file.cpu().numpy()
    assert (host[:3] == GUARD).all() and (host[int(f_off[-1]):] == GUARD).all()
    lens = file_len.cpu().tolist()
    for k, im in enumerate(images):
        png = host[f_off[k]:f_off[k] + lens[k]].tobytes()
        info = fm.scan(png, crc=zlib.crc32)
        assert (info.status, info.width, info.height, info.bit_depth, info.colour_type) == (0, width, heights[k], depth, colour), (pair, k)
        assert pc.pillow_rgba(png) == im.view(np.uint8).tobytes(), (pair, k)
    back, back_off, info, status, png_status = fd.png_decode_files_rgba_batch(file, gh.dev(f_off), width, depth, colour, file_len=file_len)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0] and png_status.cpu().tolist() == [0, 0, 0]
    assert back_off.cpu().tolist() == (r_off - 1).tolist()
    assert np.array_equal(back.cpu().numpy(), rgba[1:]), pair


def test_one_batch_of_images_that_fit_and_images_that_do_not():
    """Palette files of at most 16 colours with a tRNS of at most four entries: images that fit between one of 17 colours
    (12), one whose slot is rows and a half (2), one with five translucent colours (11) and one whose file slot is too
    small (the encoder's status); grey files between a coloured image and a translucent one (13).  Each image gets its
    own status, a failed image no file, and the others open in Pillow."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(10800)
    width, height = 29, 6
    good = lambda colours, clear: pc.palette_image(r, width, height, colours, clear).view(np.uint32)
    images = [good(16, 4), good(17, 0), good(3, 3), good(16, 4)[:width * height - width // 2], good(1, 0), good(9, 5), good(16, 0), good(2, 1)]
    want = [0, 12, 0, 2, 0, 11, None, 0]
    r_off = np.concatenate([[0], np.cumsum([4 * im.size for im in images])]).astype(np.int64)
    rgba = np.concatenate([im.view(np.uint8) for im in images])
    prefix = fd.png_palette_file_prefix(16, 4)
    sizes = [fd.png_file_bound(height, fm.geometry(width, 4, 3)[0]) + prefix - 41] * len(images)
    sizes[6] = prefix + 16 + 8                      # no stream fits
    f_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    file = torch.full((int(f_off[-1]),), GUARD, dtype=torch.uint8, device="cuda")
    file_len, st = fd.png_encode_rgba_files_batch(gh.dev(rgba), gh.dev(r_off), file, gh.dev(f_off), width, 4, 3, plte_entries=16, trns_entries=4)
    torch.cuda.synchronize()
    st, lens, host = st.cpu().tolist(), file_len.cpu().tolist(), file.cpu().numpy()
    assert st[6] != 0 and [s for k, s in enumerate(st) if k != 6] == [w for w in want if w is not None], st
    for k, w in enumerate(want):
        if w == 0:
            png = host[f_off[k]:f_off[k] + lens[k]].tobytes()
            assert fm.scan(png, crc=zlib.crc32).status == 0 and pc.pillow_rgba(png) == images[k].view(np.uint8).tobytes(), k
        else:
            assert lens[k] == 0, k
    # grey
    images = [gh.random_rgba(r, width, height, 8, 0), _spoil(gh.random_rgba(r, width, height, 8, 0), 77, 0xFF010000),
              gh.random_rgba(r, width, height, 8, 0), _spoil(gh.random_rgba(r, width, height, 8, 0), width * height - 1, 0x80404040), gh.random_rgba(r, width, height, 8, 0)]
    r_off = np.concatenate([[0], np.cumsum([4 * im.size for im in images])]).astype(np.int64)
    f_off = gh.file_slots(fd, [height] * len(images), width, 8, 0)
    file = torch.full((int(f_off[-1]),), GUARD, dtype=torch.uint8, device="cuda")
    file_len, st = fd.png_encode_rgba_files_batch(gh.dev(np.concatenate([im.view(np.uint8) for im in images])), gh.dev(r_off), file, gh.dev(f_off), width, 8, 0)
    torch.cuda.synchronize()
    lens, host = file_len.cpu().tolist(), file.cpu().numpy()
    assert st.cpu().tolist() == [0, 13, 0, 13, 0] and lens[1] == 0 and lens[3] == 0
    for k in (0, 2, 4):
        assert pc.pillow_rgba(host[f_off[k]:f_off[k] + lens[k]].tobytes()) == images[k].view(np.uint8).tobytes(), k


def test_bench_shape_rgb8_and_palette8():
    """4096 images of 341 x 64: packing to RGB8 equals dropping the alpha plane in torch; analysis of images that all use
    the same 256 colours gives the sorted colours, and packing to palette-8 gives each pixel's rank among them."""
    import torch
    import fdeflate_amd as fd
    n, width, rows = 4096, 341, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(10900)
    rgb = torch.randint(0, 256, (n, rows, width, 3), dtype=torch.uint8, device="cuda", generator=g)
    rgba = torch.cat([rgb, torch.full((n, rows, width, 1), 255, dtype=torch.uint8, device="cuda")], dim=3).contiguous()
    r_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 4)
    p_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 3)
    pix = torch.empty(n * rows * width * 3, dtype=torch.uint8, device="cuda")
    st = fd.png_pack_batch(rgba.view(-1), r_off, pix, p_off, width, 8, 2)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and torch.equal(pix.view(n, rows, width, 3), rgb)
    del rgb, pix
    colours = torch.randint(0, 1 << 31, (256,), dtype=torch.int64, device="cuda", generator=g) * 2 + torch.arange(256, device="cuda") % 2
    colours = torch.unique(colours)
    assert colours.numel() == 256                                   # (sorted, as unsigned 32-bit values)
    idx = torch.randint(0, 256, (n, rows, width), dtype=torch.int64, device="cuda", generator=g)
    shuffled = colours[torch.randperm(256, device="cuda", generator=g)]
    words = shuffled[idx]
    rgba.view(torch.int32).view(n, rows, width).copy_(torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32))
    pal, colour, trns_len, summary, st = fd.png_analyse_batch(rgba.view(-1), r_off, width, 256)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and bool((colour[:, 0] == 256).all())
    signed = torch.where(colours >= 1 << 31, colours - (1 << 32), colours).to(torch.int32)
    assert torch.equal(pal, signed.expand(n, 256))
    assert bool((trns_len == int((colours < 0xFF000000).sum())).all())
    i_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width)
    index = torch.empty(n * rows * width, dtype=torch.uint8, device="cuda")
    st = fd.png_pack_batch(rgba.view(-1), r_off, index, i_off, width, 8, 3, pal=pal, colour=colour)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    assert torch.equal(index.view(n, rows, width), torch.searchsorted(colours, words).to(torch.uint8))
