"""-m gpu: PNG at 16 bits per sample -- fdh_png_expand16_batch, fdh_png_expand16_mixed_batch, fdh_png_pack16_batch and
the three pipelines of fdeflate_amd.png16.

Referee: tests/png16_model.py (plain integers, pinned to the RGBA8 model, to numpy and to Pillow by
tests/test_png16_model.py); Pillow once more on 16-bit grey files, the one class it reads and writes exactly.
Everything is bit-exact.

The kernels are png_expand_kernel's at eight bytes per output pixel: grid(n, waves), a wavefront takes the bands b,
b + waves, .. of 64 rows of its image; FDH_PNG_EXPAND16_WAVES / FDH_PNG_PACK16_WAVES force the number of wavefronts per
image.  The shapes are those of tests/test_gpu_png_expand.py, for the same reasons.
"""
import io
import zlib

import numpy as np
import pytest

import png16_model as m16
import png_adam7_model as am
import png_corpus as pc
import png_expand_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_mixed_model as mm
from png_gpu_harness import GUARD, HEIGHTS, PASSED_ON

pytestmark = pytest.mark.gpu

STARTS = (0, 2, 8, 10, 4, 14, 6, 12)        # output slot starts mod 16: aligned, 2 mod 16, one pixel off, the rest
DEPTH16 = (0, 2, 4, 6)


def _p16():
    import fdeflate_amd.png16 as p16
    return p16


def _slots(sizes, starts=STARTS):
    """Offsets of 2 * len(sizes) slots: slot 2k holds sizes[k] bytes and starts at starts[k % ..] mod 16, slot 2k + 1 is
    the guard between it and the next (two bytes at least)."""
    off = [starts[0]]
    for k, size in enumerate(sizes):
        end = off[-1] + size
        nxt = end + 2
        nxt += (starts[(k + 1) % len(starts)] - nxt) % 16
        off += [end, nxt]
    return np.asarray(off, dtype=np.int64)


class Batch16:
    """Images one behind the other from an odd byte of a buffer of guard bytes, and their RGBA16 slots at the starts of
    STARTS with a slot of guard bytes between every two (an entry with no pixels that `upstream` marks as failed: its
    slot must stay as it is)."""

    def __init__(self, images, width, depth, colour, front=3):
        """images: [(pix uint8, key or None, pal or None)]"""
        self.geometry = (width, depth, colour)
        self.n = 2 * len(images)
        p_off, self.want, self.want_status = [front], [], []
        for pix, key, pal in images:
            rgba, st = m16.expand16(pix, width, depth, colour, key, pal)
            p_off += [p_off[-1] + pix.size] * 2
            self.want.append(np.frombuffer(rgba, dtype=np.uint8))
            self.want_status += [st, PASSED_ON]
        self.p_off, self.r_off = np.asarray(p_off, dtype=np.int64), _slots([w.size for w in self.want])
        self.pix = np.full(int(p_off[-1]) + 7, GUARD, dtype=np.uint8)
        for k, (pix, _, _) in enumerate(images):
            self.pix[p_off[2 * k]:p_off[2 * k + 1]] = pix
        self.expect = np.full(int(self.r_off[-1]) + 64, GUARD, dtype=np.uint8)
        for k, w in enumerate(self.want):
            self.expect[self.r_off[2 * k]:self.r_off[2 * k + 1]] = w
        self.upstream = [0, PASSED_ON] * len(images)
        self.pal = self.colour = None
        if colour == 3:
            self.pal = [w for _, _, pal in images for w in (em.pal_words(pal), [0] * 256)]
            self.colour = [w for _, _, pal in images for w in (em.colour_words(len(pal), None), [0] * 4)]
        elif any(key is not None for _, key, _ in images):
            self.colour = [w for _, key, _ in images for w in (em.colour_words(0, key), [0] * 4)]

    def check(self, what):
        import torch
        d_pix = gh.dev(self.pix)
        rgba = torch.full((self.expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        assert rgba.data_ptr() % 16 == 0
        st = torch.full((self.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        _p16().png_expand16_batch(d_pix, gh.dev(self.p_off), rgba, gh.dev(self.r_off), *self.geometry,
                                  pal=None if self.pal is None else gh.words(self.pal),
                                  colour=None if self.colour is None else gh.words(self.colour),
                                  upstream=gh.words(self.upstream), png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        assert np.array_equal(d_pix.cpu().numpy(), self.pix)
        st = st.cpu().numpy()
        assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + self.n:] == 0x5A5A5A5A).all()
        assert st[8:8 + self.n].tolist() == self.want_status, what
        got = rgba.cpu().numpy()
        if not np.array_equal(got, self.expect):
            at = int(np.nonzero(got != self.expect)[0][0])
            raise AssertionError("%r: byte %d of the output is %d, not %d (slots at %s)" % (what, at, got[at], self.expect[at], self.r_off.tolist()))


# ---- fdh_png_expand16_batch ----

@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_expand16_every_width_and_height(pair, monkeypatch):
    """Every width of gh.EXPAND_WIDTHS at heights 1, 2, 3 and one more than a band, one batch per width: the output buffer equals
    the model's byte for byte, guard slots and the bytes behind the last slot included, and every status is right.  The
    slots start at 0, 2, 8 and 10 mod 16.  Each batch runs with one wavefront per image (a wavefront takes two bands)
    and with seven (more wavefronts than bands)."""
    depth, colour = pair
    r = np.random.default_rng(16500 + 64 * colour + depth)
    for width in gh.EXPAND_WIDTHS:
        b = Batch16([pc.random_case(r, width, h, depth, colour, colour == 3) for h in HEIGHTS], width, depth, colour)
        assert [int(o) % 16 for o in b.r_off[0::2][:4]] == [0, 2, 8, 10]
        for waves in (1, 7):
            gh.set_env(monkeypatch, FDH_PNG_EXPAND16_WAVES=waves)
            b.check((pair, width, waves))


@pytest.mark.parametrize("pair", ((1, 0), (16, 0), (8, 2), (16, 2)), ids=lambda p: "depth%d-colour%d" % p)
def test_keys_present_and_absent(pair, monkeypatch):
    """Images with a tRNS key between images without one in the same call.  The key is an image's first pixel, further
    pixels repeat it, and at depth 16 some of those differ from it in a low byte only: they stay opaque."""
    depth, colour = pair
    r = np.random.default_rng(16600 + 64 * colour + depth)
    for width in (1, 2, 5, 33, 64, 257):
        images = [pc.random_case(r, width, h, depth, colour, k % 2 == 0) for k, h in enumerate((3, 3, gh.BAND + 1, 2, 5))]
        b = Batch16(images, width, depth, colour)
        for k, w in enumerate(b.want):
            alpha = w.view("<u2")[3::4]
            assert set(alpha.tolist()) <= {0, 65535} and (0 in alpha) == (k % 2 == 0)
        if depth == 16 and width >= 33:
            pix, key, _ = images[2]
            s = np.frombuffer(pix.tobytes(), dtype=">u2").reshape(-1, fm.CHANNELS[colour])
            near = [(row >> 8 == np.array(key) >> 8).all() and not (row == np.array(key)).all() for row in s]
            assert any(near)                    # the high bytes match, the pixel is not the key
            alpha = b.want[2].view("<u2")[3::4]
            assert all(alpha[j] == 65535 for j, hit in enumerate(near) if hit)
        for waves in (1, 7):
            gh.set_env(monkeypatch, FDH_PNG_EXPAND16_WAVES=waves)
            b.check((pair, width, waves))


@pytest.mark.parametrize("depth", (1, 2, 4, 8))
def test_palette_sizes_and_an_index_outside(depth, monkeypatch):
    """Palettes of 1, 2, 255 and 256 entries (those the depth can index) with a tRNS, whose images stay inside them, and
    one of 2^depth - 1 entries whose image holds the last index: that image gets status 9, its pixels are the model's
    ((0, 0, 0, 65535) at that index), and its neighbours get 0."""
    r = np.random.default_rng(16700 + depth)
    top = 1 << depth
    cases = [(e, False) for e in (1, 2, 255, 256) if e <= top] + [(top - 1, True), (top, False)]
    for width in (5, 33, 257):
        rb = fm.geometry(width, depth, 3)[0]
        images = []
        for entries, outside in cases:
            rows = 3
            idx = r.integers(0, top if outside else entries, (rows, width))
            if outside:
                idx[1, width // 2] = top - 1                   # the last index is present
            bits = np.zeros((rows, rb * 8), dtype=np.uint8)
            for k in range(depth):
                bits[:, k:width * depth:depth] = (idx >> (depth - 1 - k)) & 1
            bits[:, width * depth:] = r.integers(0, 2, (rows, rb * 8 - width * depth), dtype=np.uint8)      # padding bits: ignored
            pix = np.packbits(bits, axis=1).reshape(-1)
            pal = em.palette(r.integers(0, 256, 3 * entries, dtype=np.uint8).tobytes(), r.integers(0, 256, entries, dtype=np.uint8).tobytes())
            images.append((pix, None, pal))
        b = Batch16(images, width, depth, 3)
        assert b.want_status[0::2] == [9 if outside else 0 for _, outside in cases]
        for waves in (1, 7):
            gh.set_env(monkeypatch, FDH_PNG_EXPAND16_WAVES=waves)
            b.check((depth, width, waves))


def test_slots_that_do_not_fit_misaligned_slots_and_upstream():
    """A pixel slot of rows and a half, an output slot one pixel short and one pixel long, an output slot of the right
    size at an odd address: status 2 and no byte changes.  upstream != 0: that value is the status and the slot is
    untouched.  An empty pixel slot with an empty output slot: status 0.  The images in between are exact."""
    import torch
    r = np.random.default_rng(16800)
    for (depth, colour), width in (((8, 2), 21), ((1, 0), 21), ((8, 3), 70), ((16, 6), 9), ((16, 0), 5)):
        rb = fm.geometry(width, depth, colour)[0]
        rows = 4
        pal = em.palette(bytes(range(256)) * 3) if colour == 3 else None
        full, out = rows * rb, rows * width * 8
        # (pixel bytes, output bytes, bytes skipped in front of the output slot, upstream, expected status)
        plan = [(full, out, 0, 0, 0), (full + rb // 2 + 1, out + width * 8, 0, 0, 2), (full, out, 0, 0, 0), (full, out - 8, 0, 0, 2),
                (full, out + 8, 0, 0, 2), (0, 0, 0, 0, 0), (full, out, 0, 5, 5), (full, out, 0, 0, 0), (full, out, 0, 0x80000003, 0x80000003),
                (0, 8, 0, 0, 2), (rb, 0, 0, 0, 2), (full, out, 1, 0, 2), (full, out, 1, 0, 0), (full, out, 0, 0, 0)]
        # one offsets array: a slot that is "skipped into" is made by a guard entry of one byte in front of it
        entries = []
        for pb, ob, skip, up, want in plan:
            if skip:
                entries.append((0, skip, PASSED_ON, PASSED_ON))
            entries.append((pb, ob, up, want))
        p_sizes = [e[0] for e in entries]
        r_sizes = [e[1] for e in entries]
        p_off = np.concatenate([[1], 1 + np.cumsum(p_sizes)]).astype(np.int64)
        r_off = np.concatenate([[4], 4 + np.cumsum(r_sizes)]).astype(np.int64)
        pix = r.integers(0, 256, int(p_off[-1]) + 3, dtype=np.uint8)
        expect = np.full(int(r_off[-1]) + 32, GUARD, dtype=np.uint8)
        odd = 0
        for k, (pb, ob, up, want) in enumerate(entries):
            if want == 2 and pb == full and ob == out:
                assert r_off[k] % 2 == 1
                odd += 1
            if want == 0 and pb:
                assert r_off[k] % 2 == 0
                rgba, st = m16.expand16(pix[p_off[k]:p_off[k + 1]], width, depth, colour, None, pal)
                assert st == 0
                expect[r_off[k]:r_off[k + 1]] = np.frombuffer(rgba, dtype=np.uint8)
        assert odd == 1
        rgba = torch.full((expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        n = len(entries)
        st = _p16().png_expand16_batch(gh.dev(pix), gh.dev(p_off), rgba, gh.dev(r_off), width, depth, colour,
                                       pal=gh.words([em.pal_words(pal)] * n) if pal else None,
                                       colour=gh.words([em.colour_words(256, None)] * n) if pal else None,
                                       upstream=gh.words([e[2] for e in entries]))
        torch.cuda.synchronize()
        assert st.cpu().numpy().view(np.uint32).tolist() == [e[3] for e in entries], (depth, colour)
        assert np.array_equal(rgba.cpu().numpy(), expect), (depth, colour)


def test_more_images_than_wavefronts_fill():
    """5000 images of 3 x 7 two-bit palette pixels, of 2 x 5 sixteen-bit grey + alpha pixels and of 5 x 3 one-bit grey
    pixels in one call each (one wavefront per image; rows of a few pixels share a step), against the model."""
    import torch
    r = np.random.default_rng(16900)
    n = 5000
    for (depth, colour), width, rows in (((2, 3), 7, 3), ((16, 4), 5, 2), ((1, 0), 3, 5)):
        rb = fm.geometry(width, depth, colour)[0]
        pix = r.integers(0, 256, n * rows * rb + 1, dtype=np.uint8)
        pal = em.palette(r.integers(0, 256, 9, dtype=np.uint8).tobytes(), b"\x07") if colour == 3 else None
        p_off = 1 + np.arange(n + 1, dtype=np.int64) * (rows * rb)
        r_off = np.arange(n + 1, dtype=np.int64) * (rows * width * 8)
        want, want_st = m16.expand16(pix[1:], width, depth, colour, None, pal)     # (whole rows: the images one below the other)
        per = [em.expand(pix[p_off[k]:p_off[k + 1]], width, depth, colour, None, pal)[1] for k in range(n)]   # (statuses: the same in both models)
        assert (want_st == 9) == (colour == 3) and (colour != 3 or 0 in per)
        rgba = torch.full((int(r_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
        st = _p16().png_expand16_batch(gh.dev(pix), gh.dev(p_off), rgba, gh.dev(r_off), width, depth, colour,
                                       pal=gh.words([em.pal_words(pal)] * n) if pal else None,
                                       colour=gh.words([em.colour_words(3, None)] * n) if pal else None)
        torch.cuda.synchronize()
        got = rgba.cpu().numpy()
        assert st.cpu().tolist() == per
        assert got[:int(r_off[-1])].tobytes() == want and (got[int(r_off[-1]):] == GUARD).all()


# ---- fdh_png_expand16_mixed_batch ----

def _mixed_model(rec, pix, col, pal):
    """The model on one image of a mixed call -> (RGBA16 bytes, status)."""
    w, d, c = rec["width"], rec["bit_depth"], rec["colour_type"]
    if not mm.decodable(rec):
        return b"", 3
    p = key = None
    if c == 3:
        if pal is None:
            return b"", 10
        p = [(int(v) & 255, int(v) >> 8 & 255, int(v) >> 16 & 255, int(v) >> 24) for v in pal[:col[0]]]
    elif col[1]:
        key = (col[2] & 0xFFFF, col[2] >> 16, col[3])[:3 if c == 2 else 1]
    return m16.expand16(pix, w, d, c, key, p)


def _mixed_call(images, with_pal=True, short=()):
    """fdh_png_expand16_mixed_batch over `images` with a passed-on guard entry behind each -> (statuses of the images,
    their slots' bytes, the model's (bytes, status)); guards, the bytes around the buffer and the status array's
    surroundings are checked here.  short: the images whose slot is one pixel short."""
    import torch
    n = len(images)
    want = [_mixed_model(rec, pix, col, pal if with_pal else None) for rec, pix, col, pal in images]
    # a slot has the plan's size whatever the status will be (the record decides; an undecodable one gets 8 bytes)
    sizes = [(2 * mm.plan(rec)[4] if mm.decodable(rec) else 8) - (8 if k in short else 0) for k, (rec, _, _, _) in enumerate(images)]
    r_off = _slots(sizes)
    p_off = [3]
    for _, pix, _, _ in images:
        p_off += [p_off[-1] + pix.size] * 2
    p_off = np.asarray(p_off, dtype=np.int64)
    host = np.full(int(p_off[-1]) + 5, GUARD, dtype=np.uint8)
    for k, (_, pix, _, _) in enumerate(images):
        host[p_off[2 * k]:p_off[2 * k + 1]] = pix
    guard_rec = mm.record(3, 2, 8, 0)
    info = gh.words([w for rec, _, _, _ in images for w in (mm.words(rec), mm.words(guard_rec))]).view(-1, 8)
    pal = np.full((2 * n, 256), 0x5A5A5A5A, dtype=np.uint32)
    col = np.zeros((2 * n, 4), dtype=np.uint32)
    for k, (_, _, c, p) in enumerate(images):
        col[2 * k] = c
        if p is not None:
            pal[2 * k] = p
    rgba = torch.full((int(r_off[-1]) + 48,), GUARD, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    _p16().png_expand16_mixed_batch(gh.dev(host), gh.dev(p_off), rgba, gh.dev(r_off), info, pal=gh.dev(pal.view(np.int32)) if with_pal else None,
                                    colour=gh.dev(col.view(np.int32)), upstream=gh.words([0, PASSED_ON] * n), png_status=st[8:8 + 2 * n])
    torch.cuda.synchronize()
    st, got = st.cpu().numpy(), rgba.cpu().numpy()
    assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + 2 * n:] == 0x5A5A5A5A).all()
    st = st[8:8 + 2 * n].tolist()
    assert st[1::2] == [PASSED_ON] * n
    assert (got[:int(r_off[0])] == GUARD).all() and (got[int(r_off[-1]):] == GUARD).all()
    for k in range(n):
        assert (got[r_off[2 * k + 1]:r_off[2 * k + 2]] == GUARD).all(), k
    return st[0::2], [got[r_off[2 * k]:r_off[2 * k + 1]].tobytes() for k in range(n)], want


def _mixed_image(r, width, height, depth, colour, k):
    rec = mm.record(width, height, depth, colour, idat_bytes=9)
    pix, key, pal = pc.random_case(r, width, height, depth, colour, k % 2 == 0, entries=(1, 2, 1 << depth)[k % 3] if colour == 3 else None)
    if colour == 3:
        return rec, pix, em.colour_words(len(pal), None), np.array(em.pal_words(pal), dtype=np.uint32)
    return rec, pix, em.colour_words(0, key), None


def test_mixed_batch_every_pair_shuffled(monkeypatch):
    """All fifteen pairs at several widths and heights, shuffled into one call: every slot and status is the model's,
    and equal to what fdh_png_expand16_batch gives for the image alone."""
    import torch
    r = np.random.default_rng(17000)
    images, k = [], 0
    for depth, colour in fm.PAIRS:
        for width, height in ((1, 1), (3, 2), (7, gh.BAND + 1), (33, 3), (64, 2), (257, 1)):
            images.append(_mixed_image(r, width, height, depth, colour, k))
            k += 1
    images = [images[j] for j in r.permutation(len(images))]
    for waves in (1, 7):
        gh.set_env(monkeypatch, FDH_PNG_EXPAND16_WAVES=waves)
        st, slots, want = _mixed_call(images)
        for j, (w, s, got) in enumerate(zip(want, st, slots)):
            assert s == w[1] and got == w[0], (j, images[j][0])
    assert {0, 9} <= set(st)                # (random indices above a short palette's count)
    # each image alone through the per-geometry call
    for j, (rec, pix, col, pal) in enumerate(images):
        out = torch.full((len(slots[j]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
        off = np.array([0, len(slots[j])], dtype=np.int64)
        alone = _p16().png_expand16_batch(gh.dev(pix), gh.dev(np.array([0, pix.size], dtype=np.int64)), out, gh.dev(off), rec["width"], rec["bit_depth"],
                                          rec["colour_type"], pal=gh.words([pal.tolist()]) if pal is not None else None, colour=gh.words([col]))
        assert alone.cpu().tolist() == [st[j]] and out.cpu().numpy()[:len(slots[j])].tobytes() == slots[j], (j, rec)


def test_mixed_batch_refuses_one_image_among_good_ones():
    """A record that is not decodable (3), colour type 3 without `pal` (10), an index outside the palette (9, written in
    full), a slot one pixel short (2): each between good images, which are exact."""
    r = np.random.default_rng(17100)
    good = [_mixed_image(r, w, h, d, c, k) for k, (w, h, d, c) in enumerate(((5, 3, 16, 6), (9, 2, 8, 2), (33, 1, 16, 0), (4, 4, 1, 0), (7, 3, 16, 2)))]
    bad_rec = (mm.record(5, 3, 3, 0), r.integers(0, 256, 8, dtype=np.uint8), [0, 0, 0, 0], None)
    no_height = (mm.record(5, 0, 8, 0), r.integers(0, 256, 8, dtype=np.uint8), [0, 0, 0, 0], None)
    scanned_bad = (mm.record(5, 3, 8, 0, status=6), r.integers(0, 256, 15, dtype=np.uint8), [0, 0, 0, 0], None)
    pal_img = _mixed_image(r, 6, 2, 4, 3, 2)                               # sixteen entries
    short_pal = pal_img[3].copy()
    short_pal[14:] = 0xFF000000                                           # (as fdh_png_colour_batch writes a PLTE of fourteen)
    outside = (pal_img[0], np.full(6, 0xFE, dtype=np.uint8), em.colour_words(14, None), short_pal)
    images = [good[0], bad_rec, good[1], no_height, good[2], scanned_bad, good[3], outside, good[4]]
    st, slots, want = _mixed_call(images)
    assert st == [0, 3, 0, 3, 0, 3, 0, 9, 0] and [w[1] for w in want] == st
    for j in (0, 2, 4, 6, 7, 8):
        assert slots[j] == want[j][0], j
    for j in (1, 3, 5):
        assert slots[j] == bytes([GUARD]) * 8
    # a slot one pixel short: 2, nothing written
    st, slots, want = _mixed_call([good[0], good[4], good[1]], short=(1,))
    assert st == [0, 2, 0] and slots[0] == want[0][0] and slots[2] == want[2][0] and set(slots[1]) == {GUARD}
    # without pal: the palette image is 10 and untouched, the others are as before
    images = [good[0], pal_img, good[1]]
    st, slots, want = _mixed_call(images, with_pal=False)
    assert st == [0, 10, 0] and slots[0] == want[0][0] and slots[2] == want[2][0] and set(slots[1]) == {GUARD}


# ---- fdh_png_pack16_batch ----

def _representable(r, n, colour):
    p = r.integers(0, 65536, (n, 4)).astype(np.uint16)
    if colour in (0, 4):
        p[:, 1] = p[:, 2] = p[:, 0]
    if colour in (0, 2):
        p[:, 3] = 65535
    return p.astype("<u2").view(np.uint8).reshape(-1)


def _pack_call(pictures, width, colour, upstream=None, starts=STARTS, slack=0):
    """fdh_png_pack16_batch over `pictures` (uint8 arrays of RGBA16 bytes) at the input starts of `starts`, a passed-on
    guard entry behind each -> (statuses, packed slots); everything around the slots is checked."""
    import torch
    n = len(pictures)
    ch2 = 2 * fm.CHANNELS[colour]
    s_off = _slots([p.size for p in pictures], starts)
    host = np.full(int(s_off[-1]) + 16, GUARD, dtype=np.uint8)
    for k, p in enumerate(pictures):
        host[s_off[2 * k]:s_off[2 * k + 1]] = p
    sizes = [p.size // 8 * ch2 + slack for p in pictures]
    o_off = [5]
    for k, s in enumerate(sizes):
        o_off += [o_off[-1] + s, o_off[-1] + s + 3 + k % 4]
    o_off = np.asarray(o_off, dtype=np.int64)
    d_in = gh.dev(host)
    assert d_in.data_ptr() % 16 == 0
    out = torch.full((int(o_off[-1]) + 32,), GUARD, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    up = [v for u in (upstream or [0] * n) for v in (u, PASSED_ON)]
    _p16().png_pack16_batch(d_in, gh.dev(s_off), out, gh.dev(o_off), width, colour, upstream=gh.words(up), png_status=st[8:8 + 2 * n])
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), host)
    st, got = st.cpu().numpy(), out.cpu().numpy()
    assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + 2 * n:] == 0x5A5A5A5A).all()
    st = st[8:8 + 2 * n].view(np.uint32).tolist()
    assert st[1::2] == [PASSED_ON] * n
    assert (got[:5] == GUARD).all() and (got[int(o_off[-1]):] == GUARD).all()
    for k in range(n):
        assert (got[o_off[2 * k + 1]:o_off[2 * k + 2]] == GUARD).all(), k
    return st[0::2], [got[o_off[2 * k]:o_off[2 * k + 1]] for k in range(n)]


@pytest.mark.parametrize("colour", DEPTH16)
def test_pack16_every_width_and_height(colour, monkeypatch):
    """Representable pictures of every width of gh.EXPAND_WIDTHS at heights 1, 2, 3 and one more than a band, between guards, the
    RGBA16 slots starting at 0, 2, 8 and 10 mod 16: the packed bytes are the model's, and fdh_png_expand16_batch takes
    them back to the pictures."""
    import torch
    r = np.random.default_rng(17200 + colour)
    for width in gh.EXPAND_WIDTHS:
        pictures = [_representable(r, width * h, colour) for h in HEIGHTS]
        want = [m16.pack16(p.tobytes(), width, colour) for p in pictures]
        assert all(w[1] == 0 for w in want)
        for waves in (1, 7):
            gh.set_env(monkeypatch, FDH_PNG_PACK16_WAVES=waves)
            st, slots = _pack_call(pictures, width, colour)
            assert st == [0] * len(pictures), (width, waves)
            for k, (s, w) in enumerate(zip(slots, want)):
                assert s.tobytes() == w[0], (width, waves, k)
        packed = np.concatenate(slots)
        p_off = np.concatenate([[0], np.cumsum([s.size for s in slots])]).astype(np.int64)
        r_off = np.concatenate([[0], np.cumsum([p.size for p in pictures])]).astype(np.int64)
        back = torch.empty(int(r_off[-1]), dtype=torch.uint8, device="cuda")
        st = _p16().png_expand16_batch(gh.dev(packed), gh.dev(p_off), back, gh.dev(r_off), width, 16, colour)
        assert st.cpu().tolist() == [0] * len(pictures) and np.array_equal(back.cpu().numpy(), np.concatenate(pictures)), width


def test_pack16_every_reason_for_status_13_status_2_and_upstream():
    """One pixel that the pair cannot hold -- G or B off by one from R, in a high byte only, A one below 65535 or with a
    low byte only -- in the first, a middle and the last pixel of a picture of two bands: 13 for that picture and 0 for
    its neighbours, which are exact.  A pix slot one byte long, an RGBA16 slot at an odd address and one of half a row:
    2, nothing written.  An upstream value is passed on."""
    import torch
    r = np.random.default_rng(17300)
    width, rows = 13, gh.BAND + 2
    n = width * rows
    reasons = {0: ((1, 1), (2, 1), (1, 0x100), (3, -1), (3, -0xFF00)), 4: ((1, 1), (2, 1), (2, 0x100)), 2: ((3, -1), (3, -0xFF00), (3, -65535))}
    for colour, cases in reasons.items():
        for channel, delta in cases:
            for at in (0, n // 2, n - 1):
                base = [_representable(r, n, colour) for _ in range(3)]
                bad = base[1].copy().view("<u2").reshape(-1, 4)
                bad[at, 0] = 0x2345 if channel != 3 else bad[at, 0]
                if colour in (0, 4):
                    bad[at, 1] = bad[at, 2] = bad[at, 0]
                bad[at, channel] = int(bad[at, channel]) + delta
                base[1] = bad.reshape(-1).view(np.uint8)
                assert m16.pack16(base[1].tobytes(), width, colour)[1] == 13
                st, slots = _pack_call(base, width, colour)
                assert st == [0, 13, 0], (colour, channel, delta, at)
                for k in (0, 2):
                    assert slots[k].tobytes() == m16.pack16(base[k].tobytes(), width, colour)[0]
    for colour in DEPTH16:
        pictures = [_representable(r, width * 3, colour) for _ in range(4)]
        st, slots = _pack_call(pictures, width, colour, slack=1)                      # every pix slot one byte long
        assert st == [2] * 4 and all((s == GUARD).all() for s in slots)
        st, slots = _pack_call(pictures, width, colour, starts=(0, 3, 8, 2))           # the second RGBA16 slot at an odd address
        assert st == [0, 2, 0, 0] and (slots[1] == GUARD).all()
        for k in (0, 2, 3):
            assert slots[k].tobytes() == m16.pack16(pictures[k].tobytes(), width, colour)[0]
        st, slots = _pack_call(pictures, width, colour, upstream=[0, 6, 0x80000001, 0])
        assert st == [0, 6, 0x80000001, 0] and (slots[1] == GUARD).all() and (slots[2] == GUARD).all()
        half = [pictures[0], pictures[1][:width * 8 * 2 + width * 4], pictures[2]]
        import fdeflate_amd.png16 as p16
        s_off = np.concatenate([[0], np.cumsum([p.size for p in half])]).astype(np.int64)
        o_off = s_off // 8 * 2 * fm.CHANNELS[colour]
        out = torch.full((int(o_off[-1]) + 8,), GUARD, dtype=torch.uint8, device="cuda")
        st = p16.png_pack16_batch(gh.dev(np.concatenate(half)), gh.dev(s_off), out, gh.dev(o_off), width, colour)
        assert st.cpu().tolist() == [0, 2, 0] and (out.cpu().numpy()[int(o_off[1]):int(o_off[2])] == GUARD).all()


def test_pack16_refuses_colour_type_3():
    import torch
    from fdeflate_amd._lib import FdeflateHipError
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for colour in (3, 1, 5, 7):
        with pytest.raises(FdeflateHipError):
            _p16().png_pack16_batch(buf, off, buf, off, 4, colour)
    with pytest.raises(ValueError):
        _p16().png_encode_rgba16_files_batch(buf, off, buf, off, 4, 3)


# ---- files -> RGBA16, RGBA16 -> files ----

def _pillow_grey16(png):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == "I;16"
    return np.asarray(im).astype(np.uint16)


def _model_file(r, width, height, depth, colour, keyed, method=0, idat_chunks=2):
    """(file, RGBA16 bytes by the model) of a model-written file: a tEXt in front, PLTE, tRNS, random filter types."""
    import png_model as pm
    pix, key, pal = pc.random_case(r, width, height, depth, colour, keyed)
    rb, bpp = fm.geometry(width, depth, colour)
    if method:
        idat = am.stream_of(pix.tobytes(), width, height, depth, colour, r.integers(0, 5, am.pass_rows(width, height)).tolist())
    else:
        idat = zlib.compress(pm.filter_rows(pix.reshape(height, rb), bpp, r.integers(0, 5, height).tolist()).tobytes())
    f = am.write_file(idat, width, height, depth, colour, pc.pre_chunks(colour, key, pal, text=True), idat_chunks, zlib.crc32, method=method)
    rgba, st = m16.expand16(pix, width, depth, colour, key, pal)
    assert st == 0
    return f, rgba


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_files_of_one_geometry_to_rgba16(pair):
    """Model-written files of two heights (one with a key or tRNS, one interlaced) through
    png_decode_files_rgba16_batch: every picture is the model's, a grey-16 picture is Pillow's as well."""
    import torch
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(17400 + 64 * colour + depth)
    width = 37
    made = [_model_file(r, width, 3, depth, colour, colour in (0, 2, 3)), _model_file(r, width, 70, depth, colour, False),
            _model_file(r, width, 9, depth, colour, False, method=1)]
    heights = (3, 70, 9)
    host, f_off, f_len = gh.batch_of([f for f, _ in made])
    rgba, rgba_off, info, status, png_status = _p16().png_decode_files_rgba16_batch(gh.dev(host), gh.dev(f_off), width, depth, colour,
                                                                                    file_len=gh.dev(f_len), flags=fd.PNG_FLAG_ADAM7)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 3 and png_status.cpu().tolist() == [0] * 3
    off = rgba_off.cpu().tolist()
    assert off == np.concatenate([[0], np.cumsum([h * width * 8 for h in heights])]).tolist() and rgba.numel() == off[-1]
    for k, (f, want) in enumerate(made):
        picture = rgba[off[k]:off[k + 1]].view(torch.int16).view(heights[k], width, 4)
        assert picture.cpu().numpy().tobytes() == want, (pair, k)
        if pair == (16, 0) and k == 1:
            assert np.array_equal(_pillow_grey16(f), picture[..., 0].cpu().numpy().view(np.uint16))


@pytest.fixture(scope="module")
def mixed_files():
    """[(file, RGBA16 bytes, (width, height))]: model-written files of every pair, each plain and interlaced."""
    r = np.random.default_rng(17500)
    out, k = [], 0
    for depth, colour in fm.PAIRS:
        for method in (0, 1):
            w, h = 1 + (5 * k) % 41, 1 + (3 * k) % 11
            f, rgba = _model_file(r, w, h, depth, colour, k % 2 == 0 and colour in (0, 2, 3), method=method, idat_chunks=1 + k % 3)
            out.append((f, rgba, (w, h)))
            k += 1
    return out


@pytest.mark.parametrize("kind", ["any geometry", "one geometry"])
def test_mixed_files_to_rgba16_with_one_read_back_of_48_bytes(mixed_files, kind, monkeypatch):
    """Files of all fifteen pairs, half of them interlaced, through png_decode_mixed_files_rgba16_batch with
    PNG_FLAG_ADAM7 (the mixed route), and four RGB16 files of one width (the uniform route): every picture is the
    model's; exactly 48 bytes leave the device, through api._read_back, once."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import api
    if kind == "one geometry":
        r = np.random.default_rng(17550)
        mixed_files = [_model_file(r, 21, h, 16, 2, k == 0) + ((21, h),) for k, h in enumerate((4, 30, 5, 12))]
    route = None
    host, f_off, f_len = gh.batch_of([f for f, _, _ in mixed_files])
    d_file, d_off, d_len = gh.dev(host), gh.dev(f_off), gh.dev(f_len)
    moved, stray = [], []
    inner = api._read_back
    originals = {name: getattr(torch.Tensor, name) for name in ("cpu", "tolist", "item", "numpy")}

    def counted(t):
        moved.append(t.numel() * t.element_size())
        with monkeypatch.context() as m:        # (the wrapper itself may use any of them)
            for name in originals:
                m.setattr(torch.Tensor, name, originals[name])
            return inner(t)

    def spy(name):
        def call(self, *a, **k):
            if self.is_cuda:
                stray.append(name)
            return originals[name](self, *a, **k)
        return call

    monkeypatch.setattr(api, "_read_back", counted)
    for name in originals:
        monkeypatch.setattr(torch.Tensor, name, spy(name))
    rgba, rgba_off, info, status, png_status = _p16().png_decode_mixed_files_rgba16_batch(d_file, d_off, d_len, flags=fd.PNG_FLAG_ADAM7, route=route)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert moved == [48] and stray == [], (moved, stray)
    assert status.cpu().tolist() == [0] * len(mixed_files) and png_status.cpu().tolist() == [0] * len(mixed_files)
    off, got = rgba_off.cpu().tolist(), rgba.cpu().numpy()
    assert rgba.numel() == off[-1]
    for k, (f, want, (w, h)) in enumerate(mixed_files):
        assert off[k + 1] - off[k] == h * w * 8 and got[off[k]:off[k + 1]].tobytes() == want, k


def test_uniform_route_and_max_bytes():
    """A batch of one geometry takes the uniform route and gives the same tensors as route="mixed" and as
    png_decode_files_rgba16_batch.  max_bytes between a file's RGBA8 and RGBA16 sizes: status 2 and empty slots for
    that file alone -- png_decode_mixed_files_rgba_batch still decodes it."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(17600)
    width = 21
    made = [_model_file(r, width, h, 16, 2, False) for h in (4, 30, 5, 12)]
    host, f_off, f_len = gh.batch_of([f for f, _ in made])
    d_file, d_off, d_len = gh.dev(host), gh.dev(f_off), gh.dev(f_len)
    chosen = _p16().png_decode_mixed_files_rgba16_batch(d_file, d_off, d_len)
    forced = _p16().png_decode_mixed_files_rgba16_batch(d_file, d_off, d_len, route="mixed")
    uniform = _p16().png_decode_mixed_files_rgba16_batch(d_file, d_off, d_len, route="uniform")
    old = _p16().png_decode_files_rgba16_batch(d_file, d_off, width, 16, 2, file_len=d_len)
    for a, b, c, d in zip(chosen, forced, uniform, old):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert chosen[0].cpu().numpy().tobytes() == b"".join(w for _, w in made)
    # the file of 30 rows: 2520 bytes of RGBA8, 5040 of RGBA16, 3780 + 30 filtered
    limit = 4000
    for route in (None, "mixed"):
        rgba, rgba_off, _, status, png_status = _p16().png_decode_mixed_files_rgba16_batch(d_file, d_off, d_len, max_bytes=limit, route=route)
        assert png_status.cpu().tolist() == [0, 2, 0, 0]
        off = rgba_off.cpu().tolist()
        assert off[2] == off[1] and rgba.numel() == off[-1] == sum(len(w) for k, (_, w) in enumerate(made) if k != 1)
        assert rgba.cpu().numpy().tobytes() == b"".join(w for k, (_, w) in enumerate(made) if k != 1)
    assert fd.png_decode_mixed_files_rgba_batch(d_file, d_off, d_len, max_bytes=limit)[4].cpu().tolist() == [0] * 4


@pytest.mark.parametrize("colour", DEPTH16)
def test_rgba16_to_files_and_back(colour):
    """Representable pictures of several heights through png_encode_rgba16_files_batch: the files are sound by the
    model's scan, hold the model's packed rows, and png_decode_files_rgba16_batch gives the pictures back; grey-16
    files are Pillow's pictures too.  A picture the pair cannot hold gets status 13 and no file."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(17700 + colour)
    width, heights = 29, (1, 7, 66, 3)
    rb = fm.geometry(width, 16, colour)[0]
    pictures = [_representable(r, width * h, colour) for h in heights]
    if colour != 6:
        spoiled = pictures[3].copy()
        spoiled[2 if colour in (0, 4) else 6] ^= 1        # the low byte of the first pixel's G (grey pairs) or A (RGB)
        pictures[3] = spoiled
        assert m16.pack16(spoiled.tobytes(), width, colour)[1] == 13
    want_st = [0, 0, 0, 13 if colour != 6 else 0]
    s_off = np.concatenate([[0], np.cumsum([p.size for p in pictures])]).astype(np.int64)
    slot = (fd.png_file_bound(max(heights), rb) + 15) & ~15
    f_off = torch.arange(len(pictures) + 1, dtype=torch.int64, device="cuda") * slot
    files = torch.full((len(pictures) * slot + 16,), GUARD, dtype=torch.uint8, device="cuda")
    file_len, st = _p16().png_encode_rgba16_files_batch(gh.dev(np.concatenate(pictures)), gh.dev(s_off), files, f_off, width, colour)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == want_st
    lens, host = file_len.cpu().tolist(), files.cpu().numpy()
    assert (host[len(pictures) * slot:] == GUARD).all()
    for k, (p, h) in enumerate(zip(pictures, heights)):
        if want_st[k]:
            assert lens[k] == 0
            continue
        f = host[k * slot:k * slot + lens[k]].tobytes()
        w, hh, d, c, packed = am.decode(f)
        assert (w, hh, d, c) == (width, h, 16, colour) and bytes(packed) == m16.pack16(p.tobytes(), width, colour)[0], k
        if colour == 0:
            assert np.array_equal(_pillow_grey16(f), p.view("<u2").reshape(h, width, 4)[..., 0])
    rgba, rgba_off, _, status, png_status = _p16().png_decode_files_rgba16_batch(files, f_off, width, 16, colour, file_len=file_len)
    off = rgba_off.cpu().tolist()
    for k, p in enumerate(pictures):
        if want_st[k] == 0:
            assert status[k].item() == 0 and png_status[k].item() == 0
            assert np.array_equal(rgba[off[k]:off[k + 1]].cpu().numpy(), p), k


def test_bench_shape_there_and_back():
    """2048 images of 341 x 64 at the timing tool's shape: RGB16 to RGBA16 equals torch's byte swap through an int16
    view with an alpha plane behind it, RGB8 to RGBA16 equals torch's * 257, and pack16 gives the RGB16 input back."""
    import torch
    n, width, rows = 2048, 341, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(17800)
    pix = torch.randint(0, 256, (n, rows, width, 3, 2), dtype=torch.uint8, device="cuda", generator=g)
    p_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 6)
    r_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 8)
    rgba = torch.empty(n * rows * width * 8, dtype=torch.uint8, device="cuda")
    st = _p16().png_expand16_batch(pix.view(-1), p_off, rgba, r_off, width, 16, 2)
    swapped = pix.flip(-1).contiguous().view(torch.int16).view(n, rows, width, 3)
    want = torch.cat([swapped, torch.full((n, rows, width, 1), -1, dtype=torch.int16, device="cuda")], dim=3)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    assert torch.equal(rgba.view(torch.int16).view(n, rows, width, 4), want)
    back = torch.empty(n * rows * width * 6, dtype=torch.uint8, device="cuda")
    st = _p16().png_pack16_batch(rgba, r_off, back, p_off, width, 2)
    assert int(st.abs().sum()) == 0 and torch.equal(back, pix.view(-1))
    del want, swapped, back
    pix8 = pix[..., 0].contiguous()
    p8_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 3)
    st = _p16().png_expand16_batch(pix8.view(-1), p8_off, rgba, r_off, width, 8, 2)
    want8 = torch.cat([pix8.to(torch.int32) * 257, torch.full((n, rows, width, 1), 65535, dtype=torch.int32, device="cuda")], dim=3)
    assert int(st.abs().sum()) == 0
    assert torch.equal(rgba.view(torch.int16).view(n, rows, width, 4).to(torch.int32) & 0xFFFF, want8)
