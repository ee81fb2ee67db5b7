"""-m gpu: PNG decode to RGBA8 -- fdh_png_expand_batch, fdh_png_colour_batch, png_decode_files_rgba_batch.

Referee: tests/png_expand_model.py (plain integers, pinned to Pillow and to literal bytes by
tests/test_png_expand_model.py); Pillow's own convert("RGBA") once more on the files of the classes where it follows
the specification.  Everything is bit-exact.

png_expand_kernel: grid(n, waves), a wavefront takes the bands b, b + waves, .. of 64 rows of its image and makes
four pixels per lane and step; FDH_PNG_EXPAND_WAVES forces the number of wavefronts per image.
"""
import io
import zlib

import numpy as np
import pytest

import png_corpus as pc
import png_expand_model as em
import png_file_model as fm
import png_gpu_harness as gh
from png_gpu_harness import GUARD, HEIGHTS, PASSED_ON

pytestmark = pytest.mark.gpu


class Batch:
    """Images one behind the other from an odd byte of a buffer of guard bytes, and their output slots with a slot of
    guard bytes between every two (an entry with no pixels that `upstream` marks as failed: its slot must stay as it
    is): 20 bytes behind the first image, 5 behind the others, so that output slots start at every alignment."""

    def __init__(self, images, width, depth, colour, front=3):
        """images: [(pix uint8, key or None, pal or None)]"""
        self.geometry = (width, depth, colour)
        self.n = 2 * len(images)
        p_off, r_off, self.want, self.want_status = [front], [0], [], []
        for k, (pix, key, pal) in enumerate(images):
            rgba, st = em.expand(pix, width, depth, colour, key, pal)
            p_off += [p_off[-1] + pix.size] * 2
            r_off += [r_off[-1] + len(rgba), r_off[-1] + len(rgba) + (20 if k == 0 else 5)]
            self.want.append(np.frombuffer(rgba, dtype=np.uint8))
            self.want_status += [st, PASSED_ON]
        self.p_off, self.r_off = np.asarray(p_off, dtype=np.int64), np.asarray(r_off, dtype=np.int64)
        self.pix = np.full(int(p_off[-1]) + 7, GUARD, dtype=np.uint8)
        for k, (pix, _, _) in enumerate(images):
            self.pix[p_off[2 * k]:p_off[2 * k + 1]] = pix
        self.expect = np.full(int(r_off[-1]) + 64, GUARD, dtype=np.uint8)
        for k, w in enumerate(self.want):
            self.expect[r_off[2 * k]:r_off[2 * k + 1]] = w
        self.upstream = [0, PASSED_ON] * len(images)
        self.pal = self.colour = None
        if colour == 3:
            self.pal = [w for _, _, pal in images for w in (em.pal_words(pal), [0] * 256)]
            self.colour = [w for _, _, pal in images for w in (em.colour_words(len(pal), None), [0] * 4)]
        elif any(key is not None for _, key, _ in images):
            self.colour = [w for _, key, _ in images for w in (em.colour_words(0, key), [0] * 4)]

    def run(self, fd):
        """-> (output buffer, png_status) after one call; the input must not change."""
        import torch
        d_pix = gh.dev(self.pix)
        rgba = torch.full((self.expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        fd.png_expand_batch(d_pix, gh.dev(self.p_off), rgba, gh.dev(self.r_off), *self.geometry,
                            pal=None if self.pal is None else gh.words(self.pal),
                            colour=None if self.colour is None else gh.words(self.colour),
                            upstream=gh.words(self.upstream), png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        assert np.array_equal(d_pix.cpu().numpy(), self.pix)
        st = st.cpu().numpy()
        assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + self.n:] == 0x5A5A5A5A).all()
        return rgba.cpu().numpy(), st[8:8 + self.n].tolist()

    def check(self, fd, what):
        got, st = self.run(fd)
        assert st == self.want_status, what
        if not np.array_equal(got, self.expect):
            at = int(np.nonzero(got != self.expect)[0][0])
            raise AssertionError("%r: byte %d of the output is %d, not %d (slots at %s)" % (what, at, got[at], self.expect[at], self.r_off.tolist()))


# ---- fdh_png_expand_batch ----

@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_expand_every_width_and_height(pair, monkeypatch):
    """Every width of gh.EXPAND_WIDTHS at heights 1, 2, 3 and one more than a band, eight images a call (each height twice, with
    different pixels), with a key / tRNS and without: the output buffer equals the model's byte for byte, guard slots
    and the bytes behind the last slot included, and every status is right.  Each batch runs with one wavefront per
    image (a wavefront takes two bands), with seven (more wavefronts than bands) and with the default."""
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(7500 + 64 * colour + depth)
    for keyed in (False, True):
        if keyed and colour in (4, 6):
            continue                    # (no key and no tRNS in these)
        for width in gh.EXPAND_WIDTHS:
            images = [pc.random_case(r, width, h, depth, colour, keyed) for h in HEIGHTS + HEIGHTS]
            b = Batch(images, width, depth, colour)
            if keyed and colour != 3:
                assert all(0 in w[3::4] for w in b.want)
            for waves in (1, 7, None):
                gh.set_env(monkeypatch, FDH_PNG_EXPAND_WAVES=waves)
                b.check(fd, (pair, keyed, width, waves))


@pytest.mark.parametrize("depth", (1, 2, 4, 8))
def test_palette_sizes_and_an_index_outside(depth, monkeypatch):
    """Palettes of 1, 2 and 2^depth entries whose images stay inside them, and one of 2^depth - 1 entries whose image
    holds the last index: that image gets status 9, its pixels are the model's ((0, 0, 0, 255) at that index), and its
    neighbours get 0."""
    import fdeflate_amd as fd
    r = np.random.default_rng(7600 + depth)
    top = 1 << depth
    for width in (5, 33, 257):
        rb = fm.geometry(width, depth, 3)[0]
        images = []
        for entries, outside in ((1, False), (2, False), (top, False), (top - 1, True), (top, False)):
            rows = 3
            idx = r.integers(0, top if outside else entries, (rows, width))
            if outside:
                idx[1, width // 2] = top - 1                   # the last index is present
            bits = np.zeros((rows, rb * 8), dtype=np.uint8)
            for k in range(depth):
                bits[:, k:width * depth:depth] = (idx >> (depth - 1 - k)) & 1
            pad = r.integers(0, 2, (rows, rb * 8 - width * depth), dtype=np.uint8)      # padding bits: ignored
            bits[:, width * depth:] = pad
            pix = np.packbits(bits, axis=1).reshape(-1)
            assert em.samples(pix[:rb].tobytes(), width, depth, 1) == idx[0].tolist()
            pal = em.palette(r.integers(0, 256, 3 * entries, dtype=np.uint8).tobytes(), r.integers(0, 256, entries, dtype=np.uint8).tobytes())
            images.append((pix, None, pal))
        b = Batch(images, width, depth, 3)
        assert b.want_status[0::2] == [0, 0, 0, 9, 0]
        for waves in (None, 1):
            gh.set_env(monkeypatch, FDH_PNG_EXPAND_WAVES=waves)
            b.check(fd, (depth, width, waves))


def test_slots_that_do_not_fit_and_upstream():
    """A pixel slot of rows and a half, an output slot one pixel short and one pixel long: status 2 and no byte changes.
    upstream != 0: that value is the status and the slot is untouched.  An empty pixel slot with an empty output slot:
    status 0.  The images in between are exact."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(7700)
    for (depth, colour), width in (((8, 2), 21), ((1, 0), 21), ((8, 3), 70), ((16, 6), 9)):
        rb = fm.geometry(width, depth, colour)[0]
        rows = 4
        pal = em.palette(bytes(range(256)) * 3) if colour == 3 else None
        # (pixel bytes, output bytes, upstream, expected status)
        full, out = rows * rb, rows * width * 4
        plan = [(full, out, 0, 0), (full + rb // 2 + 1, out + width * 4, 0, 2), (full, out, 0, 0), (full, out - 4, 0, 2),
                (full, out + 4, 0, 2), (0, 0, 0, 0), (full, out, 5, 5), (full, out, 0, 0), (full, out, 0x80000003, 0x80000003),
                (0, 8, 0, 2), (rb, 0, 0, 2), (full, out, 0, 0)]
        p_off = np.concatenate([[1], 1 + np.cumsum([p[0] for p in plan])]).astype(np.int64)
        r_off = np.concatenate([[4], 4 + np.cumsum([p[1] for p in plan])]).astype(np.int64)
        pix = r.integers(0, 256, int(p_off[-1]) + 3, dtype=np.uint8)
        expect = np.full(int(r_off[-1]) + 32, GUARD, dtype=np.uint8)
        for k, (pb, ob, up, want) in enumerate(plan):
            if want == 0 and pb:
                rgba, st = em.expand(pix[p_off[k]:p_off[k + 1]], width, depth, colour, None, pal)
                assert st == 0
                expect[r_off[k]:r_off[k + 1]] = np.frombuffer(rgba, dtype=np.uint8)
        rgba = torch.full((expect.size,), GUARD, dtype=torch.uint8, device="cuda")
        n = len(plan)
        st = fd.png_expand_batch(gh.dev(pix), gh.dev(p_off), rgba, gh.dev(r_off), width, depth, colour,
                                 pal=gh.words([em.pal_words(pal)] * n) if pal else None,
                                 colour=gh.words([em.colour_words(256, None)] * n) if pal else None,
                                 upstream=gh.words([p[2] for p in plan]))
        torch.cuda.synchronize()
        assert st.cpu().numpy().view(np.uint32).tolist() == [p[3] for p in plan], (depth, colour)
        assert np.array_equal(rgba.cpu().numpy(), expect), (depth, colour)
        # without upstream: the two entries that were passed on are images like the others
        st = fd.png_expand_batch(gh.dev(pix), gh.dev(p_off), rgba, gh.dev(r_off), width, depth, colour,
                                 pal=gh.words([em.pal_words(pal)] * n) if pal else None)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0 if p[2] else p[3] for p in plan]
        got = rgba.cpu().numpy()
        for k in (6, 8):
            assert got[r_off[k]:r_off[k + 1]].tobytes() == em.expand(pix[p_off[k]:p_off[k + 1]], width, depth, colour, None, pal)[0]


def test_more_images_than_wavefronts_fill():
    """5000 images of 3 x 7 two-bit palette pixels and of 2 x 5 sixteen-bit grey + alpha pixels in one call each (one
    wavefront per image; rows of a few pixels share a step), against the model."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(7800)
    n = 5000
    for (depth, colour), width, rows in (((2, 3), 7, 3), ((16, 4), 5, 2), ((1, 0), 3, 5)):
        rb = fm.geometry(width, depth, colour)[0]
        pix = r.integers(0, 256, n * rows * rb + 1, dtype=np.uint8)
        pal = em.palette(r.integers(0, 256, 9, dtype=np.uint8).tobytes(), b"\x07") if colour == 3 else None
        p_off = 1 + np.arange(n + 1, dtype=np.int64) * (rows * rb)
        r_off = np.arange(n + 1, dtype=np.int64) * (rows * width * 4)
        want, want_st = em.expand(pix[1:], width, depth, colour, None, pal)     # (whole rows: the images one below the other)
        per = [em.expand(pix[p_off[k]:p_off[k + 1]], width, depth, colour, None, pal)[1] for k in range(n)]
        assert (want_st == 9) == (colour == 3) and (colour != 3 or 0 in per)
        rgba = torch.full((int(r_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
        st = fd.png_expand_batch(gh.dev(pix), gh.dev(p_off), rgba, gh.dev(r_off), width, depth, colour,
                                 pal=gh.words([em.pal_words(pal)] * n) if pal else None,
                                 colour=gh.words([em.colour_words(3, None)] * n) if pal else None)
        torch.cuda.synchronize()
        got = rgba.cpu().numpy()
        assert st.cpu().tolist() == per
        assert got[:int(r_off[-1])].tobytes() == want and (got[int(r_off[-1]):] == GUARD).all()


# ---- fdh_png_colour_batch ----

def test_colour_batch_every_status():
    """The files of png_corpus.status_files in one batch, read with every geometry that occurs among them:
    each file gets the model's status (0, 3, 7, 10, 11 all occur), and on the sound ones `pal` and `colour` are the
    model's word for word.  Nothing outside the result arrays is written."""
    import torch
    import fdeflate_amd as fd
    cases = pc.status_files()
    files = [c[1] for c in cases]
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off = gh.dev(host), gh.dev(f_off)
    info = fd.png_scan_files_batch(d_file, d_off, gh.dev(f_len))
    model_info = [fm.scan(f, crc=zlib.crc32) for f in files]
    n, seen, sound = len(files), set(), 0
    for call in sorted({c[2] for c in cases}):
        width, depth, colour = call
        pal = torch.full((n + 2, 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        col = torch.full((n + 2, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        st = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        fd.png_colour_batch(d_file, d_off, info, width, depth, colour, pal=pal[1:n + 1] if colour == 3 else None, colour=col[1:n + 1],
                            png_status=st[1:n + 1])
        torch.cuda.synchronize()
        pal, col, st = (t.cpu().numpy().view(np.uint32) for t in (pal, col, st))
        for t in (pal, col, st):
            assert (t[0] == 0x5A5A5A5A).all() and (t[n + 1] == 0x5A5A5A5A).all()
        for k, (what, f, own, want, _) in enumerate(cases):
            m_st, m_pal, m_key = em.read_colour(f, model_info[k], width, depth, colour)
            assert st[k + 1] == m_st, (call, what)
            if own == call:
                assert m_st == want, what
                seen.add(m_st)
            if m_st == 0:
                sound += 1
                assert col[k + 1].tolist() == em.colour_words(len(m_pal) if m_pal else 0, m_key), (call, what)
                if colour == 3:
                    assert pal[k + 1].tolist() == em.pal_words(m_pal), (call, what)
        if colour != 3:
            assert (pal == 0x5A5A5A5A).all()
    assert seen == {0, 3, 7, 10, 11} and sound >= 10
    assert np.array_equal(d_file.cpu().numpy(), host)


# ---- files -> RGBA ----

def _model_rgba(png, width, depth, colour):
    """The model's whole path on one file: scan, zlib, reconstruction (every row has filter type 0 or is Pillow's: the
    packed scanlines come from the caller for those), read_colour, expand."""
    info = fm.scan(png, crc=zlib.crc32)
    st, pal, key = em.read_colour(png, info, width, depth, colour)
    assert info.status == 0 and st == 0
    return info, pal, key


PILLOW_MODES = {(8, 3): "P", (8, 0): "L", (8, 2): "RGB", (8, 6): "RGBA", (8, 4): "LA", (1, 0): "1"}
END_TO_END = ((8, 3, True), (2, 3, True), (8, 0, True), (4, 0, True), (1, 0, False), (8, 2, True), (16, 2, True), (8, 4, False),
              (8, 6, False), (16, 0, True))


@pytest.mark.parametrize("cls", END_TO_END, ids=["depth%d-colour%d" % c[:2] for c in END_TO_END])
def test_files_to_rgba(cls):
    """Model-written files (a tEXt in front, PLTE, tRNS, the stream in three IDAT chunks) of two heights and, where
    Pillow has a mode for the class, a file that Image.save wrote, one batch per class through
    png_decode_files_rgba_batch: every picture equals the model's, the Pillow-written one and -- on the classes where
    Pillow follows the specification -- the model-written ones equal Pillow's convert("RGBA") as well."""
    import torch
    import fdeflate_amd as fd
    depth, colour, keyed = cls
    r = np.random.default_rng(7900 + 64 * colour + depth)
    width = 37
    rb = fm.geometry(width, depth, colour)[0]
    files, want, heights = [], [], []
    for height in (3, 70):
        pix, key, pal = pc.random_case(r, width, height, depth, colour, keyed)
        files.append(em.write_file(pc.stream_of(pix, rb), width, height, depth, colour, pc.pre_chunks(colour, key, pal, text=True), 3, zlib.crc32))
        rgba = em.expand(pix, width, depth, colour, key, pal)[0]
        if (depth, colour) not in pc.LEFT_OUT:
            assert pc.pillow_rgba(files[-1]) == rgba
        want.append(rgba)
        heights.append(height)
    mode = PILLOW_MODES.get((depth, colour))
    if mode:
        height = 41
        im = pc.corpus_image(r, mode, width, height)
        buf = io.BytesIO()
        im.save(buf, format="PNG")
        png = buf.getvalue()
        info, pal, key = _model_rgba(png, width, depth, colour)
        assert (info.width, info.height) == (width, height)
        rgba = em.expand(pc.packed_scanlines(im), width, depth, colour, key, pal)[0]
        assert rgba == im.convert("RGBA").tobytes()
        files.append(png)
        want.append(rgba)
        heights.append(height)
    host, f_off, f_len = gh.batch_of(files)
    for with_len in (True, False):
        rgba, rgba_off, info, status, png_status = fd.png_decode_files_rgba_batch(gh.dev(host), gh.dev(f_off), width, depth, colour,
                                                                                 file_len=gh.dev(f_len) if with_len else None)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * len(files) and png_status.cpu().tolist() == [0] * len(files)
        off = rgba_off.cpu().tolist()
        assert off == np.concatenate([[0], np.cumsum([h * width * 4 for h in heights])]).tolist() and rgba.numel() == off[-1]
        for k, w in enumerate(want):
            picture = rgba[off[k]:off[k + 1]].view(heights[k], width, 4)
            assert picture.cpu().numpy().tobytes() == w, (cls, k)


def test_files_to_rgba_each_failure_has_its_status():
    """One batch of palette files: sound ones between a file with a damaged CRC field (3), no PLTE (10), a tRNS longer
    than the PLTE (11), a damaged zlib stream with sound CRCs (3 from the decoder, `status` not 0), another geometry (7)
    and an index outside the palette (9, written in full).  Every other picture is exact and the failed files' slots
    are empty."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(8000)
    width, height, depth, colour = 45, 9, 4, 3
    rb = fm.geometry(width, depth, colour)[0]
    pal = em.palette(r.integers(0, 256, 48, dtype=np.uint8).tobytes(), r.integers(0, 256, 10, dtype=np.uint8).tobytes())
    plte, trns = (b"PLTE", em.plte_body(pal)), (b"tRNS", bytes(e[3] for e in pal[:10]))

    def sound(pre=(plte, trns), idat=None, d=depth, c=colour):
        pix = r.integers(0, 256, height * fm.geometry(width, d, c)[0], dtype=np.uint8)
        return pix, em.write_file(idat or pc.stream_of(pix, fm.geometry(width, d, c)[0]), width, height, d, c, list(pre), 2, zlib.crc32)

    good = [sound() for _ in range(7)]
    crc = bytearray(good[0][1])
    crc[45] ^= 1                                                  # a byte of the PLTE's body: its CRC no longer fits
    stream = bytearray(pc.stream_of(good[0][0], rb))
    stream[len(stream) // 2] ^= 0x55
    stream[0] = 0x79                                              # (and a zlib header that cannot be)
    short_pal = em.palette(em.plte_body(pal[:15]))
    pix9 = np.full(height * rb, 0xFE, dtype=np.uint8)             # indices 15 and 14
    files = [good[0][1], bytes(crc), good[1][1], sound(pre=())[1], good[2][1], sound(pre=(plte, (b"tRNS", bytes(17))))[1], good[3][1],
             sound(idat=bytes(stream))[1], good[4][1], sound(d=8)[1], good[5][1],
             em.write_file(pc.stream_of(pix9, rb), width, height, depth, colour, [(b"PLTE", em.plte_body(short_pal))], 1, zlib.crc32), good[6][1]]
    want_st = [0, 3, 0, 10, 0, 11, 0, 3, 0, 7, 0, 9, 0]
    host, f_off, f_len = gh.batch_of(files)
    rgba, rgba_off, info, status, png_status = fd.png_decode_files_rgba_batch(gh.dev(host), gh.dev(f_off), width, depth, colour, file_len=gh.dev(f_len))
    torch.cuda.synchronize()
    assert png_status.cpu().tolist() == want_st
    assert status[7].item() != 0 and [status[k].item() for k in (0, 2, 4, 6, 8, 10, 11, 12)] == [0] * 8
    assert info[:, 0].cpu().tolist() == [6 if k == 1 else 0 for k in range(len(files))]
    off = rgba_off.cpu().tolist()
    got = rgba.cpu().numpy()
    size = height * width * 4
    for k, st in enumerate(want_st):
        assert off[k + 1] - off[k] == (0 if k in (1, 9) else size), k       # (skipped by the read-back: empty; the others have a slot)
    for k, g in zip((0, 2, 4, 6, 8, 10, 12), good):
        assert got[off[k]:off[k + 1]].tobytes() == em.expand(g[0], width, depth, colour, None, pal)[0], k
    want9, st9 = em.expand(pix9, width, depth, colour, None, short_pal)
    assert st9 == 9 and got[off[11]:off[12]].tobytes() == want9 and want9[:8] == bytes([0, 0, 0, 255]) + bytes(short_pal[14])


def test_bench_shape_there_and_back():
    """4096 images of 341 x 64 RGB8: the kernel's output equals torch.cat with an alpha plane, and dropping the alpha
    gives the input back."""
    import torch
    import fdeflate_amd as fd
    n, width, rows = 4096, 341, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(8100)
    pix = torch.randint(0, 256, (n, rows, width, 3), dtype=torch.uint8, device="cuda", generator=g)
    p_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 3)
    r_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 4)
    rgba = torch.empty(n * rows * width * 4, dtype=torch.uint8, device="cuda")
    st = fd.png_expand_batch(pix.view(-1), p_off, rgba, r_off, width, 8, 2)
    want = torch.cat([pix, torch.full((n, rows, width, 1), 255, dtype=torch.uint8, device="cuda")], dim=3)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    got = rgba.view(n, rows, width, 4)
    assert torch.equal(got, want)
    assert torch.equal(got[..., :3].contiguous(), pix)
