"""-m gpu: fdh_png_choose_filters_batch (the per-row filter types, chosen on the GPU) and
png_encode_ultrafast_batch (choose, then filter + ultra-fast encode).

The referee for the choice is tests/png_choose_model.py -- the PNG specification's minimum sum of
absolute values, lowest type number on a tie, in plain integers --, which tests/test_png_choose_model.py
pins against the oracle's filtered bytes.  Pillow is no referee for the choice (its encoder follows
another rule); it only decodes a finished stream at the end.  Everything is bit-exact.

png_choose_kernel gives a row a group of G lanes (a power of two), 64 / G rows of a band of 64 rows
to a wavefront step, and loops along rows of more than 16 G bytes.  By default G is the row's chunk
count rounded up to a power of two (64 at most): narrow-row groups up to 512 bytes, one step per row
up to 1024, looped rows above.  FDH_PNG_CHOOSE_LANES forces G (so every shape, and every
combination -- looped groups, one step with idle lanes -- runs at the widths of the subset);
FDH_PNG_CHOOSE_WAVES sets how many wavefronts share an image's bands (one: a wavefront walks every
band; three: bands b, b + 3, ..).  Types slots sit at odd offsets with odd slack in a buffer of fill
bytes that is compared as a whole; the pixel buffer starts at an odd offset, so rows are unaligned.
"""
import io
import struct
import time
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_choose_model as cm
import png_gpu_harness as gh
import png_model

pytestmark = pytest.mark.gpu

BPPS = (1, 2, 3, 4, 6, 8)
EXTRA_CHUNKS = (4, 32)                      # the default choice's G = 4 and G = 32 (N = 3..4 and 17..32)
SUBSET_CHUNKS = (1, 9, 64, 65, 256)         # the forced shapes
GATE = 4096
FILL = 0xEE
ENV = ("FDH_PNG_CHOOSE_LANES", "FDH_PNG_CHOOSE_WAVES")


def _shape(monkeypatch, lanes=None, waves=None):
    gh.set_env(monkeypatch, **dict(zip(ENV, (lanes, waves))))


class Batch:
    """Images of one (row_bytes, bpp) with the model's types.  Pixels are packed back to back from
    byte 3 of their buffer.  The ABI has ONE offsets array and insists that slot i =
    [types_off[i], types_off[i + 1]) is exactly image i's row count, so inside one call the slots are
    contiguous: they start 7 bytes into a buffer of fill bytes, odd row counts put the later ones at
    odd offsets, and 33 fill bytes follow the last one.  (Slack BETWEEN slots:
    test_slack_between_types_slots.)  `want` is the expected image of the whole buffer."""

    def __init__(self, imgs, bpp):
        self.bpp, self.n = bpp, len(imgs)
        self.rb = imgs[0].shape[1]
        self.imgs = imgs
        self.rows = [im.shape[0] for im in imgs]
        self.types, self.sums = zip(*(cm.choose(im, bpp) for im in imgs))
        self.p_off = gh.offsets([im.size for im in imgs], 3, [0] * self.n)
        self.pix = np.zeros(int(self.p_off[-1]) + 5, dtype=np.uint8)
        for o, im in zip(self.p_off[:-1], imgs):
            self.pix[int(o):int(o) + im.size] = im.reshape(-1)
        self.t_off = gh.offsets(self.rows, 7, [0] * self.n)
        self.want = np.full(int(self.t_off[-1]) + 33, FILL, dtype=np.uint8)
        for o, t in zip(self.t_off[:-1], self.types):
            self.want[int(o):int(o) + t.size] = t


def _run(fd, b, faults, what, status=None):
    import torch
    d_t = torch.full((b.want.size,), FILL, dtype=torch.uint8, device="cuda")
    st = fd.png_choose_filters_batch(gh.dev(b.pix), gh.dev(b.p_off), d_t, gh.dev(b.t_off), b.rb, b.bpp)
    torch.cuda.synchronize()
    got = d_t.cpu().numpy()
    if st.cpu().tolist() != (status or [0] * b.n):
        faults.append((what, "status", st.cpu().tolist()))
    if not np.array_equal(got, b.want):
        at = int(np.nonzero(got != b.want)[0][0])
        slot = int(np.searchsorted(b.t_off, at, side="right")) - 1
        row = at - int(b.t_off[slot]) if 0 <= slot < b.n else -1
        sums = b.sums[slot][:, row].tolist() if 0 <= slot < b.n and 0 <= row < b.rows[slot] else None
        faults.append((what, "byte %d: image %d (%d rows) row %d, got %d, want %d, sums %s" % (at, slot, b.rows[slot] if 0 <= slot < b.n else -1, row, int(got[at]), int(b.want[at]), sums)))


def test_slack_between_types_slots():
    """Types slots at odd offsets with odd slack between them, in one buffer of fill bytes that is
    compared as a whole.  The slots of ONE call are contiguous by the ABI (slot i =
    [types_off[i], types_off[i + 1]) must be exactly the row count), so every image is a call of its
    own into the shared buffer; its pixels start at byte 1 of theirs."""
    import torch
    import fdeflate_amd as fd
    bpp, rb = 3, 93
    r = np.random.default_rng(4700)
    imgs = cm.choose_images(r, rb, bpp)
    # every image alone, at its own odd offset with odd slack behind it, in one shared buffer
    t_at = gh.offsets([im.shape[0] for im in imgs], 9, [2 * (i % 5) + 1 for i in range(len(imgs))])
    want = np.full(int(t_at[-1]) + 33, FILL, dtype=np.uint8)
    d_t = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
    for i, im in enumerate(imgs):
        types, _ = cm.choose(im, bpp)
        want[int(t_at[i]):int(t_at[i]) + types.size] = types
        pix = np.concatenate([np.zeros(1, dtype=np.uint8), im.reshape(-1)])
        st = fd.png_choose_filters_batch(gh.dev(pix), gh.dev(np.array([1, 1 + im.size], dtype=np.int64)), d_t,
                                         gh.dev(np.array([t_at[i], t_at[i] + im.shape[0]], dtype=np.int64)), rb, bpp)
        assert st.cpu().tolist() == [0]
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy(), want)


@pytest.mark.parametrize("bpp", BPPS)
def test_types_at_every_width_class(bpp, monkeypatch):
    """Every width class x 13 ragged images (0 .. 200 rows, every kind of png_choose_model.KINDS in
    turn) against the model, by the default choice of shape and with one and three wavefronts per
    image: every width.  G forced to 1, 4, 16, 32 and 64 lanes per row: the widths of N in
    {1, 9, 64, 65, 256} and the three widths above 4096.  The coverage the comparison relies on is
    asserted over exactly these images: every type chosen, one row in ten (at least) tied."""
    import torch
    import fdeflate_amd as fd
    assert torch.cuda.is_available()
    t0 = time.time()
    r = np.random.default_rng(4600 + bpp)
    widths = [(n, w) for n in gh.CHUNKS + EXTRA_CHUNKS for w in sorted(set(gh.widths_of(bpp, n)))] + [(0, w) for w in gh.widths_above(bpp, GATE)]
    faults, runs = [], 0
    count, ties, total = np.zeros(5, dtype=np.int64), 0, 0
    for k, (n, rb) in enumerate(widths):
        b = Batch(cm.choose_images(r, rb, bpp, shift=k), bpp)
        for t, s in zip(b.types, b.sums):
            count += np.bincount(t, minlength=5)
            ties += int(cm.tied(s).sum())
            total += t.size
        for waves in (None, 1, 3):
            _shape(monkeypatch, waves=waves)
            _run(fd, b, faults, (bpp, rb, "default lanes", "waves", waves))
            runs += 1
        if n == 0 or n in SUBSET_CHUNKS:
            for lanes in (1, 4, 16, 32, 64):
                _shape(monkeypatch, lanes=lanes, waves=2)
                _run(fd, b, faults, (bpp, rb, "lanes", lanes))
                runs += 1
        _shape(monkeypatch)
    print("bpp %d: %d widths, %d kernel runs, %d rows (%s per type, %d tied), %.1f s" % (bpp, len(widths), runs, total, count.tolist(), ties, time.time() - t0))
    assert (count > 0).all() and 10 * ties >= total, (count.tolist(), ties, total)
    assert not faults, "%d runs differ, at row widths %s; the first ones: %s" % (len(faults), sorted({f[0][1] for f in faults}), faults[:12])


@pytest.mark.parametrize("bpp", (1, 3, 8))
def test_sizes_that_do_not_fit(bpp, monkeypatch):
    """Status 2 and an untouched types slot for: a pixel slot one byte short of whole rows; a types
    slot one too long; one too short.  The neighbours stay exact.  At a narrow, a one-step and a looped width."""
    import torch
    import fdeflate_amd as fd
    _shape(monkeypatch)
    r = np.random.default_rng(4800 + bpp)
    for rb in (24 // bpp * bpp, 1016 // bpp * bpp, 1536):
        rows = (5, 70, 3, 64, 9)
        imgs = cm.choose_images(r, rb, bpp, rows=rows, shift=rb)
        types = [cm.choose(im, bpp)[0] for im in imgs]
        for case in ("pixels short", "types long", "types short"):
            bad = 1 if case == "pixels short" else 3
            psize = [im.size for im in imgs]
            tsize = list(rows)
            if case == "pixels short":
                psize[bad] -= 1
                tsize[bad] -= 1           # exactly the whole rows the short slot holds: only the pixel slot is at fault
            elif case == "types long":
                tsize[bad] += 1
            else:
                tsize[bad] -= 1
            p_off, t_off = gh.offsets(psize, 3, [0] * 5), gh.offsets(tsize, 7, [0] * 5)
            pix = np.zeros(int(p_off[-1]) + 16, dtype=np.uint8)
            want = np.full(int(t_off[-1]) + 33, FILL, dtype=np.uint8)
            for i, im in enumerate(imgs):
                pix[int(p_off[i]):int(p_off[i]) + psize[i]] = im.reshape(-1)[:psize[i]]
                if i != bad:
                    want[int(t_off[i]):int(t_off[i]) + rows[i]] = types[i]
            d_t = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
            st = fd.png_choose_filters_batch(gh.dev(pix), gh.dev(p_off), d_t, gh.dev(t_off), rb, bpp)
            torch.cuda.synchronize()
            assert st.cpu().tolist() == [2 if i == bad else 0 for i in range(5)], (bpp, rb, case, st.cpu().tolist())
            assert np.array_equal(d_t.cpu().numpy(), want), (bpp, rb, case)


def test_refused_arguments():
    """row_bytes == 0, a bpp outside 1, 2, 3, 4, 6, 8 and row_bytes >= 2^25: FDH_ERR_INVALID_ARGUMENT and a message,
    nothing launched; 2^25 - 1 is accepted."""
    import ctypes as C
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import _lib
    pix = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = gh.dev(np.array([0, 0], dtype=np.int64))
    types = torch.full((8,), FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(rb, bpp):
        return L.fdh_png_choose_filters_batch(C.c_void_p(pix.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(types.data_ptr()),
                                              C.c_void_p(off.data_ptr()), C.c_void_p(st.data_ptr()), 1, rb, bpp, None)
    for rb, bpp, word in ((0, 3, b"row_bytes"), (48, 5, b"bpp"), (48, 0, b"bpp"), (48, 7, b"bpp"), (1 << 25, 4, b"2^25"), (0xFFFFFFFF, 1, b"2^25")):
        assert call(rb, bpp) == 1, (rb, bpp)          # FDH_ERR_INVALID_ARGUMENT
        assert word in L.fdh_last_error(), (rb, bpp, L.fdh_last_error())
        with pytest.raises(_lib.FdeflateHipError):
            fd.png_choose_filters_batch(pix, off, types, off, rb, bpp, st)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [77] and types.cpu().tolist() == [FILL] * 8
    assert call((1 << 25) - 1, 4) == 0                # an image of 0 rows of the widest row there is
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] and types.cpu().tolist() == [FILL] * 8


def _png_container(idat, width, height, bpp):
    """Signature, IHDR, one IDAT, IEND: 8-bit grey, grey + alpha, RGB, RGBA for bpp 1, 2, 3, 4."""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    colour = {1: 0, 2: 4, 3: 2, 4: 6}[bpp]
    ihdr = struct.pack(">IIBBBBB", width, height, 8, colour, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


@pytest.mark.parametrize("bpp", BPPS)
def test_pixels_to_idat_end_to_end(bpp, monkeypatch):
    """png_encode_ultrafast_batch on 240 images of every kind, 1 .. 40 rows of 8 .. 87 pixels, once with
    the types buffer left to the call and once with the caller's: the types are the model's, every
    stream is compress_ultra_fast(png_filter(pixels, model's types)) of the oracle bit for bit,
    zlib.decompress + png_model.unfilter give the pixels back, and (where Pillow imports, bpp 1 .. 4)
    Pillow decodes a stream wrapped in a PNG container to the same pixels."""
    import torch
    import fdeflate_amd as fd
    _shape(monkeypatch)
    t0 = time.time()
    r = np.random.default_rng(4900 + bpp)
    n = 240
    rb = int(r.integers(8, 88)) * bpp
    rows = [int(v) for v in r.integers(1, 41, n)]
    imgs = [cm.image(r, cm.KINDS[i % len(cm.KINDS)], nr, rb, bpp) for i, nr in enumerate(rows)]
    types = [cm.choose(im, bpp)[0] for im in imgs]
    filt, want = [], []
    for im, t in zip(imgs, types):
        st, f = ob.png_filter(im.reshape(-1), rb, bpp, t)
        assert st == 0
        filt.append(f)
        want.append(ob.compress_ultra_fast(f))
    p_off = gh.offsets([im.size for im in imgs], 3, [0] * n)
    pix = np.zeros(int(p_off[-1]) + 1, dtype=np.uint8)
    for o, im in zip(p_off[:-1], imgs):
        pix[int(o):int(o) + im.size] = im.reshape(-1)
    caps = [int(fd.ultrafast_bound(nr * (rb + 1))) for nr in rows]
    o_off = gh.offsets(caps, 7, [2 * (i % 4) + 1 for i in range(n)])
    expect = np.full(int(o_off[-1]) + 33, FILL, dtype=np.uint8)
    for o, w in zip(o_off[:-1], want):
        expect[int(o):int(o) + len(w)] = np.frombuffer(w, dtype=np.uint8)
    all_types = np.concatenate(types)
    d_pix, d_poff, d_ooff = gh.dev(pix), gh.dev(p_off), gh.dev(o_off)
    for own in (False, True):
        d_out = torch.full((expect.size,), FILL, dtype=torch.uint8, device="cuda")
        if own:
            t_off = gh.offsets(rows, 5, [0] * n)
            d_types = torch.full((int(t_off[-1]) + 9,), FILL, dtype=torch.uint8, device="cuda")
            ol, st, ty = fd.png_encode_ultrafast_batch(d_pix, d_poff, d_out, d_ooff, rb, bpp, types=d_types, types_off=gh.dev(t_off))
            assert ty is d_types
            got_t = ty.cpu().numpy()
            assert (got_t[:5] == FILL).all() and (got_t[int(t_off[-1]):] == FILL).all()
            got_t = got_t[5:int(t_off[-1])]
        else:
            ol, st, ty = fd.png_encode_ultrafast_batch(d_pix, d_poff, d_out, d_ooff, rb, bpp)
            got_t = ty.cpu().numpy()
            assert ty.dtype == torch.uint8 and got_t.size == all_types.size
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n
        assert np.array_equal(got_t, all_types), (bpp, rb, own, int(np.nonzero(got_t != all_types)[0][0]))
        assert ol.cpu().tolist() == [len(w) for w in want]
        assert np.array_equal(d_out.cpu().numpy(), expect), (bpp, rb, own)
    got = d_out.cpu().numpy()
    for i in range(n):
        stream = got[int(o_off[i]):int(o_off[i]) + len(want[i])].tobytes()
        f = zlib.decompress(stream)
        assert f == filt[i]
        assert png_model.unfilter(f, rb, bpp) == imgs[i].tobytes(), i
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and bpp <= 4:
        i = int(np.argmax(rows))
        stream = got[int(o_off[i]):int(o_off[i]) + len(want[i])].tobytes()
        im = Image.open(io.BytesIO(_png_container(stream, rb // bpp, rows[i], bpp)))
        im.load()
        assert im.size == (rb // bpp, rows[i]) and im.tobytes() == imgs[i].tobytes()
    print("bpp %d, %d-byte rows: %.1f s%s" % (bpp, rb, time.time() - t0, "" if Image is not None else " (no Pillow)"))


def test_the_bench_shape_against_the_model_and_against_torch(monkeypatch):
    """65 536 images x 64 rows x 1023 bytes, bpp 3, the pixels bench.py's streams reconstruct to.  Types
    against the model on 64 images (every 1024th, from image 5), and on ALL images against a second
    GPU computation that shares no code with the kernel: fd.png_filter_batch with each constant type,
    then torch integer arithmetic on the filtered bytes (cost, row sums, first minimum)."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import synth
    _shape(monkeypatch)
    t0 = time.time()
    dev = "cuda"
    n, L, bpp = 65536, 65536, 3
    rb, rows = synth.ROW_BYTES - 1, L // synth.ROW_BYTES
    assert (rb, rows) == (1023, 64)
    buf = synth.gen_batch_torch(0, n, L, model="D", device=dev).view(-1)     # filtered images; later the filter output
    f_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    p_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (rows * rb)
    t_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * rows
    pix = torch.empty(n * rows * rb, dtype=torch.uint8, device=dev)
    assert int(fd.png_unfilter_batch(buf, f_off, pix, p_off, rb, bpp).abs().sum()) == 0
    types = torch.full((n * rows,), FILL, dtype=torch.uint8, device=dev)
    st = fd.png_choose_filters_batch(pix, p_off, types, t_off, rb, bpp)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(types.max()) <= 4
    # the model on a strided sample
    for i in range(5, n, 1024):
        want, sums = cm.choose(pix[i * rows * rb:(i + 1) * rows * rb].cpu().numpy().reshape(rows, rb), bpp)
        got = types[i * rows:(i + 1) * rows].cpu().numpy()
        assert np.array_equal(got, want), (i, int(np.nonzero(got != want)[0][0]), sums[:, int(np.nonzero(got != want)[0][0])].tolist())
    # every image: filter with each constant type, sum the costs with torch
    sums = torch.empty((5, n, rows), dtype=torch.int32, device=dev)
    step = 2048
    for t in range(5):
        const = torch.full((n * rows,), t, dtype=torch.uint8, device=dev)
        assert int(fd.png_filter_batch(pix, p_off, const, t_off, buf, f_off, rb, bpp).abs().sum()) == 0
        f = buf.view(n, rows, rb + 1)
        assert bool((f[:, :, 0] == t).all())
        for i in range(0, n, step):
            v = f[i:i + step, :, 1:].to(torch.int32)
            sums[t, i:i + step] = torch.where(v < 128, v, 256 - v).sum(dim=2, dtype=torch.int32)
    best = torch.zeros((n, rows), dtype=torch.uint8, device=dev)
    least = sums[0].clone()
    for t in range(1, 5):
        better = sums[t] < least
        best[better] = t
        least = torch.minimum(least, sums[t])
    same = best.view(-1) == types
    hist = torch.bincount(types.to(torch.int64), minlength=5).cpu().tolist()
    print("bench shape: types %s, %.1f s" % (hist, time.time() - t0))
    assert bool(same.all()), (int((~same).sum()), int((~same).nonzero()[0]))
