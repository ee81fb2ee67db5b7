"""-m gpu: the PNG kernels at the row widths real images have, and every predictor input there is.

png_pipe_kernel (reconstruction, rows up to 4 KiB) walks a row in N 16-byte chunks with a row period
P = max(N rounded up to 8, 64); the lane-63 -> lane-0 row buffer, the parity of its double-buffered
input lines, the owner arithmetic of its transposed stores and its step bound all depend on P, and
P > 64 means rows of 1025..4096 bytes: a 512-pixel RGB row, a 1366-pixel RGB row, a 1024-pixel RGBA
row.  Rows above 4 KiB go to png_wave_kernel; FDH_PNG_LANE_PER_IMAGE=1 selects png_filter_kernel.
The widths below take every one of them through partial and full last chunks on both sides of every
multiple of eight chunks, up to the pipeline's last width and across the gate.

Everything is bit-exact.  The expectation is the oracle (oracle/fdeflate_oracle.c), which
tests/test_oracle_png.py pins against Pillow and against tests/png_model.py; the exhaustive test uses
png_model directly (2^24 predictions in numpy) and checks it against the oracle on a sample.
Destination slots are looser than their images by an odd number of bytes, start at odd offsets and
lie in a buffer of fill bytes: a whole-buffer comparison shows any byte written outside an image.
"""
import time
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_gpu_harness as gh
import png_model
import streams

pytestmark = pytest.mark.gpu

BPPS = (1, 2, 3, 4, 6, 8)
PIPE_CHUNKS = (1, 2, 8, 9, 63, 64, 65, 71, 72, 73, 127, 128, 129, 200, 255, 256)   # N = ceil(row_bytes / 16)
SUBSET_CHUNKS = (1, 64, 65, 128, 256)     # the kernels that are not the default for reconstruction
GATE = 4096                               # 16 * kPipeMaxChunks (png_filter.hip): the pipeline's last row width
ROWS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1, 70)      # 13 images: 3 and 8 per wavefront do not divide the batch
PATTERNS = ("random", "random", "random", "random", 0, 1, 2, 3, 4, "4/3", "random", "random", "random")
FILL = 0xEE
ENV = ("FDH_PNG_LANE_PER_IMAGE", "FDH_PNG_NO_PIPELINE", "FDH_PNG_IMAGES_PER_WAVE")


def _choose(monkeypatch, per_lane=None, no_pipe=None, per_wave=None):
    gh.set_env(monkeypatch, **dict(zip(ENV, (per_lane, no_pipe, per_wave))))


class Batch:
    """Images of one (row_bytes, bpp) with the oracle's filtered bytes.  Source buffers are packed
    exactly (the kernels derive the row count from the slot); destination buffers are the expected
    image of the WHOLE device buffer: fill in front of, between and behind the images."""

    def __init__(self, r, rb, bpp, rows=ROWS, patterns=PATTERNS, shift=0):
        self.rb, self.bpp, self.n = rb, bpp, len(rows)
        self.pix, self.types, self.filt = [], [], []
        for i, (nr, pat) in enumerate(zip(rows, patterns)):
            p = png_model.pixels(r, png_model.DATA_KINDS[(i + shift) % 4], nr * rb)
            t = png_model.row_types(r, pat, nr)
            st, f = ob.png_filter(p, rb, bpp, t)
            assert st == 0 and len(f) == nr * (rb + 1)
            self.pix.append(p.tobytes())
            self.types.append(t.tobytes())
            self.filt.append(f)
        self.finish()

    def finish(self):
        n = self.n
        slack = [2 * (i % 5) + 1 for i in range(n)]
        zero = [0] * n
        self.src_p_off = gh.offsets([len(p) for p in self.pix], 3, zero)
        self.src_f_off = gh.offsets([len(f) for f in self.filt], 5, zero)
        self.dst_p_off = gh.offsets([len(p) for p in self.pix], 7, slack)
        self.dst_f_off = gh.offsets([len(f) for f in self.filt], 9, slack)
        tbuf, toff = streams.pack_exact(self.types)
        self.tbuf = tbuf if tbuf.size else np.zeros(1, dtype=np.uint8)
        self.toff = toff.astype(np.int64)
        self.src_p = self._image(self.src_p_off, self.pix, 0, 0)
        self.src_f = self._image(self.src_f_off, self.filt, 0, 0)
        self.want_p = self._image(self.dst_p_off, self.pix, FILL, 33)
        self.want_f = self._image(self.dst_f_off, self.filt, FILL, 33)

    @staticmethod
    def _image(off, blobs, fill, tail):
        a = np.full(int(off[-1]) + tail, fill, dtype=np.uint8)
        for o, b in zip(off[:-1], blobs):
            a[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
        return a


def _first_diff(got, want, off):
    """Where a device buffer first differs from its expected image: (slot, byte in the slot); slot -1: in front."""
    at = int(np.nonzero(got != want)[0][0])
    slot = int(np.searchsorted(off, at, side="right")) - 1
    return slot, at - int(off[slot]) if slot >= 0 else at


def _run_unfilter(fd, b, faults, what, status=None):
    import torch
    d_p = torch.full((b.want_p.size,), FILL, dtype=torch.uint8, device="cuda")
    st = fd.png_unfilter_batch(gh.dev(b.src_f), gh.dev(b.src_f_off), d_p, gh.dev(b.dst_p_off), b.rb, b.bpp)
    torch.cuda.synchronize()
    got = d_p.cpu().numpy()
    if st.cpu().tolist() != (status or [0] * b.n):
        faults.append((what, "status", st.cpu().tolist()))
    if not np.array_equal(got, b.want_p):
        slot, at = _first_diff(got, b.want_p, b.dst_p_off)
        faults.append((what, "image %d of %d rows, byte %d = row %d, x %d" % (slot, ROWS[slot] if b.n == len(ROWS) else -1, at, at // b.rb, at % b.rb)))


def _run_filter(fd, b, faults, what):
    import torch
    d_f = torch.full((b.want_f.size,), FILL, dtype=torch.uint8, device="cuda")
    st = fd.png_filter_batch(gh.dev(b.src_p), gh.dev(b.src_p_off), gh.dev(b.tbuf), gh.dev(b.toff), d_f, gh.dev(b.dst_f_off), b.rb, b.bpp)
    torch.cuda.synchronize()
    got = d_f.cpu().numpy()
    if st.cpu().tolist() != [0] * b.n:
        faults.append((what, "status", st.cpu().tolist()))
    if not np.array_equal(got, b.want_f):
        slot, at = _first_diff(got, b.want_f, b.dst_f_off)
        faults.append((what, "image %d, byte %d = row %d, column %d" % (slot, at, at // (b.rb + 1), at % (b.rb + 1))))


@pytest.mark.parametrize("bpp", BPPS)
def test_row_width_classes_through_every_kernel(bpp, monkeypatch):
    """Every width class x 13 ragged images (0 .. 200 rows; one image per pure filter type, one
    alternating Paeth / Average, the others random; random, uniform, 0..3 and 0x00 / 0xFF data in
    turn) against the oracle:
      reconstruction by the default choice (the pipeline up to 4096-byte rows, one image per
      wavefront; png_wave_kernel above) and with 3 and 8 images per wavefront: every width;
      FDH_PNG_NO_PIPELINE=1 (png_wave_kernel at every width) and FDH_PNG_LANE_PER_IMAGE=1, and
      filtering by the default choice and with one image per lane: the widths of N in
      {1, 64, 65, 128, 256} and the three widths above the gate."""
    import torch
    import fdeflate_amd as fd
    assert torch.cuda.is_available()
    t0 = time.time()
    r = np.random.default_rng(4100 + bpp)
    widths = [(n, w) for n in PIPE_CHUNKS for w in gh.widths_of(bpp, n)] + [(0, w) for w in gh.widths_above(bpp, GATE)]
    assert max(w for n, w in widths if n) == GATE // bpp * bpp       # the pipeline's last width
    faults, runs = [], 0
    for k, (n, rb) in enumerate(widths):
        b = Batch(r, rb, bpp, shift=k)
        for per_wave in (None, 3, 8):
            _choose(monkeypatch, per_wave=per_wave)
            _run_unfilter(fd, b, faults, (bpp, rb, "unfilter", "per_wave", per_wave))
            runs += 1
        if n == 0 or n in SUBSET_CHUNKS:
            _choose(monkeypatch, no_pipe=1)
            _run_unfilter(fd, b, faults, (bpp, rb, "unfilter", "no pipeline"))
            _choose(monkeypatch, per_lane=1)
            _run_unfilter(fd, b, faults, (bpp, rb, "unfilter", "lane per image"))
            _run_filter(fd, b, faults, (bpp, rb, "filter", "lane per image"))
            _choose(monkeypatch)
            _run_filter(fd, b, faults, (bpp, rb, "filter", "default"))
            runs += 4
    print("bpp %d: %d widths, %d kernel runs, %.1f s" % (bpp, len(widths), runs, time.time() - t0))
    assert not faults, "%d runs differ, at row widths %s; the first ones: %s" % (len(faults), sorted({f[0][1] for f in faults}), faults[:12])


@pytest.mark.parametrize("bpp", (3, 4))
def test_bad_filter_type_in_a_wide_row(bpp, monkeypatch):
    """Rows of 1536 bytes (N = 96, P = 96), 150 rows, filter type 9 in row 100 -- alone in its call,
    and as the second of eight images with 3 and with 8 images per wavefront: status 1 (the
    oracle's too), rows 0..99 reconstructed, the rows from 100 on not produced, the neighbours
    exact with status 0, nothing written outside the images."""
    import fdeflate_amd as fd
    rb = 1536
    r = np.random.default_rng(4200 + bpp)
    for rows, per_wave in (((150,), None), ((70, 150, 129, 1, 64, 0, 65, 3), 3), ((70, 150, 129, 1, 64, 0, 65, 3), 8)):
        bad = 0 if len(rows) == 1 else 1
        b = Batch(r, rb, bpp, rows=rows, patterns=("random",) * len(rows), shift=bad)
        f = bytearray(b.filt[bad])
        f[100 * (rb + 1)] = 9
        b.filt[bad] = bytes(f)
        est, epix = ob.png_unfilter(b.filt[bad], rb, bpp)
        assert est == 1 and epix[:100 * rb] == b.pix[bad][:100 * rb]
        b.finish()
        o = int(b.dst_p_off[bad])
        b.want_p[o + 100 * rb:o + 150 * rb] = FILL         # not produced: the serial walk stops at the bad row
        faults = []
        _choose(monkeypatch, per_wave=per_wave)
        _run_unfilter(fd, b, faults, (bpp, per_wave), status=[1 if i == bad else 0 for i in range(len(rows))])
        assert not faults, faults


def _gate_widths(bpp):
    return 1024, 1025, 1536, GATE // bpp * bpp, (GATE // bpp + 1) * bpp, 5760


@pytest.mark.parametrize("bpp", (3, 4))
def test_fused_decode_of_mixed_streams_at_real_widths(bpp, monkeypatch):
    """fdh_inflate_png_batch, 100 images of 64 rows per call, at 1024, 1025 and 1536 bytes per row, the
    pipeline's last width, the first width above the gate and 5760: the streams of one call are, in
    turn, the oracle's ultra-fast encoding, zlib level 6 (what a real IDAT holds), zlib level 1 and
    stored blocks -- four decode chains in front of the same gate.  Stream 5 is cut (decode status
    2, png_status 3), stream 9 is a valid stream one row short (png_status 2): neither writes a
    pixel.  Pixels, statuses, lengths and Adler-32 against the oracle, with 1, 4 and 8 images per
    wavefront."""
    import torch
    import fdeflate_amd as fd
    n, rows = 100, 64
    r = np.random.default_rng(4300 + bpp)
    encoders = (ob.compress_ultra_fast, lambda f: zlib.compress(f, 6), lambda f: zlib.compress(f, 1), lambda f: zlib.compress(f, 0))
    t0 = time.time()
    for rb in _gate_widths(bpp):
        b = Batch(r, rb, bpp, rows=(rows,) * n, patterns=("random",) * n, shift=rb)
        comps = [encoders[i % 4](f) for i, f in enumerate(b.filt)]
        comps[5] = comps[5][:-9]
        comps[9] = encoders[1](b.filt[9][:(rows - 1) * (rb + 1)])
        want = [ob.decompress_bounded(c, rows * (rb + 1)) for c in comps]
        assert want[5][0] == 2 and want[9][0] == 0 and len(want[9][1]) == (rows - 1) * (rb + 1)
        for i in (5, 9):   # nothing is reconstructed
            b.want_p[int(b.dst_p_off[i]):int(b.dst_p_off[i]) + rows * rb] = FILL
        cbuf, coff = streams.pack_exact(comps)
        foff = np.arange(n + 1, dtype=np.int64) * (rows * (rb + 1))      # exact: a decoded image fills its slot
        for per_wave in (1, 4, 8):
            _choose(monkeypatch, per_wave=per_wave)
            d_f = torch.zeros(int(foff[-1]), dtype=torch.uint8, device="cuda")
            d_p = torch.full((b.want_p.size,), FILL, dtype=torch.uint8, device="cuda")
            out_len, status, adler, pst = fd.inflate_png_batch(gh.dev(cbuf), gh.dev(coff.astype(np.int64)), d_f, gh.dev(foff),
                                                               d_p, gh.dev(b.dst_p_off), rb, bpp)
            torch.cuda.synchronize()
            stl, psl = status.cpu().numpy().view(np.uint32), pst.cpu().tolist()
            oll, adl = out_len.cpu().numpy().view(np.uint32), adler.cpu().numpy().view(np.uint32)
            what = (bpp, rb, per_wave)
            for i in range(n):
                est, eout, ead = want[i]
                assert int(stl[i]) == est, (what, i, int(stl[i]), est)
                assert psl[i] == (3 if i == 5 else 2 if i == 9 else 0), (what, i, psl[i])
                if est == 0:
                    assert int(oll[i]) == len(eout) and int(adl[i]) == ead, (what, i, int(oll[i]), len(eout))
            got = d_p.cpu().numpy()
            assert np.array_equal(got, b.want_p), (what,) + _first_diff(got, b.want_p, b.dst_p_off)
            hf = d_f.cpu().numpy()
            for i in range(n):
                if i != 5:
                    eout = want[i][1]
                    assert hf[int(foff[i]):int(foff[i]) + len(eout)].tobytes() == eout, (what, "filtered", i)
    print("bpp %d: %.1f s" % (bpp, time.time() - t0))


@pytest.mark.parametrize("bpp", BPPS)
def test_fused_encoder_at_real_widths(bpp):
    """fdh_png_filter_deflate_ultrafast_batch at the two widths of N in {1, 2, 8, 9, 64, 65, 128, 256},
    then 5760, 15 360 and 131 072 bytes per row; 1, 2, 5, 64 and 130 rows; about 40 % of the bytes
    zero and two zero rows (runs in the encoder); random filter types: bit for bit
    compress_ultra_fast(png_filter(...)) of the oracle, nothing written behind a stream."""
    import torch
    import fdeflate_amd as fd
    t0 = time.time()
    r = np.random.default_rng(4400 + bpp)
    widths = [w for n in (1, 2, 8, 9, 64, 65, 128, 256) for w in gh.widths_of(bpp, n)] + [5760, 15360, 131072]
    row_counts = (1, 2, 5, 64, 130)
    for rb in widths:
        pixs, types, want = [], [], []
        for rows in row_counts:
            pix = r.integers(0, 256, rows * rb, dtype=np.uint8)
            pix[r.random(rows * rb) < 0.4] = 0
            if rows >= 5:
                pix[rb:3 * rb] = 0
            t = r.integers(0, 5, rows, dtype=np.uint8)
            est, filt = ob.png_filter(pix, rb, bpp, t)
            assert est == 0
            pixs.append(pix.tobytes())
            types.append(t.tobytes())
            want.append(ob.compress_ultra_fast(filt))
            assert zlib.decompress(want[-1]) == filt
        pbuf, poff = streams.pack_exact(pixs)
        tbuf, toff = streams.pack_exact(types)
        caps = [int(fd.ultrafast_bound(rows * (rb + 1))) for rows in row_counts]
        ooff = gh.offsets(caps, 7, [2 * i + 1 for i in range(len(caps))])
        expect = Batch._image(ooff, want, FILL, 33)
        d_out = torch.full((expect.size,), FILL, dtype=torch.uint8, device="cuda")
        ol, st = fd.png_filter_deflate_ultrafast_batch(gh.dev(pbuf), gh.dev(poff.astype(np.int64)), gh.dev(tbuf), gh.dev(toff.astype(np.int64)),
                                                       d_out, gh.dev(ooff), rb, bpp)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * len(caps), (bpp, rb, st.cpu().tolist())
        assert ol.cpu().tolist() == [len(w) for w in want], (bpp, rb, ol.cpu().tolist(), [len(w) for w in want])
        got = d_out.cpu().numpy()
        assert np.array_equal(got, expect), (bpp, rb) + _first_diff(got, expect, ooff)
    print("bpp %d: %d widths, %.1f s" % (bpp, len(widths), time.time() - t0))


# ---- every (left, up, up-left) triple ----

def _triple_pixels():
    """65 536 images of two 512-byte rows, bpp 1, image a * 256 + c: row 0 is [c, b] for b in 0..255,
    row 1 the constant a.  At every odd x of row 1: left = a, up = b = x // 2, up-left = c."""
    pix = np.empty((256, 256, 2, 512), dtype=np.uint8)
    pix[:, :, 0, 0::2] = np.arange(256, dtype=np.uint8)[None, :, None]
    pix[:, :, 0, 1::2] = np.arange(256, dtype=np.uint8)[None, None, :]
    pix[:, :, 1, :] = np.arange(256, dtype=np.uint8)[:, None, None]
    return pix.reshape(65536, 2, 512)


def _triple_of(at, row):
    """The (a, b, c) behind byte `at` of a buffer of 65 536 images of 2 rows of `row` bytes (512 pixels / 513 filtered)."""
    img, rest = divmod(at, 2 * row)
    x = rest % row - (row - 512)
    return {"a": img >> 8, "c": img & 0xFF, "b": x // 2, "row": rest // row, "x": x}


def _same_on_device(torch, d, expected, row):
    e = gh.dev(expected.reshape(-1))
    if torch.equal(d, e):
        return None
    return _triple_of(int((d != e).nonzero()[0]), row)


@pytest.mark.parametrize("ftype", (4, 3), ids=("paeth", "average"))
def test_every_predictor_triple(ftype, monkeypatch):
    """All 2^24 (left, up, up-left) byte triples through the Paeth and the Average predictor of
    png_filter_batch and png_unfilter_batch -- by the library's OWN kernel choice: 65 536 images make
    it put eight of them on a wavefront of the pipeline, the one case where that rule decides and
    not the environment -- and of the fused encoder, whose streams are decoded again on the GPU.
    Expected: tests/png_model.py (the specification in int32 numpy), equal to the oracle on 256 of
    the images.  All comparisons stay on the device."""
    import torch
    import fdeflate_amd as fd
    _choose(monkeypatch)
    t0 = time.time()
    n, rb = 65536, 512
    pix = _triple_pixels()
    types = np.array([0, ftype], dtype=np.uint8)
    filt = np.empty((n, 2, rb + 1), dtype=np.uint8)
    for i in range(0, n, 4096):
        filt[i:i + 4096] = png_model.filter_rows(pix[i:i + 4096], 1, types)
    for i in (np.arange(256) * 255).tolist():
        assert ob.png_filter(pix[i].tobytes(), rb, 1, types) == (0, filt[i].tobytes()), i
        assert ob.png_unfilter(filt[i].tobytes(), rb, 1) == (0, pix[i].tobytes()), i
    # left = a, up = b, up-left = c at the odd bytes of row 1: every triple is there
    assert np.array_equal(filt[:, 1, 2::2].reshape(256, 256, 256)[7, 9], (7 - png_model.predictor(ftype, 7, np.arange(256), 9)) & 0xFF)
    poff = gh.dev(np.arange(n + 1, dtype=np.int64) * (2 * rb))
    foff = gh.dev(np.arange(n + 1, dtype=np.int64) * (2 * (rb + 1)))
    toff = gh.dev(np.arange(n + 1, dtype=np.int64) * 2)
    d_types = gh.dev(np.tile(types, n))
    d_pix, d_filt = gh.dev(pix.reshape(-1)), gh.dev(filt.reshape(-1))
    # filter
    out = torch.full((n * 2 * (rb + 1),), FILL, dtype=torch.uint8, device="cuda")
    st = fd.png_filter_batch(d_pix, poff, d_types, toff, out, foff, rb, 1)
    assert int(st.abs().sum()) == 0
    assert torch.equal(out, d_filt), ("filter", _same_on_device(torch, out, filt, rb + 1))
    # reconstruction
    out = torch.full((n * 2 * rb,), FILL, dtype=torch.uint8, device="cuda")
    st = fd.png_unfilter_batch(d_filt, foff, out, poff, rb, 1)
    assert int(st.abs().sum()) == 0
    assert torch.equal(out, d_pix), ("unfilter", _same_on_device(torch, out, pix, rb))
    # the fused encoder, decoded again
    bound = (int(fd.ultrafast_bound(2 * (rb + 1))) + 15) & ~15
    coff = gh.dev(np.arange(n + 1, dtype=np.int64) * bound)
    comp = torch.zeros(n * bound, dtype=torch.uint8, device="cuda")
    clen, pst = fd.png_filter_deflate_ultrafast_batch(d_pix, poff, d_types, toff, comp, coff, rb, 1)
    assert int(pst.abs().sum()) == 0
    assert int(clen.min()) > 0 and int(clen.max()) <= bound
    out = torch.full((n * 2 * (rb + 1),), FILL, dtype=torch.uint8, device="cuda")
    out_len, status, adler = fd.inflate_batch(comp, coff, out, foff)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and bool((out_len == 2 * (rb + 1)).all())
    assert torch.equal(out, d_filt), ("fused encoder", _same_on_device(torch, out, filt, rb + 1))
    for i in (0, 255, 4660, 65535):   # ... and four of its streams bit for bit
        w = ob.compress_ultra_fast(filt[i].tobytes())
        assert int(clen[i]) == len(w) and comp[i * bound:i * bound + len(w)].cpu().numpy().tobytes() == w, i
    print("filter type %d: %.1f s" % (ftype, time.time() - t0))
