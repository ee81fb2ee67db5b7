"""-m gpu: Adam7 interlaced PNG images -- fdh_png_unfilter_interlaced_batch, FDH_PNG_FLAG_ADAM7 in the scan and in
png_decode_files_batch / png_decode_files_rgba_batch.

Referee: tests/png_adam7_model.py (plain integers, pinned to Pillow's reader and to the specification's pass pattern by
tests/test_png_adam7_model.py); Pillow once more on the files that go end to end.  Everything is byte for byte.

png_adam7_recon_kernel: grid(n), one wavefront per image (there is no cap on the grid: a batch of more images than the
device holds wavefronts is queued by the hardware), bands of 64 pass rows.  png_adam7_place_kernel: grid(n, waves), a
wavefront takes the bands b, b + waves, .. of 64 picture rows; waves = min(4096, ceil(32768 / n)), one from n = 32768 on.
"""
import zlib

import numpy as np
import pytest

import png_adam7_model as am
import png_corpus as pc
import png_expand_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_model as pm

pytestmark = pytest.mark.gpu

GUARD = 0x5A
PASSED_ON = 77          # an upstream status (png_status 3): such entries are the guards between the images
ANY = "any"             # a pix slot whose contents are not specified (status 1)


class Entry:
    """One image of a call: the bytes of its filt slot, the size of its pix slot, and what is expected."""

    def __init__(self, filt, pix_size, want, status=0, method=1, upstream=0, upstream_len=None):
        self.filt = np.frombuffer(bytes(filt), dtype=np.uint8)
        self.pix_size, self.want, self.status, self.method, self.upstream = pix_size, want, status, method, upstream
        self.upstream_len = len(self.filt) if upstream_len is None else upstream_len


def run(fd, entries, geometry, guards=True, method="given", gates=True, front=3):
    """One call over `entries` (with guards: a guard entry in front of, between and behind them; the buffers start at
    byte `front`, odd, and have guard bytes behind the last slot).  Checks every status, every pix slot (want: bytes, None
    = untouched, ANY), every guard byte of both buffers.  -> the pix buffer."""
    import torch
    if guards:
        # a guard entry -- slots of guard bytes that `upstream` marks as failed, so they must stay as they are -- in front of
        # every image and behind the last one, sized so that what follows starts at an odd address in both buffers
        seq, f_at, p_at = [], front, front
        for k, e in enumerate(list(entries) + [None]):
            fl, pl = 5 + 2 * (k % 3), 7 + 2 * (k % 2)
            fl += (f_at + fl + 1) % 2
            pl += (p_at + pl + 1) % 2
            seq.append(Entry(bytes([GUARD]) * fl, pl, None, status=3, method=k % 2, upstream=PASSED_ON))
            f_at, p_at = f_at + fl, p_at + pl
            if e is not None:
                assert f_at % 2 == 1 and p_at % 2 == 1
                seq.append(e)
                f_at, p_at = f_at + len(e.filt), p_at + e.pix_size
    else:
        seq = list(entries)
    n = len(seq)
    f_off = np.concatenate([[front], front + np.cumsum([len(e.filt) for e in seq])]).astype(np.int64)
    p_off = np.concatenate([[front], front + np.cumsum([e.pix_size for e in seq])]).astype(np.int64)
    filt = np.full(int(f_off[-1]) + 9, GUARD, dtype=np.uint8)
    for o, e in zip(f_off[:-1], seq):
        filt[int(o):int(o) + len(e.filt)] = e.filt
    d_filt = gh.dev(filt)
    d_pix = torch.full((int(p_off[-1]) + 33,), GUARD, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    fd.png_unfilter_interlaced_batch(
        d_filt, gh.dev(f_off), d_pix, gh.dev(p_off), *geometry,
        method=None if method is None else gh.dev(np.array([e.method for e in seq], dtype=np.uint8)),
        upstream=gh.words([e.upstream for e in seq]) if gates else None,
        upstream_len=gh.words([e.upstream_len for e in seq]) if gates else None, png_status=st[8:8 + n])
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + n:] == 0x5A5A5A5A).all()
    assert st[8:8 + n].tolist() == [e.status for e in seq], (geometry, st[8:8 + n].tolist(), [e.status for e in seq])
    got, after = d_pix.cpu().numpy(), d_filt.cpu().numpy()
    assert (got[:front] == GUARD).all() and (got[int(p_off[-1]):] == GUARD).all()
    assert (after[:front] == GUARD).all() and (after[int(f_off[-1]):] == GUARD).all()
    for k, e in enumerate(seq):
        slot = got[int(p_off[k]):int(p_off[k + 1])]
        if e.want is None:
            assert (slot == GUARD).all(), (geometry, k, "a slot that must stay as it is was written")
            if e.status != 0:       # nothing written and nothing reconstructed: the filt slot is as it was
                assert np.array_equal(after[int(f_off[k]):int(f_off[k + 1])], e.filt), (geometry, k)
        elif e.want is not ANY:
            want = np.frombuffer(bytes(e.want), dtype=np.uint8)
            if not np.array_equal(slot, want):
                at = int(np.nonzero(slot != want)[0][0])
                raise AssertionError("%r image %d of %d (method %d, %d pix bytes): byte %d is %d, not %d"
                                     % (geometry, k, n, e.method, e.pix_size, at, slot[at], want[at]))
    return got


def random_types(r, width, height, force=None):
    """Random types per pass row; with `force` every pass's first row has that type."""
    types, at = r.integers(0, 5, am.pass_rows(width, height)).tolist(), 0
    for _, ph in am.passes(width, height):
        if ph and force is not None:
            types[at] = force
        at += ph
    return types


def adam7_entry(r, width, height, depth, colour, force=None, types=None):
    """A random picture (padding bits zero), interlaced and filtered by the model."""
    rb = fm.geometry(width, depth, colour)[0]
    pix = pc.clear_padding(r.integers(0, 256, height * rb, dtype=np.uint8), width, height, depth, colour)
    types = random_types(r, width, height, force) if types is None else types
    stream = am.filter_passes(am.interlace(pix, width, height, depth, colour), width, height, depth, colour, types)
    assert len(stream) == am.size(width, height, depth, colour)
    return Entry(stream, height * rb, pix.tobytes())


def progressive_entry(r, width, height, depth, colour):
    """Random filtered bytes of a progressive image: what pm.unfilter makes of them, padding bits as they come."""
    rb, bpp = fm.geometry(width, depth, colour)
    filt = r.integers(0, 256, (height, rb + 1), dtype=np.uint8)
    filt[:, 0] = r.integers(0, 5, height)
    return Entry(filt.tobytes(), height * rb, pm.unfilter(filt.tobytes(), rb, bpp), method=0)


def special_widths(depth, colour):
    """Widths that put the picture row (= a row of pass 7) and a row of pass 6 at 15 / 16 / 17 / 33 and 127 / 128 / 129
    bytes, or as near as whole pixels allow on either side; below 8 bits per pixel also widths at which neither the
    picture's rows nor most passes' rows fill their last byte."""
    bits = fm.CHANNELS[colour] * depth
    out = set()
    for size in (15, 16, 17, 33, 127, 128, 129):
        for w in (max(1, size * 8 // bits), -(-size * 8 // bits)):
            out |= {w, 2 * w, 2 * w + 1}
    if bits < 8:
        out |= {21, 23, 43}
    return sorted(out)


@pytest.mark.parametrize("pair", fm.PAIRS, ids=["depth%d-colour%d" % p for p in fm.PAIRS])
def test_every_pair_smallest_shapes(pair):
    """Widths and heights 1 .. 9 -- every combination of empty passes: widths below 5, 3, 2 empty passes 2, 4, 6,
    heights below 5, 3, 2 empty passes 3, 5, 7 --, one call per width with the nine heights; then the widths of
    special_widths at heights 2 and 9.  Random filter types per pass row, every pass's first row forced to Up, Average
    and Paeth in three of four images: a kernel that takes the last row of the pass before as "above" fails there.  The
    pix buffer equals the model's byte for byte, guards included."""
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(8400 + 64 * colour + depth)
    for width in range(1, 10):
        entries = [adam7_entry(r, width, h, depth, colour, force=(2, 3, 4, None)[(width + h) % 4]) for h in range(1, 10)]
        run(fd, entries, (width, depth, colour))
    for k, width in enumerate(special_widths(depth, colour)):
        entries = [adam7_entry(r, width, h, depth, colour, force=(2, 3, 4, None)[(k + h) % 4]) for h in (2, 9)]
        run(fd, entries, (width, depth, colour))


@pytest.mark.parametrize("pair", ((1, 0), (2, 0), (4, 0), (1, 3), (2, 3), (4, 3)), ids=lambda p: "depth%d-colour%d" % p)
def test_padding_bits_of_the_pass_rows_do_not_reach_the_picture(pair):
    """Below 8 bits per pixel a pass row may carry anything in the padding bits of its last byte -- pass 7's rows are
    the picture's odd rows, byte for byte otherwise.  Every pass row's padding bits set: the picture's are zero, as the
    model's deinterlace gives them.  Widths whose row ends in byte 1, 16, 17 of a chunk; also as method None."""
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(8450 + 8 * colour + depth)
    per = 8 // depth
    for width in (1, per + 1, 3 * per - 1, 16 * per - 1, 16 * per + 1, 21 * per + 1):
        rb = fm.geometry(width, depth, colour)[0]
        entries = []
        for height in (2, 9):
            pix = pc.clear_padding(r.integers(0, 256, height * rb, dtype=np.uint8), width, height, depth, colour)
            images = []
            for (pw, ph), img in zip(am.passes(width, height), am.interlace(pix, width, height, depth, colour)):
                spare = -(pw * depth) % 8
                if ph and spare:
                    a = np.array(np.frombuffer(img, dtype=np.uint8)).reshape(ph, -1)
                    a[:, -1] |= (1 << spare) - 1
                    img = a.tobytes()
                images.append(img)
            assert am.deinterlace(images, width, height, depth, colour) == pix.tobytes()
            stream = am.filter_passes(images, width, height, depth, colour, random_types(r, width, height))
            entries.append(Entry(stream, height * rb, pix.tobytes()))
        assert (width * depth) % 8
        run(fd, entries, (width, depth, colour))
        run(fd, entries, (width, depth, colour), method=None, guards=False, gates=False)


def test_band_boundaries():
    """3 x 131 RGB8: pass 7 has 65 rows, 230 pass rows in all; 9 x 513 grey-8: pass 1 has 65 rows, 964 in all.  The row
    list is cut into bands of 64: lane 0 of a later band reads the row above from memory, or starts a pass."""
    import fdeflate_amd as fd
    r = np.random.default_rng(8500)
    assert am.passes(3, 131)[6] == (3, 65) and am.pass_rows(3, 131) == 230
    assert am.passes(9, 513)[0] == (2, 65) and am.pass_rows(9, 513) == 964
    for width, height, depth, colour in ((3, 131, 8, 2), (9, 513, 8, 0)):
        for force in (4, 3, None):
            run(fd, [adam7_entry(r, width, height, depth, colour, force=force), adam7_entry(r, width, 7, depth, colour)], (width, depth, colour))
        # every row Paeth / every row Average: each row needs the one above it, across every band boundary
        for t in (4, 3):
            run(fd, [adam7_entry(r, width, height, depth, colour, types=[t] * am.pass_rows(width, height))], (width, depth, colour))


@pytest.mark.parametrize("shape", ((345, 8, 2), (8301, 1, 0), (2051, 4, 3), (130, 16, 6)), ids=lambda s: "width%d-depth%d-colour%d" % s)
def test_rows_of_more_than_64_chunks(shape):
    """Picture rows of 1035 to 1040 bytes, 65 chunks of 16: the placement's lanes take more than one chunk of a row,
    the last of them partial; the widest pass rows are as long."""
    import fdeflate_amd as fd
    width, depth, colour = shape
    assert 1024 < fm.geometry(width, depth, colour)[0] <= 1040
    r = np.random.default_rng(8550 + depth)
    run(fd, [adam7_entry(r, width, h, depth, colour, force=f) for h, f in ((2, 4), (9, 3), (5, None))] + [progressive_entry(r, width, 3, depth, colour)],
        (width, depth, colour))


@pytest.mark.parametrize("pair", ((8, 2), (1, 0), (4, 3), (16, 6)), ids=lambda p: "depth%d-colour%d" % p)
def test_methods_in_one_batch(pair):
    """A batch alternating progressive and Adam7 images: the progressive ones are pm.unfilter's bytes and equal
    fdh_png_unfilter_batch on the same bytes; method = None reads every image as Adam7, as a method array of ones does."""
    import torch
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(8600 + depth)
    for width in (7, 37, 70):
        rb, bpp = fm.geometry(width, depth, colour)
        entries = []
        for h in (1, 4, 9, 67):
            entries += [progressive_entry(r, width, h, depth, colour), adam7_entry(r, width, h, depth, colour)]
        run(fd, entries, (width, depth, colour))
        run(fd, entries, (width, depth, colour), guards=False, gates=False, front=1)
        prog = entries[0::2]
        f_off = np.concatenate([[1], 1 + np.cumsum([len(e.filt) for e in prog])]).astype(np.int64)
        p_off = np.concatenate([[0], np.cumsum([e.pix_size for e in prog])]).astype(np.int64)
        filt = np.concatenate([[0]] + [e.filt for e in prog]).astype(np.uint8)
        pix = torch.empty(int(p_off[-1]), dtype=torch.uint8, device="cuda")
        st = fd.png_unfilter_batch(gh.dev(filt), gh.dev(f_off), pix, gh.dev(p_off), rb, bpp)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * len(prog)
        assert pix.cpu().numpy().tobytes() == b"".join(bytes(e.want) for e in prog)
        inter = entries[1::2]
        run(fd, inter, (width, depth, colour), method=None)
        run(fd, inter, (width, depth, colour), method=None, guards=False, gates=False)


def test_statuses():
    """A filter type of 5 in each of the seven passes in turn: 1.  A filt slot one byte short or long, a pix slot that is
    not whole rows, a short upstream_len, a method byte of 2: 2 and nothing written.  upstream not 0: 3 and nothing
    written.  Two empty slots: 0.  Sound images in between are exact and every guard byte is intact."""
    import fdeflate_amd as fd
    r = np.random.default_rng(8700)
    width, height, depth, colour = 7, 9, 8, 2
    rb = fm.geometry(width, depth, colour)[0]
    geometry = (width, depth, colour)

    def good():
        return adam7_entry(r, width, height, depth, colour)

    entries = [good()]
    at = 0
    for pw, ph in am.passes(width, height):
        assert ph
        e = good()
        filt = e.filt.copy()
        filt[at + (ph - 1) * (1 + pw * 3)] = 5              # the type byte of the pass's last row
        entries += [Entry(filt, e.pix_size, ANY, status=1), good()]
        at += ph * (1 + pw * 3)
    e = good()
    entries += [Entry(e.filt[:-1], e.pix_size, None, status=2), good()]
    entries += [Entry(np.concatenate([e.filt, [0]]).astype(np.uint8), e.pix_size, None, status=2), good()]
    entries += [Entry(e.filt, e.pix_size + 1, None, status=2), Entry(e.filt, e.pix_size - rb + 1, None, status=2), good()]
    entries += [Entry(e.filt, e.pix_size, None, status=2, upstream_len=len(e.filt) - 1), good()]
    entries += [Entry(e.filt, e.pix_size, None, status=2, method=2), Entry(e.filt, e.pix_size, None, status=2, method=255), good()]
    entries += [Entry(e.filt, e.pix_size, None, status=3, upstream=15), Entry(e.filt, e.pix_size, None, status=3, upstream=0x80000000), good()]
    entries += [Entry(b"", 0, b""), Entry(b"", 0, b"", method=0), Entry(b"", rb, None, status=2), Entry(e.filt, 0, None, status=2), good()]
    # the same bytes as a progressive image: 9 rows of 22 bytes are not this stream's size
    entries += [Entry(e.filt, e.pix_size, None, status=2, method=0), good()]
    run(fd, entries, geometry)
    # without the gates the entries they refused are images like the others
    run(fd, [x for x in entries if x.upstream == 0 and x.upstream_len == len(x.filt)], geometry, guards=False, gates=False)


def test_one_by_nine_reads_both_ways():
    """1 x 9 grey-8 is 18 bytes progressive and 18 bytes interlaced: the same bytes as method 0 and as method 1 pass the
    size check both ways and give different pictures where the types refer to the row above."""
    import fdeflate_amd as fd
    r = np.random.default_rng(8800)
    assert am.size(1, 9, 8, 0) == 18
    filt = r.integers(1, 256, (9, 2), dtype=np.uint8)
    filt[:, 0] = [2, 2, 4, 3, 2, 2, 4, 3, 2]
    raw = filt.tobytes()
    progressive = pm.unfilter(raw, 1, 1)
    interlaced = am.deinterlace(am.unfilter_passes(raw, 1, 9, 8, 0), 1, 9, 8, 0)
    assert progressive != interlaced
    run(fd, [Entry(raw, 9, progressive, method=0), Entry(raw, 9, interlaced, method=1), Entry(raw, 9, progressive, method=0)], (1, 8, 0))


@pytest.mark.parametrize("n", (5000, 33000))
def test_more_images_than_wavefronts(n):
    """5 x 5 images, more than the device holds wavefronts at once and, at 33 000, more than the count from which the
    placement runs one wavefront per image: 40 different RGB8 images and 40 one-bit ones, repeated."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(8900)
    for depth, colour in ((8, 2), (1, 0)):
        kinds = [adam7_entry(r, 5, 5, depth, colour) for _ in range(40)]
        fs, ps = len(kinds[0].filt), kinds[0].pix_size
        reps = -(-n // 40)
        filt = np.tile(np.concatenate([e.filt for e in kinds]), reps)[:n * fs]
        want = np.tile(np.concatenate([np.frombuffer(e.want, dtype=np.uint8) for e in kinds]), reps)[:n * ps]
        d_filt = gh.dev(np.concatenate([[GUARD], filt, [GUARD] * 8]).astype(np.uint8))
        pix = torch.full((n * ps + 32,), GUARD, dtype=torch.uint8, device="cuda")
        st = fd.png_unfilter_interlaced_batch(d_filt, gh.dev(1 + np.arange(n + 1, dtype=np.int64) * fs), pix,
                                              gh.dev(3 + np.arange(n + 1, dtype=np.int64) * ps), 5, depth, colour)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        got = pix.cpu().numpy()
        assert (got[:3] == GUARD).all() and (got[3 + n * ps:] == GUARD).all()
        assert np.array_equal(got[3:3 + n * ps], want), (n, depth, colour)


# ---- the scan ----

def test_scan_accepts_adam7_on_request():
    """An interlaced file with the flag: status 0, interlace 1, every count as the scan of the same file with method 0;
    without the flag 4 and the walk ends at IHDR, as ever.  Method 2 is 3 both ways; a CRC error behind the IHDR of an
    interlaced file is 6 with the flag (4 without); a progressive file reads the same both ways."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(9000)
    width, height = 11, 6
    pix = r.integers(0, 256, height * width * 3, dtype=np.uint8)
    types = random_types(r, width, height)
    pre = [(b"tEXt", b"Comment\0in front")]
    stream = am.stream_of(pix, width, height, 8, 2, types)
    inter = am.write_file(stream, width, height, 8, 2, pre, 3, zlib.crc32)
    as_progressive = am.write_file(stream, width, height, 8, 2, pre, 3, zlib.crc32, method=0)
    two = am.write_file(stream, width, height, 8, 2, pre, 3, zlib.crc32, method=2)
    damaged = bytearray(inter)
    damaged[8 + 25 + 8 + 3] ^= 0x10                          # a byte of the tEXt's body
    in_ihdr = bytearray(inter)
    in_ihdr[29] ^= 1                                        # the IHDR's own CRC field
    files = [inter, as_progressive, two, bytes(damaged), bytes(in_ihdr), inter[:60], inter]
    host, f_off, f_len = gh.batch_of(files)
    for flags, adam7, ignore in ((0, False, False), (fd.PNG_FLAG_ADAM7, True, False),
                                 (fd.PNG_FLAG_ADAM7 | fd.PNG_FLAG_IGNORE_CRC, True, True), (fd.PNG_FLAG_IGNORE_CRC, False, True)):
        info = fd.png_scan_files_batch(gh.dev(host), gh.dev(f_off), gh.dev(f_len), flags=flags)
        torch.cuda.synchronize()
        rows = gh.info_rows(fd, info)
        assert rows == [am.scan(f, adam7, ignore, zlib.crc32).fields() for f in files], flags
        st = [w[0] for w in rows]
        if adam7:
            assert st == [0, 0, 3, 0 if ignore else 6, 0 if ignore else 6, 2, 0]
            plain = fm.scan(as_progressive, crc=zlib.crc32).fields()
            assert rows[0][5] == 1 and rows[0][:5] + rows[0][6:] == plain[:5] + plain[6:] and plain[7] == 3
        else:
            assert st == [4, 0, 3, 4, 4, 4, 4] and rows[0][5] == 1 and rows[0][6:] == (0, 0, 0, 0)


# ---- files end to end ----

END_TO_END = ((8, 3, True), (2, 3, True), (8, 2, True), (16, 6, False), (1, 0, False), (8, 0, True), (16, 4, False))


@pytest.mark.parametrize("cls", END_TO_END, ids=["depth%d-colour%d" % c[:2] for c in END_TO_END])
def test_files_end_to_end(cls):
    """Model-written Adam7 files (a tEXt in front, PLTE, tRNS, a level-6 stream in three IDAT chunks) in one batch with
    progressive files, a truncated file and an interlaced file of another width, through png_decode_files_batch and
    png_decode_files_rgba_batch.  With PNG_FLAG_ADAM7: the packed pixels are the model's and the pictures the model's
    expansion and Pillow's convert("RGBA").  Without it: the interlaced files are info.status 4 / png_status 3 with
    empty slots, and everything else is as with the flag."""
    import torch
    import fdeflate_amd as fd
    depth, colour, keyed = cls
    r = np.random.default_rng(9100 + 64 * colour + depth)
    width = 37
    rb = fm.geometry(width, depth, colour)[0]

    def make(height, interlaced, w=width):
        pix, key, pal = pc.random_case(r, w, height, depth, colour, keyed)
        pix = pc.clear_padding(pix, w, height, depth, colour)
        pre = pc.pre_chunks(colour, key, pal, text=True)
        if interlaced:
            png = am.write_file(am.stream_of(pix, w, height, depth, colour, random_types(r, w, height)), w, height, depth, colour, pre, 3, zlib.crc32)
        else:
            png = em.write_file(pc.stream_of(pix, fm.geometry(w, depth, colour)[0]), w, height, depth, colour, pre, 3, zlib.crc32)
        rgba = em.expand(pix, w, depth, colour, key, pal)[0]
        assert pc.pillow_rgba(png) == rgba or (keyed and (depth, colour) in pc.LEFT_OUT)
        return png, pix.tobytes(), rgba, height, interlaced

    cases = [make(9, True), make(7, False), make(70, True), make(3, False), make(1, True)]
    cut = cases[2][0][:len(cases[2][0]) // 2]
    other = make(5, True, w=width + 1)[0]
    #        file, pixels, rgba, height, interlaced, png_status with the flag
    plan = [cases[0] + (0,), cases[1] + (0,), (cut, b"", b"", 0, True, 3), cases[2] + (0,), (other, b"", b"", 0, True, 7),
            cases[3] + (0,), cases[4] + (0,)]
    host, f_off, f_len = gh.batch_of([p[0] for p in plan])
    for flags in (fd.PNG_FLAG_ADAM7, 0):
        shown = [p if (flags or not p[4]) else (p[0], b"", b"", 0, True, 3) for p in plan]
        want_info = [4 if (p[4] and not flags) else (2 if p[0] is cut else 0) for p in plan]
        pix, pix_off, info, status, png_status = fd.png_decode_files_batch(gh.dev(host), gh.dev(f_off), width, depth, colour,
                                                                           file_len=gh.dev(f_len), flags=flags)
        torch.cuda.synchronize()
        assert info[:, 0].cpu().tolist() == want_info, (cls, flags)
        assert gh.info_rows(fd, info) == [am.scan(p[0], bool(flags), False, zlib.crc32).fields() for p in plan]
        assert png_status.cpu().tolist() == [p[5] for p in shown], (cls, flags)
        assert [status[k].item() for k, p in enumerate(shown) if p[5] == 0] == [0] * sum(1 for p in shown if p[5] == 0)
        assert pix_off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(p[1]) for p in shown])]).tolist()
        assert pix.cpu().numpy().tobytes() == b"".join(p[1] for p in shown), (cls, flags)
        rgba, rgba_off, info, status, png_status = fd.png_decode_files_rgba_batch(gh.dev(host), gh.dev(f_off), width, depth, colour,
                                                                                 file_len=gh.dev(f_len), flags=flags)
        torch.cuda.synchronize()
        assert info[:, 0].cpu().tolist() == want_info and png_status.cpu().tolist() == [p[5] for p in shown], (cls, flags)
        assert rgba_off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(p[2]) for p in shown])]).tolist()
        assert rgba.cpu().numpy().tobytes() == b"".join(p[2] for p in shown), (cls, flags)


def test_a_batch_without_interlaced_files_is_the_same_with_the_flag():
    """Progressive files only: with PNG_FLAG_ADAM7 every output equals the one without it."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(9200)
    width, depth, colour = 29, 8, 6
    rb = fm.geometry(width, depth, colour)[0]
    files = []
    for height in (1, 5, 66):
        pix = r.integers(0, 256, height * rb, dtype=np.uint8)
        files.append(em.write_file(pc.stream_of(pix, rb), width, height, depth, colour, (), 2, zlib.crc32))
    files.insert(1, files[0][:50])
    host, f_off, f_len = gh.batch_of(files)
    outs = []
    for flags in (0, fd.PNG_FLAG_ADAM7):
        res = fd.png_decode_files_rgba_batch(gh.dev(host), gh.dev(f_off), width, depth, colour, file_len=gh.dev(f_len), flags=flags)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy().tobytes() for t in res])
    assert outs[0] == outs[1]


def test_bench_shape_against_torch():
    """4096 interlaced 341 x 64 RGB8 images, every row of type None: the reconstruction leaves the bytes as they are, and
    the placement equals strided slice assignment per pass in torch on the device."""
    import torch
    import fdeflate_amd as fd
    n, width, rows = 4096, 341, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(9300)
    picture = torch.randint(0, 256, (n, rows, width, 3), dtype=torch.uint8, device="cuda", generator=g)
    parts = []
    for p, (pw, ph) in enumerate(am.passes(width, rows)):
        sub = picture[:, am.Y0[p]::am.DY[p], am.X0[p]::am.DX[p], :].reshape(n, ph, pw * 3)
        parts.append(torch.cat([torch.zeros((n, ph, 1), dtype=torch.uint8, device="cuda"), sub], dim=2).reshape(n, -1))
    filt = torch.cat(parts, dim=1).contiguous()
    size = am.size(width, rows, 8, 2)
    assert filt.shape == (n, size) and size == 65592
    # the torch formulation of the placement, from the stream's bytes
    want = torch.empty_like(picture)
    at = 0
    for p, (pw, ph) in enumerate(am.passes(width, rows)):
        block = filt[:, at:at + ph * (1 + pw * 3)].view(n, ph, 1 + pw * 3)[:, :, 1:]
        want[:, am.Y0[p]::am.DY[p], am.X0[p]::am.DX[p], :] = block.reshape(n, ph, pw, 3)
        at += ph * (1 + pw * 3)
    assert torch.equal(want, picture)
    f_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * size
    p_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * width * 3)
    pix = torch.empty(n * rows * width * 3, dtype=torch.uint8, device="cuda")
    st = fd.png_unfilter_interlaced_batch(filt.view(-1), f_off, pix, p_off, width, 8, 2)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    assert torch.equal(pix.view(n, rows, width, 3), want)
