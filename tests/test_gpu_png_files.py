"""-m gpu: PNG files on the device -- fdh_crc32_batch, fdh_png_frame_batch / png_encode_files_batch,
fdh_png_scan_files_batch, fdh_png_gather_idat_batch / png_decode_files_batch.

Referees: zlib.crc32 for every checksum; tests/png_file_model.py (pinned to zlib and Pillow by
tests/test_png_file_model.py) for the framing and for what the scan reports; the oracle's ultra-fast
encoder around png_choose_model's types for the streams; Pillow for the pixels of every file it can show
in full (8-bit samples and 16-bit grey; of 16-bit colour it keeps the high bytes, which are compared).
Where the model writes many large files it is handed zlib's crc32 in place of its bit-at-a-time one (the
two are compared in the CPU test).  Everything is bit-exact.

crc32_ranges_kernel gives a range one wavefront in a batch of 4096 ranges or more and several in a smaller
one; FDH_CRC_PIECES forces the number, FDH_CRC_COPIES the number of table copies in the LDS (1, 8, 32).
"""
import time
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import png_choose_model as cm
import png_corpus as pc
import png_file_model as fm
import png_gpu_harness as gh

pytestmark = pytest.mark.gpu

FILL = 0xEE
GUARD32 = 0x5A5A5A5A
GATE = 4096         # the row widths are those of tests/test_gpu_png_choose.py: its gate
ENV = ("FDH_CRC_PIECES", "FDH_CRC_COPIES")
# (bytes per pixel, bit depth, colour type): bpp 1, 2, 3, 4 at 8 bits, 2, 4, 6, 8 at 16
GEOMETRIES = ((1, 8, 0), (2, 8, 4), (3, 8, 2), (4, 8, 6), (2, 16, 0), (4, 16, 4), (6, 16, 2), (8, 16, 6))


def _shape(monkeypatch, pieces=None, copies=None):
    gh.set_env(monkeypatch, **dict(zip(ENV, (pieces, copies))))


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _guarded(n):
    """An int32 [n] view with 8 guard words either side -> (whole buffer, view)."""
    import torch
    whole = torch.full((n + 16,), GUARD32, dtype=torch.int32, device="cuda")
    return whole, whole[8:8 + n]


def _guards_intact(whole, n):
    w = _u32(whole)
    return bool((w[:8] == GUARD32).all() and (w[8 + n:] == GUARD32).all())


def _crc(fd, data, off, length=None, seed=None):
    """fd.crc32_batch into guarded result arrays -> (crc, status) as int64 numpy."""
    import torch
    n = off.size - 1
    cw, c = _guarded(n)
    sw, s = _guarded(n)
    fd.crc32_batch(data, gh.dev(off), None if length is None else gh.dev(np.asarray(length, dtype=np.uint32).view(np.int32)),
                   None if seed is None else gh.dev(np.asarray(seed, dtype=np.uint32).view(np.int32)), c, s)
    torch.cuda.synchronize()
    assert _guards_intact(cw, n) and _guards_intact(sw, n)
    return _u32(c), _u32(s)


# ---- fdh_crc32_batch ----

@pytest.mark.parametrize("shape", ((None, None), (3, None), (None, 8), (2, 32)), ids=("default", "3-pieces", "8-copies", "2-pieces-32-copies"))
def test_crc_every_length_at_every_alignment(shape, monkeypatch):
    """Ranges of every length 0 .. 300 at every alignment 0 .. 15 of their first byte, one batch of 4816: with `len`
    (the ranges lie apart, in slots that are longer) and without (the ranges are the slots, back to back from an odd
    offset), with seeds and without."""
    import torch
    import fdeflate_amd as fd
    _shape(monkeypatch, *shape)
    r = np.random.default_rng(6100)
    lens, off = [], [0]
    for n in range(301):
        for al in range(16):
            start = off[-1] + ((al - off[-1]) % 16)
            off[-1] = start                    # (the slack goes to the slot in front)
            lens.append(n)
            off.append(start + n + int(r.integers(0, 3)))
    off = np.asarray(off, dtype=np.int64)
    assert sorted(set((off[:-1] % 16).tolist())) == list(range(16))
    host = r.integers(0, 256, int(off[-1]) + 16, dtype=np.uint8)
    data = gh.dev(host)
    assert data.data_ptr() % 16 == 0
    raw = host.tobytes()
    seeds = r.integers(0, 1 << 32, len(lens), dtype=np.uint64).astype(np.uint32)
    for seed in (None, seeds):
        want = [zlib.crc32(raw[int(o):int(o) + n], 0 if seed is None else int(seed[k])) for k, (o, n) in enumerate(zip(off[:-1], lens))]
        crc, st = _crc(fd, data, off, lens, seed)
        assert st.tolist() == [0] * len(lens)
        assert crc.tolist() == want, int(np.nonzero(crc != np.asarray(want))[0][0])
        # without len: the slots themselves, from byte 5 on
        off2 = np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.int64)
        want = [zlib.crc32(raw[int(a):int(b)], 0 if seed is None else int(seed[k])) for k, (a, b) in enumerate(zip(off2[:-1], off2[1:]))]
        crc, st = _crc(fd, data, off2, None, seed)
        assert st.tolist() == [0] * len(lens) and crc.tolist() == want
    assert np.array_equal(data.cpu().numpy(), host)


@pytest.mark.parametrize("copies", (None, 8, 32))
def test_crc_ragged_ranges(copies, monkeypatch):
    """70 ranges of 0 .. 300 000 bytes (several wavefronts each): the slots, and shorter lengths inside them."""
    import fdeflate_amd as fd
    r = np.random.default_rng(6200)
    sizes = [0, 1, 15, 16, 17, 300000, 299999, 65536, 65537] + [int(v) for v in r.integers(0, 300001, 61)]
    assert len(sizes) == 70
    off = np.concatenate([[3], 3 + np.cumsum(sizes)]).astype(np.int64)
    host = r.integers(0, 256, int(off[-1]) + 7, dtype=np.uint8)
    raw = host.tobytes()
    data = gh.dev(host)
    lens = [int(r.integers(0, s + 1)) if k % 2 else s for k, s in enumerate(sizes)]
    for pieces in (None, 1, 7):
        _shape(monkeypatch, pieces, copies)
        crc, st = _crc(fd, data, off)
        assert st.tolist() == [0] * 70
        assert crc.tolist() == [zlib.crc32(raw[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])], pieces
        crc, st = _crc(fd, data, off, lens)
        assert st.tolist() == [0] * 70
        assert crc.tolist() == [zlib.crc32(raw[int(a):int(a) + n]) for a, n in zip(off[:-1], lens)], pieces


def test_crc_one_range_of_256_mib(monkeypatch):
    """256 MiB + 3 bytes next to a range of one byte, from an odd address; with a seed as well."""
    import torch
    import fdeflate_amd as fd
    _shape(monkeypatch)
    t0 = time.time()
    big = (256 << 20) + 3
    g = torch.Generator(device="cuda")
    g.manual_seed(6300)
    data = torch.randint(0, 256, (big + 9,), dtype=torch.uint8, device="cuda", generator=g)
    raw = data.cpu().numpy().tobytes()
    off = np.array([5, 5 + big, 6 + big], dtype=np.int64)
    crc, st = _crc(fd, data, off)
    assert st.tolist() == [0, 0]
    assert crc.tolist() == [zlib.crc32(raw[5:5 + big]), zlib.crc32(raw[5 + big:6 + big])]
    crc, st = _crc(fd, data, off, [big - 1, 1], [0xDEADBEEF, 0xFFFFFFFF])
    assert crc.tolist() == [zlib.crc32(raw[5:4 + big], 0xDEADBEEF), zlib.crc32(raw[5 + big:6 + big], 0xFFFFFFFF)]
    print("256 MiB range: %.1f s" % (time.time() - t0))


def test_crc_seeds_join_type_and_body():
    """A chunk's type and its body as two ranges, the second seeded with the first one's CRC: the CRC of the chunk."""
    import fdeflate_amd as fd
    r = np.random.default_rng(6400)
    bodies = [int(v) for v in r.integers(0, 5000, 200)]
    off = np.concatenate([[1], 1 + np.cumsum([4 + b for b in bodies])]).astype(np.int64)
    host = r.integers(0, 256, int(off[-1]) + 3, dtype=np.uint8)
    raw = host.tobytes()
    data = gh.dev(host)
    whole, st = _crc(fd, data, off)
    types, st1 = _crc(fd, data, off, [4] * 200)
    body_off = np.concatenate([off[:-1] + 4, off[-1:]]).astype(np.int64)   # slot k: from the body of chunk k to the body of chunk k + 1
    joined, st2 = _crc(fd, data, body_off, bodies, types)
    assert st.tolist() == st1.tolist() == st2.tolist() == [0] * 200
    assert joined.tolist() == whole.tolist() == [zlib.crc32(raw[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("pieces", (None, 1))
def test_crc_lengths_that_do_not_fit(pieces, monkeypatch):
    """len[i] above the slot and len[i] == 0xFFFFFFFF: status 2 and CRC 0; the neighbours exact."""
    import fdeflate_amd as fd
    _shape(monkeypatch, pieces)
    r = np.random.default_rng(6500)
    sizes = [100, 37, 0, 5000, 64, 999, 16]
    off = np.concatenate([[2], 2 + np.cumsum(sizes)]).astype(np.int64)
    host = r.integers(0, 256, int(off[-1]) + 5000, dtype=np.uint8)
    raw = host.tobytes()
    lens = [100, 38, 0, 0xFFFFFFFF, 64, 6000, 1]
    crc, st = _crc(fd, gh.dev(host), off, lens, [7] * 7)
    assert st.tolist() == [0, 2, 0, 2, 0, 2, 0]
    assert crc.tolist() == [zlib.crc32(raw[int(a):int(a) + n], 7) if s == 0 else 0 for a, n, s in zip(off[:-1], lens, st.tolist())]
    assert crc[2] == 7           # no bytes: the seed


# ---- pixels -> files ----

def _file_case(r, rb, bpp, depth, colour, shift):
    """The shared images of one width with everything the encode test expects of them."""
    imgs = cm.choose_images(r, rb, bpp, shift=shift)
    width = rb // bpp
    files, types = [], []
    for im in imgs:
        t = cm.choose(im, bpp)[0]
        st, filt = ob.png_filter(im.reshape(-1), rb, bpp, t)
        assert st == 0
        types.append(t)
        files.append(fm.write_file(ob.compress_ultra_fast(filt), width, im.shape[0], depth, colour, crc=zlib.crc32))
    return imgs, types, files


def _pillow_check(png, im, width, depth, colour):
    mode, size, shown = pc.pillow_view(png)
    want_mode, want = pc.pillow_expected(im, width, depth, colour)
    assert (mode, size) == (want_mode, (width, im.shape[0])) and shown == want


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["bpp%d-depth%d" % g[:2] for g in GEOMETRIES])
def test_pixels_to_files_at_every_width_class(geometry):
    """png_encode_files_batch on the shared images of png_choose_model (13 per width, 0 .. 200 rows) at the smallest and
    the largest width of every class of tests/test_gpu_png_choose.py and the three widths above 4096 bytes, into slots
    of exactly png_file_bound from byte 7 of a buffer of fill bytes.  Every file equals the model's framing around the
    oracle's ultra-fast stream of the image filtered with the model's types, and Pillow shows its pixels.  The image of
    no rows gets status 2 (height 0).  Slots 2, 5, 8 and 11 are too small -- by one byte, half, 57 bytes, none at all --:
    status 2, file_len 0, the slot's first 41 bytes untouched, and for the one that is a byte short (the encoder's
    stream still fits) every byte of the slot but the stream.  No byte in front of the first or behind the last slot
    changes."""
    import torch
    import fdeflate_amd as fd
    bpp, depth, colour = geometry
    t0 = time.time()
    r = np.random.default_rng(6600 + 16 * bpp + depth)
    widths = [w for n in gh.CHUNKS for w in sorted(set(gh.widths_of(bpp, n)))] + list(gh.widths_above(bpp, GATE))
    opened = 0
    for k, rb in enumerate(widths):
        assert fd.png_geometry(rb // bpp, depth, colour) == fm.geometry(rb // bpp, depth, colour) == (rb, bpp)
        imgs, types, files = _file_case(r, rb, bpp, depth, colour, k)
        n = len(imgs)
        rows = [im.shape[0] for im in imgs]
        slots = [fd.png_file_bound(nr, rb) for nr in rows]
        small = {}
        for j, i in enumerate(range(2, n, 3)):
            slots[i] = (len(files[i]) - 1, len(files[i]) // 2, 57, 0)[j % 4]
            small[i] = j % 4
        f_off = np.concatenate([[7], 7 + np.cumsum(slots)]).astype(np.int64)
        p_off = np.concatenate([[3], 3 + np.cumsum([im.size for im in imgs])]).astype(np.int64)
        pix = np.zeros(int(p_off[-1]) + 1, dtype=np.uint8)
        for o, im in zip(p_off[:-1], imgs):
            pix[int(o):int(o) + im.size] = im.reshape(-1)
        d_file = torch.full((int(f_off[-1]) + 64,), FILL, dtype=torch.uint8, device="cuda")
        file_len, st, ty = fd.png_encode_files_batch(gh.dev(pix), gh.dev(p_off), d_file, gh.dev(f_off), rb // bpp, depth, colour)
        torch.cuda.synchronize()
        got = d_file.cpu().numpy()
        bad = [i for i in range(n) if rows[i] == 0 or i in small]
        what = (geometry, rb)
        assert st.cpu().tolist() == [2 if i in bad else 0 for i in range(n)], what
        assert _u32(file_len).tolist() == [0 if i in bad else len(files[i]) for i in range(n)], what
        assert np.array_equal(ty.cpu().numpy()[:sum(rows)], np.concatenate(types)), what
        assert (got[:7] == FILL).all() and (got[int(f_off[-1]):] == FILL).all(), what
        for i in range(n):
            slot = got[int(f_off[i]):int(f_off[i + 1])]
            if i not in bad:
                assert slot[:len(files[i])].tobytes() == files[i], (what, i)
                _pillow_check(files[i], imgs[i], rb // bpp, depth, colour)      # (16-bit colour: the high bytes)
                opened += 1
            else:
                assert (slot[:41] == FILL).all(), (what, i)
                if small.get(i) == 0:         # one byte short: the stream is in place, nothing else
                    assert slot[41:].tobytes()[:len(files[i]) - 57] == files[i][41:-16] and (slot[len(files[i]) - 16:] == FILL).all(), (what, i)
    print("bpp %d depth %d: %d widths, %d files opened by Pillow, %.1f s" % (bpp, depth, len(widths), opened, time.time() - t0))


def test_last_slot_too_small_and_frame_alone():
    """The encoder is never given room behind the last file slot: a last slot that is too small leaves the bytes behind
    it alone.  fdh_png_frame_batch by itself: width 0 and an illegal depth / colour pair are refused, idat_len 0,
    0xFFFFFFFF, above 2^31 - 1, a height of 0 and a slot one byte short give status 2 with nothing written."""
    import ctypes as C
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import _lib
    r = np.random.default_rng(6700)
    rb, bpp = 300, 3
    imgs = cm.choose_images(r, rb, bpp, rows=(9, 30, 17))
    p_off = np.concatenate([[0], np.cumsum([im.size for im in imgs])]).astype(np.int64)
    pix = np.concatenate([im.reshape(-1) for im in imgs])
    for last in (0, 30, 57, 300):
        slots = [fd.png_file_bound(9, rb), fd.png_file_bound(30, rb), last]
        f_off = np.concatenate([[1], 1 + np.cumsum(slots)]).astype(np.int64)
        d_file = torch.full((int(f_off[-1]) + 100,), FILL, dtype=torch.uint8, device="cuda")
        file_len, st, _ = fd.png_encode_files_batch(gh.dev(pix), gh.dev(p_off), d_file, gh.dev(f_off), 100, 8, 2)
        torch.cuda.synchronize()
        got = d_file.cpu().numpy()
        assert st.cpu().tolist() == [0, 0, 2] and _u32(file_len)[2] == 0
        assert (got[int(f_off[-1]):] == FILL).all() and got[0] == FILL, last
        assert (got[int(f_off[2]):int(f_off[2]) + min(41, last)] == FILL).all(), last
        for i in range(2):
            f = got[int(f_off[i]):int(f_off[i]) + int(_u32(file_len)[i])].tobytes()
            assert pc.pillow_view(f)[2] == imgs[i].tobytes()
    # the framing call alone
    L = _lib.lib()
    stream = zlib.compress(bytes(5 * 31), 1)
    slot = len(stream) + 57
    f_off = np.arange(7, dtype=np.int64) * slot + 3
    f_off[6] -= 1                                             # the last slot is a byte short
    host = np.full(int(f_off[-1]) + 40, FILL, dtype=np.uint8)
    for o in f_off[:-1]:
        host[int(o) + 41:int(o) + 41 + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    d_file = gh.dev(host)
    idat_len = gh.dev(np.array([len(stream), 0, 0xFFFFFFFF, 0x80000000, len(stream), len(stream)], dtype=np.uint32).view(np.int32))
    height = gh.dev(np.array([5, 5, 5, 5, 0, 5], dtype=np.uint32).view(np.int32))
    lw, flen = _guarded(6)
    sw, st = _guarded(6)
    d_off = gh.dev(f_off)
    args = [C.c_void_p(t.data_ptr()) for t in (d_file, d_off, idat_len, height, flen, st)]
    for width, depth, colour in ((0, 8, 0), (1 << 31, 8, 0), (30, 3, 0), (30, 16, 3), (30, 8, 7)):
        assert L.fdh_png_frame_batch(*args, 6, width, depth, colour, None) == 1
        with pytest.raises(_lib.FdeflateHipError):
            fd.png_frame_batch(d_file, d_off, idat_len, height, width, depth, colour)
    torch.cuda.synchronize()
    assert np.array_equal(d_file.cpu().numpy(), host) and (_u32(st) == GUARD32).all()
    assert L.fdh_png_frame_batch(*args, 6, 30, 8, 0, None) == 0
    torch.cuda.synchronize()
    assert _u32(st).tolist() == [0, 2, 2, 2, 2, 2] and _u32(flen).tolist() == [slot, 0, 0, 0, 0, 0]
    assert _guards_intact(lw, 6) and _guards_intact(sw, 6)
    got = d_file.cpu().numpy()
    want = host.copy()
    want[3:3 + slot] = np.frombuffer(fm.write_file(stream, 30, 5, 8, 0), dtype=np.uint8)
    assert np.array_equal(got, want)
    assert pc.pillow_view(got[3:3 + slot].tobytes()) == ("L", (30, 5), bytes(150))


# ---- files -> pixels ----

def test_pillow_files_to_pixels():
    """Every file of the Pillow-written corpus (level-6 streams in three or more IDAT chunks behind tEXt, pHYs and PLTE
    chunks), three copies a call -- with file_len, and without it and fill bytes behind IEND --: info is the model's, all
    statuses are 0, the pixels are the ones Pillow shows."""
    import torch
    import fdeflate_amd as fd
    for name, png, width, height, depth, colour, pixels in pc.pillow_corpus():
        want_info = fm.scan(png, crc=zlib.crc32).fields()
        host, f_off, f_len = gh.batch_of([png] * 3, fill=FILL)
        for with_len in (True, False):
            pix, pix_off, info, status, png_status = fd.png_decode_files_batch(gh.dev(host), gh.dev(f_off), width, depth, colour,
                                                                               file_len=gh.dev(f_len) if with_len else None)
            torch.cuda.synchronize()
            assert gh.info_rows(fd, info) == [want_info] * 3, (name, with_len)
            assert status.cpu().tolist() == [0] * 3 and png_status.cpu().tolist() == [0] * 3, name
            assert pix_off.cpu().tolist() == [k * len(pixels) for k in range(4)]
            assert pix.cpu().numpy().tobytes() == pixels * 3, (name, with_len)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["bpp%d-depth%d" % g[:2] for g in GEOMETRIES])
def test_own_files_to_pixels(geometry):
    """Files written by png_encode_files_batch, read back by png_decode_files_batch: info is the model's, the pixels
    are the source's."""
    import torch
    import fdeflate_amd as fd
    bpp, depth, colour = geometry
    r = np.random.default_rng(6800 + 16 * bpp + depth)
    for rb in (5 * bpp, 1023 // bpp * bpp, 4099 // bpp * bpp + bpp):
        imgs = [im for im in cm.choose_images(r, rb, bpp, shift=rb) if im.shape[0]]
        n = len(imgs)
        p_off = np.concatenate([[0], np.cumsum([im.size for im in imgs])]).astype(np.int64)
        f_off = np.concatenate([[9], 9 + np.cumsum([fd.png_file_bound(im.shape[0], rb) for im in imgs])]).astype(np.int64)
        d_file = torch.full((int(f_off[-1]) + 16,), FILL, dtype=torch.uint8, device="cuda")
        file_len, st, _ = fd.png_encode_files_batch(gh.dev(np.concatenate([im.reshape(-1) for im in imgs])), gh.dev(p_off), d_file,
                                                    gh.dev(f_off), rb // bpp, depth, colour)
        assert st.cpu().tolist() == [0] * n
        pix, pix_off, info, status, png_status = fd.png_decode_files_batch(d_file, gh.dev(f_off), rb // bpp, depth, colour, file_len=file_len)
        torch.cuda.synchronize()
        got = d_file.cpu().numpy()
        lens = _u32(file_len)
        want = [fm.scan(got[int(o):int(o) + int(m)].tobytes(), crc=zlib.crc32).fields() for o, m in zip(f_off[:-1], lens)]
        assert gh.info_rows(fd, info) == want and all(w[0] == 0 and w[1:3] == (rb // bpp, im.shape[0]) for w, im in zip(want, imgs))
        assert status.cpu().tolist() == [0] * n and png_status.cpu().tolist() == [0] * n
        assert pix_off.cpu().tolist() == p_off.tolist()
        assert pix.cpu().numpy().tobytes() == b"".join(im.tobytes() for im in imgs), (geometry, rb)


def _mixed_batch():
    """Good files of one geometry between one file of every kind of damage, and one good file of another geometry."""
    corpus = pc.pillow_corpus()
    name, png, width, height, depth, colour, pixels = corpus[1]
    other = corpus[4][1]
    files, expect = [png], [(0, 0, 0)]        # (info.status, the same ignoring CRCs, png_status of the decode)
    for what, f, status, status_ignoring, _ in pc.damaged_files(png):
        files += [f, png]
        expect += [(status, status_ignoring, 3), (0, 0, 0)]
    files += [other, png]
    expect += [(0, 0, 7), (0, 0, 0)]
    return files, expect, (width, depth, colour), pixels, png


def test_mixed_batch_every_status():
    """One batch: sound files between one file of every kind of damage (statuses 1 .. 6, several ways each) and a file of
    another geometry (7).  Each file gets exactly its code from the scan (the model's whole record) and from the decode;
    every sound file decodes to Pillow's pixels.  With FDH_PNG_FLAG_IGNORE_CRC the files whose only fault is a CRC field
    read as sound and decode to the same pixels.  The input is not written."""
    import torch
    import fdeflate_amd as fd
    files, expect, (width, depth, colour), pixels, png = _mixed_batch()
    assert {e[0] for e in expect} == {0, 1, 2, 3, 4, 5, 6}
    host, f_off, f_len = gh.batch_of(files, fill=FILL)
    d_file = gh.dev(host)
    for flags in (0, fd.PNG_FLAG_IGNORE_CRC):
        pix, pix_off, info, status, png_status = fd.png_decode_files_batch(d_file, gh.dev(f_off), width, depth, colour, file_len=gh.dev(f_len), flags=flags)
        torch.cuda.synchronize()
        rows = gh.info_rows(fd, info)
        assert rows == [fm.scan(f, ignore_crc=bool(flags), crc=zlib.crc32).fields() for f in files]
        assert [w[0] for w in rows] == [e[1] if flags else e[0] for e in expect]
        got_pix, off = pix.cpu().numpy().tobytes(), pix_off.cpu().tolist()
        whole_idat, exact = fm.scan(png, True, zlib.crc32).idat, 0
        for i, (f, e) in enumerate(zip(files, expect)):
            sound = (e[1] if flags else e[0]) == 0 and e[2] != 7
            if not sound:
                assert png_status[i].item() == e[2] and off[i + 1] == off[i], (i, e)
            elif fm.scan(f, True, zlib.crc32).idat == whole_idat:
                # a sound file, or one whose only fault is a CRC field that is being ignored
                assert (status[i].item(), png_status[i].item()) == (0, 0), (i, e)
                assert got_pix[off[i]:off[i + 1]] == pixels, (i, e)
                exact += 1
        assert exact == sum(1 for e in expect if e == (0, 0, 0)) + (4 if flags else 0)
        assert sum(1 for i in range(len(files)) if off[i + 1] > off[i]) >= (len(files) + 1) // 2
    assert np.array_equal(d_file.cpu().numpy(), host)


def test_gather_slots_and_guards():
    """The two-step calls on the mixed batch: comp slots of exactly idat_bytes at odd offsets in a buffer of fill bytes,
    one sound file's slot a byte short (8) and one empty (8).  comp_len and png_status are exact, every gathered stream
    is the model's concatenation, and no byte outside the gathered streams changes."""
    import torch
    import fdeflate_amd as fd
    files, expect, (width, depth, colour), pixels, png = _mixed_batch()
    host, f_off, f_len = gh.batch_of(files, fill=FILL)
    d_file, d_off = gh.dev(host), gh.dev(f_off)
    info = fd.png_scan_files_batch(d_file, d_off, gh.dev(f_len))
    model = [fm.scan(f, crc=zlib.crc32) for f in files]
    sound = [i for i, e in enumerate(expect) if e == (0, 0, 0)]
    short, empty = sound[1], sound[3]
    sizes = [m.idat_bytes if m.status == 0 else 3 for m in model]
    sizes[short] -= 1
    sizes[empty] = 0
    c_off = np.concatenate([[11], 11 + np.cumsum(sizes)]).astype(np.int64)
    want = np.full(int(c_off[-1]) + 32, FILL, dtype=np.uint8)
    want_len, want_st = [], []
    for i, (m, e) in enumerate(zip(model, expect)):
        st = 3 if m.status else (7 if e[2] == 7 else (8 if i in (short, empty) else 0))
        want_st.append(st)
        want_len.append(0 if st else m.idat_bytes)
        if st == 0:
            want[int(c_off[i]):int(c_off[i]) + m.idat_bytes] = np.frombuffer(m.idat, dtype=np.uint8)
    comp = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
    lw, comp_len = _guarded(len(files))
    sw, st = _guarded(len(files))
    fd.png_gather_idat_batch(d_file, d_off, info, comp, gh.dev(c_off), width, depth, colour, comp_len=comp_len, png_status=st)
    torch.cuda.synchronize()
    assert _u32(st).tolist() == want_st and _u32(comp_len).tolist() == want_len
    assert _guards_intact(lw, len(files)) and _guards_intact(sw, len(files))
    assert np.array_equal(comp.cpu().numpy(), want)
    assert np.array_equal(d_file.cpu().numpy(), host)


# ---- at scale ----

def test_round_trip_of_4096_images():
    """4096 images of 64 rows x 1024 bytes (RGBA, 8 bits) go pixels -> files -> pixels on the device and come back equal
    (one wavefront per file in every kernel).  Of 64 files, every 64th from file 5, every chunk's CRC is checked with
    zlib and the whole record with the model; Pillow opens 8 of them."""
    import torch
    import fdeflate_amd as fd
    t0 = time.time()
    n, rows, rb, width = 4096, 64, 1024, 256
    g = torch.Generator(device="cuda")
    g.manual_seed(6900)
    x = torch.arange(rb, device="cuda").view(1, 1, rb)
    y = torch.arange(rows, device="cuda").view(1, rows, 1)
    i = torch.arange(n, device="cuda").view(n, 1, 1)
    noise = torch.randint(0, 4, (n, rows, rb), device="cuda", generator=g)
    pix = ((x // 4 * (i % 7 + 1) + y * 3 + i + noise) & 0xFF).to(torch.uint8)
    pix[:, 40:48] = torch.randint(0, 256, (n, 8, rb), device="cuda", generator=g).to(torch.uint8)
    pix = pix.view(-1)
    p_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (rows * rb)
    slot = fd.png_file_bound(rows, rb) + 3
    f_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * slot + 1
    d_file = torch.full((n * slot + 2,), FILL, dtype=torch.uint8, device="cuda")
    file_len, st, _ = fd.png_encode_files_batch(pix, p_off, d_file, f_off, width, 8, 6)
    assert int(st.abs().sum()) == 0
    back, back_off, info, status, png_status = fd.png_decode_files_batch(d_file, f_off, width, 8, 6, file_len=file_len)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0 and int(info[:, 0].abs().sum()) == 0
    assert torch.equal(back_off, p_off) and torch.equal(back, pix)
    lens = _u32(file_len)
    rows_info = gh.info_rows(fd, info)
    opened = 0
    for k in range(5, n, 64):
        f = d_file[k * slot + 1:k * slot + 1 + int(lens[k])].cpu().numpy().tobytes()
        assert [t for t, _ in pc.chunks_of(f)] == [b"IHDR", b"IDAT", b"IEND"]       # (chunks_of checks every CRC with zlib)
        assert rows_info[k] == fm.scan(f, crc=zlib.crc32).fields() == (0, width, rows, 8, 6, 0, len(f) - 57, 1, 33, 3)
        if k % 512 == 5:
            assert pc.pillow_view(f) == ("RGBA", (width, rows), pix[k * rows * rb:(k + 1) * rows * rb].cpu().numpy().tobytes())
            opened += 1
    assert opened == 8
    assert d_file[0].item() == FILL and d_file[-1].item() == FILL
    print("round trip of %d images: %.1f s" % (n, time.time() - t0))
