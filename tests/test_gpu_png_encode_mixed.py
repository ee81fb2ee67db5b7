"""PNG encode of mixed batches on the GPU (include/fdeflate_hip.h, "PNG encode: mixed batches"): every mixed call against
the per-geometry call it derives from, byte for byte and status for status on the device, against the Python models
(tests/png_encode_mixed_model.py, png_pack_model.py, png_choose_model.py, the oracle's ultra-fast encoder), and the
pipeline against Pillow and against the mixed decode pipeline.  Bad inputs are refused by status: one wrong image among
good ones, whose bytes stay what they are."""
import zlib

import numpy as np
import pytest

import png_choose_model as cm
import png_corpus as pc
import png_encode_mixed_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_mixed_model as mm
import png_model
import png_pack_model as pm
from png_gpu_harness import GUARD, HEIGHTS, PASSED_ON

pytestmark = pytest.mark.gpu

GUARD_WORD = 0x5A5A5A5A


class Picture:
    """One image of a batch: its pixel words, the pair it is written with, and what analysis says about it."""

    def __init__(self, px, width, height, depth, colour):
        self.px, self.width, self.height, self.depth, self.colour = np.ascontiguousarray(px, dtype=np.uint32), width, height, depth, colour
        assert self.px.size == width * height
        self.pal, self.count, self.trns = [0xFF000000] * 256, 0, 0
        if colour == 3:
            _, self.pal, self.count, self.trns, _ = pm.analyse(self.px.view(np.uint8), width, 256)
        self.rb, self.bpp = fm.geometry(width, depth, colour)
        st, d, c, self.pix_size, self.types_size, self.prefix, self.file_size = em.plan(
            mm.record(width, height, depth, colour), self.count, self.trns, 0, 0)
        assert (st, d, c) == (0, depth, colour)

    def record(self):
        return mm.words(mm.record(self.width, self.height, self.depth, self.colour))


def representable(r, width, height, depth, colour):
    if colour == 3:
        colours = int(r.integers(1, (1 << depth) + 1))
        px = pc.palette_image(r, width, height, colours, int(r.integers(0, colours + 1))).view(np.uint32)
    else:
        px = gh.random_rgba(r, width, height, depth, colour)
    return Picture(px, width, height, depth, colour)


_CROSS = []


def cross_product():
    """All fifteen pairs times gh.PACK_WIDTHS times HEIGHTS, built once."""
    if not _CROSS:
        r = np.random.default_rng(12200)
        for depth, colour in fm.PAIRS:
            for width in gh.PACK_WIDTHS:
                for height in HEIGHTS:
                    _CROSS.append(representable(r, width, height, depth, colour))
    return _CROSS


class Mixed:
    """A batch of pictures in one order, every buffer between guard bytes, and the four mixed calls on it."""

    def __init__(self, pictures, file_sizes=None):
        self.p = pictures
        self.n = len(pictures)
        self.r_off = gh.offsets([4 * p.px.size for p in pictures], 5)
        self.p_off = gh.offsets([p.pix_size for p in pictures], 3)
        self.t_off = gh.offsets([p.types_size for p in pictures], 1)
        self.f_off = gh.offsets(file_sizes or [p.file_size for p in pictures], 7)
        self.e_off = self.f_off.copy()
        self.e_off[:self.n] += [p.prefix for p in pictures]
        self.e_off[self.n] = max(self.f_off[self.n] - 16, self.e_off[self.n - 1]) if self.n else self.f_off[0]
        self.rgba = np.full(int(self.r_off[-1]) + 9, GUARD, dtype=np.uint8)
        for k, p in enumerate(pictures):
            self.rgba[self.r_off[k]:self.r_off[k + 1]] = p.px.view(np.uint8)
        self.info = np.asarray([p.record() for p in pictures], dtype=np.uint32).reshape(-1, 8)
        self.pal = np.asarray([p.pal for p in pictures], dtype=np.uint32).reshape(-1, 256)
        self.colour = np.asarray([[p.count, 0, 0, 0] for p in pictures], dtype=np.uint32).reshape(-1, 4)
        self.trns = np.asarray([p.trns for p in pictures], dtype=np.uint32)

    def device(self):
        import torch
        self.d_rgba, self.d_info = gh.dev(self.rgba), gh.words(self.info)
        self.d_pal, self.d_colour, self.d_trns = gh.words(self.pal), gh.words(self.colour), gh.words(self.trns)
        self.d_r_off, self.d_p_off, self.d_t_off = gh.dev(self.r_off), gh.dev(self.p_off), gh.dev(self.t_off)
        self.d_f_off, self.d_e_off = gh.dev(self.f_off), gh.dev(self.e_off)
        full = lambda size: torch.full((int(size),), GUARD, dtype=torch.uint8, device="cuda")
        self.pix, self.types, self.file = full(self.p_off[-1] + 11), full(self.t_off[-1] + 11), full(self.f_off[-1] + 11)
        return self

    def status(self):
        import torch
        return torch.full((self.n + 16,), GUARD_WORD, dtype=torch.int32, device="cuda")

    def run(self, fd, pal=True, upstream=(None, None, None), types=None):
        """pack, choose, fused encode, frame -> the four statuses, out_len and file_len (lists); guards checked."""
        import torch
        self.device()
        st = [self.status() for _ in range(6)]
        view = lambda t: t[8:8 + self.n]
        up = [None if u is None else gh.words(u) for u in upstream]
        fd.png_pack_mixed_batch(self.d_rgba, self.d_r_off, self.pix, self.d_p_off, self.d_info, pal=self.d_pal if pal else None,
                                colour=self.d_colour if pal else None, upstream=up[0], png_status=view(st[0]))
        fd.png_choose_filters_mixed_batch(self.pix, self.d_p_off, self.types, self.d_t_off, self.d_info, upstream=up[1], png_status=view(st[1]))
        if types is not None:
            self.types[self.t_off[0]:self.t_off[-1]] = gh.dev(types)
        fd.png_filter_deflate_ultrafast_mixed_batch(self.pix, self.d_p_off, self.types, self.d_t_off, self.file, self.d_e_off, self.d_info,
                                                    upstream=up[2], out_len=view(st[2]), png_status=view(st[3]))
        idat = torch.where(view(st[3]) != 0, torch.zeros_like(view(st[2])), view(st[2]))
        fd.png_frame_mixed_batch(self.file, self.d_f_off, idat, self.d_info, self.d_pal, self.d_colour, self.d_trns,
                                 file_len=view(st[4]), png_status=view(st[5]))
        torch.cuda.synchronize()
        assert np.array_equal(self.d_rgba.cpu().numpy(), self.rgba)
        got = []
        for s in st:
            s = s.cpu().numpy()
            assert (s[:8] == GUARD_WORD).all() and (s[8 + self.n:] == GUARD_WORD).all()
            got.append(s[8:8 + self.n].tolist())
        self.h_pix, self.h_types, self.h_file = self.pix.cpu().numpy(), self.types.cpu().numpy(), self.file.cpu().numpy()
        for buf, off in ((self.h_pix, self.p_off), (self.h_types, self.t_off), (self.h_file, self.f_off)):
            assert (buf[:off[0]] == GUARD).all() and (buf[off[-1]:] == GUARD).all()
        self.packed, self.chosen, self.out_len, self.encoded, self.file_len, self.framed = got
        return self

    def slot(self, which, k):
        buf, off = {"pix": (self.h_pix, self.p_off), "types": (self.h_types, self.t_off), "file": (self.h_file, self.f_off)}[which]
        return buf[off[k]:off[k + 1]]

    def png(self, k):
        return self.h_file[self.f_off[k]:self.f_off[k] + self.file_len[k]].tobytes()


_REFERENCE = {}
_KEPT = []          # (the pictures behind _REFERENCE's keys stay alive, so that no other picture gets their id)


def reference(fd, pictures):
    """The per-geometry calls on every group of pictures with one (depth, colour, width) -> {id(picture): (pix, types, stream,
    file)} as bytes, computed once."""
    import torch
    groups = {}
    for p in pictures:
        if id(p) not in _REFERENCE:
            groups.setdefault((p.depth, p.colour, p.width), []).append(p)
    for (depth, colour, width), group in groups.items():
        n = len(group)
        rb, bpp = group[0].rb, group[0].bpp
        r_off = gh.offsets([4 * p.px.size for p in group])
        p_off, t_off = gh.offsets([p.pix_size for p in group]), gh.offsets([p.height for p in group])
        o_off = gh.offsets([p.file_size for p in group])
        rgba = gh.dev(np.concatenate([p.px.view(np.uint8) for p in group]))
        pix = torch.zeros(int(p_off[-1]), dtype=torch.uint8, device="cuda")
        types = torch.zeros(int(t_off[-1]), dtype=torch.uint8, device="cuda")
        out = torch.zeros(int(o_off[-1]), dtype=torch.uint8, device="cuda")
        d_p_off, d_t_off = gh.dev(p_off), gh.dev(t_off)
        pal = gh.words([p.pal for p in group]) if colour == 3 else None
        col = gh.words([[p.count, 0, 0, 0] for p in group]) if colour == 3 else None
        st1 = fd.png_pack_batch(rgba, gh.dev(r_off), pix, d_p_off, width, depth, colour, pal=pal, colour=col)
        st2 = fd.png_choose_filters_batch(pix, d_p_off, types, d_t_off, rb, bpp)
        out_len, st3 = fd.png_filter_deflate_ultrafast_batch(pix, d_p_off, types, d_t_off, out, gh.dev(o_off), rb, bpp)
        assert st1.cpu().tolist() == [0] * n and st2.cpu().tolist() == [0] * n and st3.cpu().tolist() == [0] * n
        h_pix, h_types, h_out, lens = pix.cpu().numpy(), types.cpu().numpy(), out.cpu().numpy(), out_len.cpu().tolist()
        for k, p in enumerate(group):
            stream = h_out[o_off[k]:o_off[k] + lens[k]]
            # the framing of the image alone, with its own palette sizes: the stream goes where the prefix ends
            prefix = p.prefix
            slot = torch.zeros(prefix + lens[k] + 16, dtype=torch.uint8, device="cuda")
            slot[prefix:prefix + lens[k]] = gh.dev(stream)
            f_off = gh.dev(np.asarray([0, slot.numel()], dtype=np.int64))
            idat, height = gh.words([lens[k]]), gh.words([p.height])
            if colour == 3:
                f_len, st4 = fd.png_frame_palette_batch(slot, f_off, idat, height, gh.words([p.pal]), gh.words([[p.count, 0, 0, 0]]), gh.words([p.trns]),
                                                        width, depth, p.count, p.trns)
            else:
                f_len, st4 = fd.png_frame_batch(slot, f_off, idat, height, width, depth, colour)
            assert st4.cpu().tolist() == [0] and f_len.cpu().tolist() == [slot.numel()]
            _KEPT.append(p)
            _REFERENCE[id(p)] = (h_pix[p_off[k]:p_off[k + 1]].tobytes(), h_types[t_off[k]:t_off[k + 1]].tobytes(), stream.tobytes(),
                                 slot.cpu().numpy().tobytes())
    return _REFERENCE


def check_against_reference(fd, b, skip=()):
    ref = reference(fd, [p for k, p in enumerate(b.p) if k not in skip])
    for k, p in enumerate(b.p):
        if k in skip:
            continue
        pix, types, stream, file = ref[id(p)]
        what = (k, p.depth, p.colour, p.width, p.height)
        assert (b.packed[k], b.chosen[k], b.encoded[k], b.framed[k]) == (0, 0, 0, 0), what
        assert b.slot("pix", k).tobytes() == pix, what
        assert b.slot("types", k).tobytes() == types, what
        assert b.out_len[k] == len(stream) and b.file_len[k] == len(file), what
        assert b.png(k) == file, what


# ---- the cross product ----

@pytest.mark.parametrize("order", [0, 1])
def test_every_pair_width_and_height_in_one_batch(order):
    """All fifteen pairs times every width and height as encodable records in ONE shuffled batch between guard bytes: the
    packed rows, the filter types, the zlib stream and the file of every image are the per-geometry calls' on its group,
    every status 0, nothing outside the slots written; in two orders."""
    import fdeflate_amd as fd
    pictures = cross_product()
    perm = np.random.default_rng(12300 + order).permutation(len(pictures))
    b = Mixed([pictures[k] for k in perm]).run(fd)
    check_against_reference(fd, b)


def test_every_seventh_image_against_the_models():
    """... and the same batch against plain Python: png_pack_model, png_choose_model, the oracle's ultra-fast encoder
    over the filtered rows, and the model's exact-palette writer."""
    import fdeflate_amd as fd
    import oracle_binding as ob
    pictures = cross_product()
    perm = np.random.default_rng(12300).permutation(len(pictures))[::7]
    b = Mixed([pictures[k] for k in perm]).run(fd)
    for k, p in enumerate(b.p):
        what = (k, p.depth, p.colour, p.width, p.height)
        want, st = pm.pack(p.px.view(np.uint8), p.width, p.depth, p.colour, p.pal, p.count or 256)
        assert st == 0 and b.slot("pix", k).tobytes() == want, what
        rows = np.frombuffer(want, dtype=np.uint8).reshape(p.height, p.rb)
        types, _ = cm.choose(rows, p.bpp)
        assert b.slot("types", k).tolist() == types.tolist(), what
        idat = ob.compress_ultra_fast(png_model.filter_rows(rows, p.bpp, types.tolist()).tobytes())
        assert b.png(k) == em.write_file(idat, p.width, p.height, p.depth, p.colour, p.pal, p.count, p.trns, zlib.crc32), what
        assert pc.pillow_rgba(b.png(k)) == p.px.view(np.uint8).tobytes() or p.depth == 16, what


# ---- the plan on the device ----

def _chosen_pictures():
    r = np.random.default_rng(12400)
    out = []
    for width, height in ((37, 29), (64, 17), (5, 3)):
        out += [(name, px, width, height) for name, px, _, _ in pc.kinds(r, width, height)]
    two = np.asarray([0xFF000000, 0xFFFFFFFF], dtype=np.uint32)
    for side in (1, 2):                                             # the palette loses to its own chunks
        out.append(("two-greys", two[r.integers(0, 2, side * side)].view(np.uint8), side, side))
        out.append(("two-colours", (two ^ 0xFF)[r.integers(0, 2, side * side)].view(np.uint8), side, side))
    greys = np.asarray([0xFF111111, 0xFF222222, 0xFF444444, 0xFF777777], dtype=np.uint32)
    for height in (11, 12, 13):                                     # grey-4 and palette-2 tie at 8 x 12
        px = greys[r.integers(0, 4, 8 * height)]
        px[:4] = greys
        out.append(("tie", px.view(np.uint8), 8, height))
    out.append(("many", r.integers(0, 1 << 32, 40 * 40, dtype=np.uint64).astype(np.uint32).view(np.uint8), 40, 40))
    return out


@pytest.mark.parametrize("allowed", [0, 1 << 6, (1 << 3) | (1 << 6), (1 << 0) | (1 << 2), (1 << 4) | (1 << 2) | (1 << 3), 1 << 3])
def test_analyse_and_plan_choose_what_the_model_chooses(allowed):
    """Pictures that are grey-1 / 2 / 4 / 8, palette-1 / 2 / 4 / 8, grey-alpha, RGB and RGBA by construction, the tie, the
    palettes that lose, and one of more than 256 colours, as dimension records through analyse_mixed and plan_batch: the
    analysis is the model's, the records and sizes the model's plan of it, under every mask."""
    import torch
    import fdeflate_amd as fd
    cases = _chosen_pictures()
    n = len(cases)
    r_off = gh.offsets([px.size for _, px, _, _ in cases], 3)
    rgba = np.full(int(r_off[-1]) + 5, GUARD, dtype=np.uint8)
    for k, (_, px, _, _) in enumerate(cases):
        rgba[r_off[k]:r_off[k + 1]] = px
    info = fd.png_encode_records(gh.words([c[2] for c in cases]), gh.words([c[3] for c in cases]))
    pal, colour, trns, summary, analysed = fd.png_analyse_mixed_batch(gh.dev(rgba), gh.dev(r_off), info)
    before = info.clone()
    sizes = fd.png_encode_plan_batch(info, colour, trns, summary, analysed, allowed)
    torch.cuda.synchronize()
    got = [t.cpu().tolist() for t in sizes]
    h_info, h_pal = info.cpu().numpy().view(np.uint32), pal.cpu().numpy().view(np.uint32)
    h_colour, h_trns, h_summary, h_analysed = colour.cpu().tolist(), trns.cpu().tolist(), summary.cpu().tolist(), analysed.cpu().tolist()
    winners = set()
    for k, (name, px, width, height) in enumerate(cases):
        a_st, a_pal, count, trns_len, summ = pm.analyse(px, width, 256)
        assert (h_analysed[k], h_summary[k]) == (a_st, summ), name
        if a_st == 0:
            assert (h_colour[k], h_trns[k], h_pal[k].tolist()) == ([count, 0, 0, 0], trns_len, a_pal), name
        st, depth, c, pix, types, prefix, size = em.plan(mm.record(width, height, 0, 0), count, trns_len, summ, a_st, allowed)
        assert (got[4][k], got[0][k], got[1][k], got[2][k], got[3][k]) == (st, pix, types, prefix, size), (name, allowed)
        want = mm.words(mm.record(width, height, depth, c))[:4] + [0, 0, 0, 0]
        assert h_info[k].tolist() == want, (name, allowed)
        if st == 0:
            winners.add((name, depth, c))
    if allowed == 0:
        assert {("grey1", 1, 0), ("grey8", 8, 0), ("palette1", 1, 3), ("palette8", 8, 3), ("grey-alpha", 8, 4), ("rgb", 8, 2), ("rgba", 8, 6),
                ("two-greys", 1, 0), ("two-colours", 8, 2), ("tie", 4, 0), ("tie", 2, 3), ("many", 8, 6)} <= winners, winners
    # every output is nullable, and an encodable record keeps its pair
    fd.png_encode_plan_batch(before, colour, trns, summary, analysed, allowed, pix_size=None, types_size=None, prefix=None, file_size=None)
    torch.cuda.synchronize()
    assert torch.equal(before, info)
    again = fd.png_encode_plan_batch(info, colour, trns, summary, analysed, allowed)
    torch.cuda.synchronize()
    assert torch.equal(before, info) and [t.cpu().tolist() for t in again] == got


# ---- refusals ----

def _some_pictures(seed, extra=()):
    r = np.random.default_rng(seed)
    shapes = [(8, 2, 33, 5), (1, 0, 9, 3), (4, 3, 31, 66), (16, 6, 5, 2), (8, 4, 64, 1), (2, 3, 7, 7), (8, 3, 40, 9)]
    return [representable(r, w, h, d, c) for d, c, w, h in shapes] + list(extra)


def test_one_wrong_image_among_good_ones():
    """A record of neither kind, interlace 1, each slot off by one, a file slot one byte too small, a pixel the pair cannot
    hold: the image gets its status from the first call that can see the fault, nothing is written for it from there on,
    and its neighbours are bit-exact."""
    import fdeflate_amd as fd
    good = _some_pictures(12500)
    n = len(good)

    def batch(**kw):
        return Mixed(list(good), **kw)

    # records
    for word3, name in ((8 | 1 << 8, "pair"), (8 | 2 << 8 | 1 << 16, "interlace"), (0, "dimension")):
        b = batch()
        b.info[0, 3] = word3
        b.run(fd)
        assert (b.packed[0], b.chosen[0], b.encoded[0], b.framed[0], b.out_len[0], b.file_len[0]) == (3, 3, 3, 3, 0, 0), name
        assert (b.slot("pix", 0) == GUARD).all() and (b.slot("types", 0) == GUARD).all() and (b.slot("file", 0) == GUARD).all(), name
        check_against_reference(fd, b, skip=(0,))
    b = batch()
    b.info[3, 0] = 6                                  # a scan finding
    b.run(fd)
    assert (b.packed[3], b.chosen[3], b.encoded[3], b.framed[3]) == (3, 3, 3, 3)
    check_against_reference(fd, b, skip=(3,))
    # slots: rgba one byte short (2 from pack; choose and the encoder run on the unwritten pix slot), pix, types
    for which in ("r_off", "p_off", "t_off"):
        b = batch()
        getattr(b, which)[2:] += 1                    # image 1 one byte longer, the rest moved
        if which == "r_off":
            b.rgba = np.concatenate([b.rgba[:b.r_off[2] - 1], [GUARD], b.rgba[b.r_off[2] - 1:]]).astype(np.uint8)
        b.run(fd)
        want = {"r_off": (2, 0, 0), "p_off": (2, 2, 2), "t_off": (0, 2, 2)}[which]
        assert (b.packed[1], b.chosen[1], b.encoded[1]) == want, which
        if which != "r_off":
            assert b.out_len[1] == 0 and b.framed[1] == 2 and b.file_len[1] == 0 and (b.slot("file", 1) == GUARD).all()
        if which == "p_off":
            assert (b.slot("pix", 1) == GUARD).all() and (b.slot("types", 1) == GUARD).all()
        check_against_reference(fd, b, skip=(1,))
    # a file slot one byte too small: in the middle of the batch the encoder's slot reaches into the next file's prefix, so
    # the stream is whole and the framing refuses (2); at the end the encoder's slot is too small as well (0xFFFFFFFF)
    ref = reference(fd, good)
    for k in (4, n - 1):
        sizes = [p.file_size for p in good]
        sizes[k] = len(ref[id(good[k])][3]) - 1
        b = batch(file_sizes=sizes).run(fd)
        assert b.encoded[k] == 0 and b.out_len[k] & 0xFFFFFFFF == (0xFFFFFFFF if k == n - 1 else len(ref[id(good[k])][2])), k
        assert (b.framed[k], b.file_len[k]) == (2, 0), k
        check_against_reference(fd, b, skip=(k,))
    # a pixel the pair cannot hold
    r = np.random.default_rng(12501)
    px = gh.random_rgba(r, 33, 5, 8, 0)
    spoilt = Picture(px, 33, 5, 8, 0)
    spoilt.px = px.copy()
    spoilt.px[77] = 0xFF010000
    b = Mixed(good[:3] + [spoilt] + good[3:]).run(fd)
    assert b.packed[3] == 13
    check_against_reference(fd, b, skip=(3,))


def test_upstream_at_each_call_null_palette_colours_and_filter_types():
    import torch
    import fdeflate_amd as fd
    good = _some_pictures(12600)
    n = len(good)
    for call in range(3):
        up = [None, None, None]
        up[call] = [PASSED_ON if k == 2 else 0 for k in range(n)]
        b = Mixed(list(good)).run(fd, upstream=tuple(up))
        got = (b.packed[2], b.chosen[2], b.encoded[2])
        assert got[call] == PASSED_ON and all(g == 0 for g in got[:call]), (call, got)
        if call == 0:
            assert (b.slot("pix", 2) == GUARD).all()
        if call == 1:
            assert (b.slot("types", 2) == GUARD).all()
        if call == 2:
            assert b.out_len[2] == 0 and b.framed[2] == 2 and (b.slot("file", 2) == GUARD).all()
        check_against_reference(fd, b, skip=(2,))
    # analyse: upstream, more colours than max_colours, a slot off by one, a record of neither kind
    b = Mixed(list(good)).device()
    up = gh.words([0, PASSED_ON] + [0] * (n - 2))
    info = b.d_info.clone()
    info[4, 2] += 1                                   # one row more than the slot holds
    info[5, 3] = 8 | 5 << 8
    pal, colour, trns, summary, st = fd.png_analyse_mixed_batch(b.d_rgba, b.d_r_off, info, max_colours=16, upstream=up)
    torch.cuda.synchronize()
    want = [pm.analyse(p.px.view(np.uint8), p.width, 16) for p in good]
    expect = [w[0] for w in want]
    expect[1], expect[4], expect[5] = PASSED_ON, 2, 3
    assert st.cpu().tolist() == expect and 12 in expect
    for k, w in enumerate(want):
        if expect[k] == 0:
            assert (colour[k, 0].item(), trns[k].item(), summary[k].item()) == (w[2], w[3], w[4])
            assert pal[k].cpu().numpy().view(np.uint32).tolist() == w[1]
        elif expect[k] == 12:
            assert summary[k].item() == w[4]
    # pal null: an image of colour type 3 is 10, the others are packed
    b = Mixed(list(good)).run(fd, pal=False)
    for k, p in enumerate(good):
        assert b.packed[k] == (10 if p.colour == 3 else 0)
        if p.colour != 3:
            assert b.slot("pix", k).tobytes() == reference(fd, good)[id(p)][0]
    # a filter type 5 handed to the fused encoder
    types = np.concatenate([np.frombuffer(reference(fd, good)[id(p)][1], dtype=np.uint8) for p in good]).copy()
    at = int(sum(p.height for p in good[:2])) + 40
    types[at] = 5
    b = Mixed(list(good)).run(fd, types=types)
    assert (b.encoded[2], b.out_len[2], b.framed[2]) == (1, 0, 2) and (b.slot("file", 2) == GUARD).all()
    check_against_reference(fd, b, skip=(2,))


def test_more_images_than_the_launch_thresholds_one_and_none():
    """5000 small images (above kFillWaves: the launch shapes change), one image, no image."""
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(12700)
    few = [representable(r, w, h, d, c) for (d, c), w, h in zip(fm.PAIRS, (1, 2, 3, 5, 7, 8, 9, 11, 13, 16, 17, 4, 6, 10, 12), (1, 2, 3) * 5)]
    pictures = [few[k % len(few)] for k in range(5000)]
    b = Mixed(pictures).run(fd)
    ref = reference(fd, few)
    assert b.packed == b.chosen == b.encoded == b.framed == [0] * 5000
    for k in list(range(0, 5000, 97)) + [4999]:
        assert b.png(k) == ref[id(pictures[k])][3], k
    lens = np.asarray(b.file_len)
    assert (lens == np.asarray([len(ref[id(p)][3]) for p in pictures])).all()
    b = Mixed(few[7:8]).run(fd)
    check_against_reference(fd, b)
    # n == 0: success, nothing touched, null pointers welcome
    e64, e32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    e8 = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert fd.png_pack_mixed_batch(e8, e64, e8, e64, e32, png_status=e32).numel() == 0
    assert fd.png_choose_filters_mixed_batch(e8, e64, e8, e64, e32, png_status=e32).numel() == 0
    assert fd.png_filter_deflate_ultrafast_mixed_batch(e8, e64, e8, e64, e8, e64, e32, out_len=e32, png_status=e32)[0].numel() == 0
    assert fd.png_frame_mixed_batch(e8, e64, e32, e32, file_len=e32, png_status=e32)[0].numel() == 0
    assert fd.png_encode_plan_batch(e32, png_status=e32)[4].numel() == 0
    out = fd.png_encode_mixed_rgba_files_batch(e8[:0], e64, e32, e32)
    assert out[2].numel() == 0 and out[3].numel() == 0


# ---- the pipeline ----

def _ragged(seed):
    r = np.random.default_rng(seed)
    out = []
    for width, height in ((37, 29), (64, 17), (5, 3), (341, 64), (1, 1), (2, 2), (1023, 3)):
        out += [(name, px, width, height, depth, colour) for name, px, depth, colour in pc.kinds(r, width, height)]
    order = r.permutation(len(out))
    return [out[k] for k in order]


def _collection(cases):
    r_off = gh.offsets([c[1].size for c in cases])
    rgba = np.concatenate([c[1] for c in cases]).astype(np.uint8)
    return gh.dev(rgba), gh.dev(r_off), gh.words([c[2] for c in cases]), gh.words([c[3] for c in cases])


def test_ragged_collection_end_to_end():
    """A ragged collection through png_encode_mixed_rgba_files_batch: every file is the model's writer's around the
    oracle's stream with the model's filter types, has the planned pair in its IHDR, opens in Pillow to the input, and
    png_decode_mixed_files_rgba_batch gives the input pictures back."""
    import torch
    import fdeflate_amd as fd
    import oracle_binding as ob
    cases = _ragged(12800)
    rgba, r_off, width, height = _collection(cases)
    file, f_off, f_len, st, info = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(cases)
    host, offs, lens = file.cpu().numpy(), f_off.cpu().tolist(), f_len.cpu().tolist()
    fields = info.cpu().numpy().view(np.uint32)
    for k, (name, px, w, h, _, _) in enumerate(cases):
        png = host[offs[k]:offs[k] + lens[k]].tobytes()
        choose = lambda rows, bpp: cm.choose(rows, bpp)[0].tolist()
        m_st, want, depth, colour = em.encode(px.tobytes(), w, h, compress=ob.compress_ultra_fast, choose=choose)
        assert m_st == 0 and png == want, (k, name, w, h)
        scan = fm.scan(png, crc=zlib.crc32)
        assert (scan.status, scan.width, scan.height, scan.bit_depth, scan.colour_type) == (0, w, h, depth, colour), (k, name)
        assert fields[k, 3] == depth | colour << 8 and offs[k + 1] - offs[k] >= lens[k]
        assert pc.pillow_rgba(png) == px.tobytes(), (k, name)
    back, back_off, _, status, png_status = fd.png_decode_mixed_files_rgba_batch(file, f_off, file_len=f_len)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(cases) and png_status.cpu().tolist() == [0] * len(cases)
    assert torch.equal(back_off, r_off) and torch.equal(back, rgba)
    # a mask: nothing but RGB and RGBA
    _, _, f_len2, st2, info2 = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height, allowed=(1 << 2) | (1 << 6))
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [0] * len(cases)
    pairs = {(int(w3) & 0xFF, (int(w3) >> 8) & 0xFF) for w3 in info2.cpu().numpy().view(np.uint32)[:, 3]}
    assert pairs == {(8, 2), (8, 6)}


@pytest.mark.parametrize("pair", [(8, 2), (16, 6), (1, 0), (8, 4), (4, 3), (8, 3)], ids=lambda p: "depth%d-colour%d" % p)
def test_forced_pair_against_the_per_geometry_pipeline(pair):
    """pairs= forced to one geometry: the IDAT streams are png_encode_rgba_files_batch's; a palette file differs only in
    its PLTE / tRNS, which are not padded.  A picture the pair cannot hold gets its status and no file."""
    import torch
    import fdeflate_amd as fd
    depth, colour = pair
    r = np.random.default_rng(12900 + 64 * colour + depth)
    width, heights = 37, (1, 5, 70, 3)
    images = [representable(r, width, h, depth, colour) for h in heights]
    spoilt = 0xFF010203 if colour != 2 and (depth, colour) != (16, 6) and colour != 3 else None
    rgba = np.concatenate([p.px.view(np.uint8) for p in images])
    r_off = gh.offsets([4 * p.px.size for p in images])
    d_rgba, d_off = gh.dev(rgba), gh.dev(r_off)
    w, h = gh.words([width] * 4), gh.words(list(heights))
    file, f_off, f_len, st, info = fd.png_encode_mixed_rgba_files_batch(d_rgba, d_off, w, h, pairs=pair)
    extra = fd.png_palette_file_prefix(1 << depth, 1 << depth) - 41 if colour == 3 else 0
    u_off = gh.file_slots(fd, heights, width, depth, colour, extra)
    u_file = torch.full((int(u_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    u_len, u_st = fd.png_encode_rgba_files_batch(d_rgba, d_off, u_file, gh.dev(u_off), width, depth, colour)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 4 and u_st.cpu().tolist() == [0] * 4
    host, offs, lens = file.cpu().numpy(), f_off.cpu().tolist(), f_len.cpu().tolist()
    u_host, u_lens = u_file.cpu().numpy(), u_len.cpu().tolist()

    def chunks(png):
        out, at = [], 8
        while at < len(png):
            size = fm.rd32(png, at)
            out.append((png[at + 4:at + 8], png[at + 8:at + 8 + size]))
            at += 12 + size
        return out

    for k, p in enumerate(images):
        mine, theirs = host[offs[k]:offs[k] + lens[k]].tobytes(), u_host[u_off[k]:u_off[k] + u_lens[k]].tobytes()
        if colour != 3:
            assert mine == theirs, (pair, k)
            continue
        a, b = chunks(mine), chunks(theirs)
        assert [t for t, _ in a] == [t for t, _ in b if t != b"tRNS" or p.trns]
        for tag, body in a:
            other = dict(b)[tag]
            if tag == b"PLTE":
                assert len(body) == 3 * p.count and other[:len(body)] == body and not any(other[len(body):])
            elif tag == b"tRNS":
                assert len(body) == p.trns and other[:len(body)] == body and set(other[len(body):]) <= {255}
            else:
                assert body == other, (pair, k, tag)
        assert pc.pillow_rgba(mine) == p.px.view(np.uint8).tobytes()
    if spoilt is not None:
        bad = rgba.copy()
        bad.view(np.uint32)[images[0].px.size + 3] = spoilt
        _, _, f_len, st, _ = fd.png_encode_mixed_rgba_files_batch(gh.dev(bad), d_off, w, h, pairs=pair)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0, 13, 0, 0] and f_len.cpu().tolist()[1] == 0


def test_caller_slots_too_many_colours_and_bad_records_in_the_pipeline():
    import torch
    import fdeflate_amd as fd
    cases = _ragged(13000)[:12]
    rgba, r_off, width, height = _collection(cases)
    file, f_off, f_len, st, _ = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height)
    torch.cuda.synchronize()
    lens = f_len.cpu().numpy().astype(np.int64)
    # the caller's slots: exact for all but one, which is one byte short, and one shorter than its prefix
    sizes = lens.copy()
    sizes[3] -= 1
    sizes[8] = 20
    own_off = gh.offsets(sizes, 6)
    own = torch.full((int(own_off[-1]) + 9,), GUARD, dtype=torch.uint8, device="cuda")
    _, _, own_len, own_st, _ = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height, file=own, file_off=gh.dev(own_off))
    torch.cuda.synchronize()
    want = [0] * 12
    want[3] = want[8] = 2
    assert own_st.cpu().tolist() == want and own_len.cpu().tolist() == [0 if w else int(v) for w, v in zip(want, lens)]
    host, first = own.cpu().numpy(), file.cpu().numpy()
    offs = f_off.cpu().tolist()
    assert (host[:6] == GUARD).all() and (host[own_off[-1]:] == GUARD).all() and (host[own_off[8]:own_off[9]] == GUARD).all()
    for k in range(12):
        if not want[k]:
            assert host[own_off[k]:own_off[k + 1]].tobytes() == first[offs[k]:offs[k] + lens[k]].tobytes(), k
    # a forced palette pair on a picture of more than 256 colours: the analysis' 12; width 0: 3; both without a file
    many = np.random.default_rng(13001).integers(0, 1 << 32, 40 * 40, dtype=np.uint64).astype(np.uint32).view(np.uint8)
    few = pc.palette_image(np.random.default_rng(13002), 40, 40, 200, 3)
    rgba2, off2 = gh.dev(np.concatenate([few, many, few])), gh.dev(gh.offsets([few.size, many.size, few.size]))
    _, _, l2, s2, _ = fd.png_encode_mixed_rgba_files_batch(rgba2, off2, gh.words([40, 40, 40]), gh.words([40, 40, 40]), pairs=(8, 3))
    _, _, l3, s3, _ = fd.png_encode_mixed_rgba_files_batch(rgba2, off2, gh.words([40, 0, 40]), gh.words([40, 40, 40]))
    _, _, l4, s4, _ = fd.png_encode_mixed_rgba_files_batch(rgba2, off2, gh.words([40, 40, 40]), gh.words([40, 41, 40]))
    torch.cuda.synchronize()
    assert s2.cpu().tolist() == [0, 12, 0] and l2.cpu().tolist()[1] == 0
    assert s3.cpu().tolist() == [0, 3, 0] and l3.cpu().tolist()[1] == 0
    assert s4.cpu().tolist() == [0, 2, 0] and l4.cpu().tolist()[1] == 0 and l4.cpu().tolist()[0] == l2.cpu().tolist()[0]


def test_one_read_back_of_at_most_64_bytes(monkeypatch):
    """Everything that leaves the device before the last kernel is enqueued goes through api._read_back, once, with at
    most 64 bytes; no .cpu(), .tolist(), .item() or .numpy() on a device tensor anywhere else in the pipeline."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import api
    cases = _ragged(13100)[:20]
    rgba, r_off, width, height = _collection(cases)
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
    out = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height)
    forced = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height, pairs=(8, 6))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(moved) == 2 and max(moved) <= 64 and stray == [], (moved, stray)
    assert out[3].cpu().tolist() == [0] * 20 and forced[3].cpu().tolist() == [0] * 20
