"""PNG encode of mixed batches of RGBA16 pictures on the GPU (include/fdeflate_hip_png16_encode.h): the analysis, the plan
and the packing against tests/png16_encode_model.py and against the calls they derive from -- png_analyse_mixed_batch and
png_pack_mixed_batch on the pictures of the high bytes, png16.png_pack16_batch per geometry -- and the pipeline against
the RGBA8 pipeline, the depth-16 pipeline, the RGBA16 mixed decode, a host route without device code and Pillow.  Guard
bytes sit between the slots: every picture stands between slots whose upstream status is set, which no call may touch."""
import numpy as np
import pytest

import png16_encode_cases as cases
import png16_encode_model as e16
import png_encode_mixed_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_mixed_model as mm
from png_gpu_harness import BAND, GUARD, HEIGHTS, PACK_WIDTHS, PASSED_ON

pytestmark = pytest.mark.gpu

GUARD_WORD = 0x5A5A5A5A
OVERFLOW = ([0xFF000000] * 256, [0, 0, 0, 0], 0)       # pal, colour, trns_len of status 12


# ---- references in numpy (the model's values, checked against the model on the small pictures) ----

def summary_np(px):
    p = px.reshape(-1, 4).astype(np.uint32)
    opaque = bool((p[:, 3] == 65535).all())
    grey = bool(((p[:, 0] == p[:, 1]) & (p[:, 1] == p[:, 2])).all())
    narrow = bool((p == 257 * (p >> 8)).all())
    depth = next(d for d in (1, 2, 4, 8, 16) if bool((p[:, :3] % e16.UNIT16[d] == 0).all()))
    return (1 if opaque else 0) | (2 if grey else 0) | (4 if narrow else 0) | depth << 8


def high8(px):
    """The RGBA8 picture of the high bytes, uint8 [4 n]."""
    return (px >> 8).astype(np.uint8)


def analysis_np(px, max_colours=256):
    """-> (status, pal, colour, trns_len, summary) as the call writes them."""
    summary = summary_np(px)
    if summary & 4:
        distinct = np.unique(high8(px).view(np.uint32))
        if distinct.size <= max_colours:
            return (0, distinct.tolist() + [0xFF000000] * (256 - distinct.size), [int(distinct.size), 0, 0, 0],
                    int((distinct >> 24 < 255).sum()), summary)
    return (12,) + OVERFLOW + (summary,)


def check_against_model(px, width, got, max_colours=256):
    st, pal, count, trns, summary = e16.analyse16(px.tobytes(), width, max_colours)
    want = (st, pal, [count, 0, 0, 0], trns, summary) if st == 0 else (12,) + OVERFLOW + (summary,)
    assert got == want


class Slots:
    """RGBA16 pictures one behind the other, each at a chosen even address mod 16, a slot of GUARD bytes with upstream
    PASSED_ON in front of every picture and behind the last one.  entries: dicts with px (uint16 array, or None for a
    guard slot), width, height, depth, colour, and optionally size (the slot's bytes where they are not the picture's),
    upstream, status (the record's), align."""

    def __init__(self, entries, front=16):
        self.e = []
        cursor = front
        for k, e in enumerate(entries):
            align = e.get("align", 2 * (k % 8))
            gap = (align - cursor - 2) % 16 + 2                     # 2 .. 17 guard bytes
            self.e.append(dict(px=None, width=1, height=1, depth=0, colour=0, size=gap, upstream=PASSED_ON))
            cursor += gap
            assert cursor % 16 == align
            e = dict(e)
            e.setdefault("size", e["px"].size * 2)
            self.e.append(e)
            cursor += e["size"]
        self.e.append(dict(px=None, width=1, height=1, depth=0, colour=0, size=5, upstream=PASSED_ON))
        self.n = len(self.e)
        self.real = [k for k, e in enumerate(self.e) if e["px"] is not None]
        self.off = gh.offsets([e["size"] for e in self.e], front)
        self.host = np.full(int(self.off[-1]) + 32, GUARD, dtype=np.uint8)
        for k, e in enumerate(self.e):
            if e["px"] is not None:
                raw = e["px"].view(np.uint8)
                size = min(raw.size, e["size"])
                self.host[self.off[k]:self.off[k] + size] = raw[:size]
        self.info = np.asarray([mm.words(mm.record(e["width"], e["height"], e["depth"], e["colour"], status=e.get("status", 0),
                                                   interlace=e.get("interlace", 0))) for e in self.e], dtype=np.uint32)
        self.upstream = np.asarray([e.get("upstream", 0) for e in self.e], dtype=np.uint32)

    def device(self):
        self.d_rgba, self.d_off = gh.dev(self.host), gh.dev(self.off)
        assert self.d_rgba.data_ptr() % 16 == 0
        self.d_info, self.d_up = gh.words(self.info), gh.words(self.upstream)
        return self

    def unchanged(self):
        assert np.array_equal(self.d_rgba.cpu().numpy(), self.host)


def run_analysis(fd16, s, max_colours=256, with_pal=True):
    """-> per entry (status, pal, colour, trns_len, summary); what the call did not write reads as GUARD_WORD."""
    import torch
    s.device()
    n = s.n
    pal = torch.full((n + 2, 256), GUARD_WORD, dtype=torch.int32, device="cuda")
    col = torch.full((n + 2, 4), GUARD_WORD, dtype=torch.int32, device="cuda")
    trns, summ, st = (torch.full((n + 2,), GUARD_WORD, dtype=torch.int32, device="cuda") for _ in range(3))
    fd16.png_analyse16_mixed_batch(s.d_rgba, s.d_off, s.d_info, max_colours, with_pal=with_pal, upstream=s.d_up,
                                   pal=pal[1:n + 1] if with_pal else None, colour=col[1:n + 1], trns_len=trns[1:n + 1],
                                   summary=summ[1:n + 1], png_status=st[1:n + 1])
    torch.cuda.synchronize()
    s.unchanged()
    pal, col, trns, summ, st = (t.cpu().numpy().view(np.uint32) for t in (pal, col, trns, summ, st))
    for t in (pal, col, trns, summ, st):
        assert (t[0] == GUARD_WORD).all() and (t[n + 1] == GUARD_WORD).all()
    if not with_pal:
        assert (pal == GUARD_WORD).all()
    got = [(int(st[k]), pal[k].tolist(), col[k].tolist(), int(trns[k]), int(summ[k])) for k in range(1, n + 1)]
    untouched = ([GUARD_WORD] * 256, [GUARD_WORD] * 4, GUARD_WORD, GUARD_WORD)
    for k, e in enumerate(s.e):
        if e["px"] is None:
            assert got[k] == (PASSED_ON,) + untouched, k           # the guards between the pictures
    return got, untouched


def entry(px, width, height, depth=0, colour=0, **kw):
    return dict(px=np.ascontiguousarray(px, dtype=np.uint16).reshape(-1), width=width, height=height, depth=depth, colour=colour, **kw)


# ---- analyse16 ----

def _spoil_positions(width, height):
    """Sample indices at which ONE offending sample is put: first, last, in a pixel that may be handled alone in front,
    and either side of a lane's four pixels and of a wavefront's 256."""
    n = width * height * 4
    return sorted({0, n - 1, 1, 4 * 1 + 2} | {4 * p + c for p, c in ((3, 3), (4, 0), (255, 1), (256, 2), (257, 0)) if 4 * p + c < n})


def _varied_picture(r, width, height, kind):
    """kind: 0 .. 14 the fifteen pairs (a random picture the pair holds), so that narrow and not, opaque and not, grey
    and not and every depth occur."""
    depth, colour = fm.PAIRS[kind % 15]
    return cases.holds(r, width, height, depth, colour)[0]


def test_analyse16_widths_heights_alignments_and_kinds_in_one_batch(monkeypatch):
    """PACK_WIDTHS x HEIGHTS in one shuffled batch, every even alignment 0 .. 14 mod 16, pictures of all fifteen kinds:
    status, sorted palette, count, trns_len and summary are the model's; on narrow pictures every output equals
    png_analyse_mixed_batch on the high bytes; at 1 and 16 wavefronts and the default the words are the same."""
    import fdeflate_amd as fd
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(16500)
    shapes = [(w, h) for w in PACK_WIDTHS for h in HEIGHTS]
    order = r.permutation(len(shapes))
    entries = []
    for k, j in enumerate(order):
        w, h = shapes[j]
        entries.append(entry(_varied_picture(r, w, h, k), w, h, align=2 * (k % 8)))
    assert {e["align"] for e in entries} == set(range(0, 16, 2))
    s = Slots(entries)
    answers = []
    for waves in (None, 1, 16):
        gh.set_env(monkeypatch, FDH_PNG_ANALYSE_WAVES=waves)
        got, _ = run_analysis(fd16, s)
        answers.append(got)
    assert answers[0] == answers[1] == answers[2]
    got = answers[0]
    seen = set()
    for k in s.real:
        e = s.e[k]
        want = analysis_np(e["px"])
        assert got[k] == want, (k, e["width"], e["height"])
        if e["px"].size <= 4 * 260:
            check_against_model(e["px"], e["width"], got[k])
        seen.add((want[0], want[4] & 7, want[4] >> 8))
    # narrow and not, opaque and not, grey and not, every depth, both statuses
    assert {d for _, _, d in seen} == {1, 2, 4, 8, 16} and {b for _, b, _ in seen} == set(range(8)) and {s for s, _, _ in seen} == {0, 12}
    # the narrow pictures against the RGBA8 analysis of their high bytes
    narrow = [k for k in s.real if got[k][4] & 4]
    assert len(narrow) > 20
    import torch
    rgba8 = np.concatenate([high8(s.e[k]["px"]) for k in narrow])
    off8 = gh.offsets([s.e[k]["px"].size for k in narrow])
    info8 = fd.png_encode_records(gh.words([s.e[k]["width"] for k in narrow]), gh.words([s.e[k]["height"] for k in narrow]))
    pal, col, trns, summ, st = fd.png_analyse_mixed_batch(gh.dev(rgba8), gh.dev(off8), info8)
    torch.cuda.synchronize()
    pal, col, trns, summ, st = (t.cpu().numpy().view(np.uint32) for t in (pal, col, trns, summ, st))
    for j, k in enumerate(narrow):
        assert got[k] == (int(st[j]), pal[j].tolist(), col[j].tolist(), int(trns[j]), int(summ[j]) | 4), k


def test_analyse16_counts_buckets_and_max_colours():
    """1, 2, 16, 17, 256 and 257 distinct pixels and colours that share a hash bucket, under max_colours 256, 16 and 1;
    without pal."""
    import fdeflate_amd as fd
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(16600)
    width, height = 23, 13
    entries = []
    for count in (1, 2, 16, 17, 256, 257):
        px8 = cases.palette_image(r, width, height, count, count // 3)
        assert np.unique(px8.view(np.uint32)).size == count
        entries.append(entry(cases.widen(px8), width, height))
    white = np.full(width * height, 0xFFFFFFFF, dtype=np.uint32)           # the word with a flag of its own
    white[5] = 0x00FFFFFF
    entries.append(entry(cases.widen(white.view(np.uint8)), width, height))
    mul, bits = fd.PNG_ANALYSE_HASH_MUL, fd.PNG_ANALYSE_HASH_BITS
    inv = pow(mul, -1, 1 << 32)
    for bucket in (0, (1 << bits) - 1):
        words = np.array([((bucket << (32 - bits)) + 7919 * j + 1) * inv % (1 << 32) for j in range(256)], dtype=np.uint32)
        assert {(int(w) * mul % (1 << 32)) >> (32 - bits) for w in words} == {bucket}
        for colours in (40, 256):
            im = words[:colours][r.integers(0, colours, 16 * 32)]
            im[r.permutation(16 * 32)[:colours]] = words[:colours]
            entries.append(entry(cases.widen(im.view(np.uint8)), 16, 32))
    s = Slots(entries)
    statuses = set()
    for max_colours in (256, 39, 16, 1):
        got, _ = run_analysis(fd16, s, max_colours)
        for k in s.real:
            assert got[k] == analysis_np(s.e[k]["px"], max_colours), (k, max_colours)
            if max_colours in (256, 16):
                check_against_model(s.e[k]["px"], s.e[k]["width"], got[k], max_colours)
            statuses.add(got[k][0])
    assert statuses == {0, 12}
    got, _ = run_analysis(fd16, s, 256, with_pal=False)
    for k in s.real:
        want = analysis_np(s.e[k]["px"])
        assert (got[k][0],) + got[k][2:] == (want[0],) + want[2:], k


def test_analyse16_one_offending_sample_and_statuses(monkeypatch):
    """ONE sample whose bytes differ -- first, last, in the pixel handled alone in front, at a lane and at a wavefront
    boundary, in R, G, B and A -- turns a narrow picture into status 12 with a valid summary; so does one A below 65535
    for bit 0 and one G != R in the low byte for bit 1.  Statuses 2 (a slot one pixel short, one byte long, an odd
    address), 3 and upstream write nothing."""
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(16700)
    width, height = 37, 29                                                   # 1073 pixels: more than a wavefront's 256
    base = cases.widen(cases.palette_image(r, width, height, 40, 0))         # narrow, opaque, coloured
    entries = []
    for at in _spoil_positions(width, height):
        for align in (0, 8):                                                 # without and with a pixel alone in front
            px = base.copy()
            px[at] ^= 0x0001
            entries.append(entry(px, width, height, align=align))
    entries.append(entry(base, width, height, align=8))
    alpha = base.copy()
    alpha[4 * 600 + 3] = 0xFFFE
    entries.append(entry(alpha, width, height))
    s = Slots(entries)
    for waves in (None, 1):
        gh.set_env(monkeypatch, FDH_PNG_ANALYSE_WAVES=waves)
        got, _ = run_analysis(fd16, s)
        for k in s.real:
            want = analysis_np(s.e[k]["px"])
            assert got[k] == want, k
            check_against_model(s.e[k]["px"], width, got[k])
        assert [got[k][0] for k in s.real] == [12] * (len(entries) - 2) + [0, 12]
        assert got[s.real[-1]][4] & 7 == 0 and got[s.real[-2]][4] & 7 == 5
    gh.set_env(monkeypatch, FDH_PNG_ANALYSE_WAVES=None)
    good = entry(base, width, height)
    bad = [dict(good, size=base.size * 2 - 8), dict(good, size=base.size * 2 + 1), dict(good, align=3), dict(good, width=0),
           dict(good, depth=3), dict(good, interlace=1), dict(good, status=4), dict(good, upstream=9),
           dict(good, depth=8, colour=6), dict(good, depth=1, colour=3)]
    want = [2, 2, 2, 3, 3, 3, 3, 9, 0, 0]
    entries = []
    for b in bad:
        entries += [good, b]
    s = Slots(entries)
    # (Slots puts entry k at an even address unless it asks for an odd one: the guard in front absorbs the difference)
    got, untouched = run_analysis(fd16, s)
    for j, k in enumerate(s.real):
        if j % 2 == 0 or want[j // 2] == 0:
            assert got[k] == analysis_np(base), (j, k)                       # the neighbours, and encodable records
        else:
            assert got[k] == (want[j // 2],) + untouched, (j, k)


# ---- pack16_mixed ----

class Packed(Slots):
    """Slots with a pix side: every entry's slot is its plan's packed size (or pix_size), guards between them."""

    def __init__(self, entries):
        super().__init__(entries)
        sizes = []
        for e in self.e:
            if e["px"] is None:
                sizes.append(3)
            else:
                sizes.append(e.get("pix_size", e["height"] * em.row_bytes(max(e["width"], 1), e["depth"] or 8, e["colour"])
                                   if (e["depth"], e["colour"]) in fm.PAIRS else 7))
        self.p_off = gh.offsets(sizes, 3)
        self.pal = np.asarray([e.get("pal") or [0xFF000000] * 256 for e in self.e], dtype=np.uint32)
        self.count = np.asarray([[e.get("count", 256), 0, 0, 0] for e in self.e], dtype=np.uint32)

    def run(self, fd16, pal=True, upstream=True):
        import torch
        self.device()
        self.pix = torch.full((int(self.p_off[-1]) + 11,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n + 16,), GUARD_WORD, dtype=torch.int32, device="cuda")
        fd16.png_pack16_mixed_batch(self.d_rgba, self.d_off, self.pix, gh.dev(self.p_off), self.d_info, pal=gh.words(self.pal) if pal else None,
                                    colour=gh.words(self.count) if pal else None, upstream=self.d_up if upstream else None,
                                    png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        self.unchanged()
        st = st.cpu().numpy().view(np.uint32)
        assert (st[:8] == GUARD_WORD).all() and (st[8 + self.n:] == GUARD_WORD).all()
        self.status = st[8:8 + self.n].tolist()
        self.h_pix = self.pix.cpu().numpy()
        assert (self.h_pix[:self.p_off[0]] == GUARD).all() and (self.h_pix[self.p_off[-1]:] == GUARD).all()
        for k, e in enumerate(self.e):
            if e["px"] is None and upstream:
                assert self.status[k] == PASSED_ON and (self.slot(k) == GUARD).all(), k
        return self

    def slot(self, k):
        return self.h_pix[self.p_off[k]:self.p_off[k + 1]]


_CROSS = []


def cross_product():
    """All fifteen pairs times PACK_WIDTHS times heights 1, 2, 3 and BAND + 1, built once."""
    if not _CROSS:
        r = np.random.default_rng(16800)
        for depth, colour in fm.PAIRS:
            for width in PACK_WIDTHS:
                for height in (1, 2, 3, BAND + 1):
                    px, pal, count = cases.holds(r, width, height, depth, colour)
                    _CROSS.append(entry(px, width, height, depth, colour, pal=pal, count=count))
    return _CROSS


_REFERENCE = {}


def reference(fd, entries):
    """{id(entry): packed bytes} from the calls the mixed call derives from: png16.png_pack16_batch per (width, colour) for
    depth 16, png_pack_mixed_batch on the high bytes below; computed once."""
    import torch
    from fdeflate_amd import png16
    todo = list({id(e): e for e in entries if id(e) not in _REFERENCE}.values())
    groups = {}
    for e in todo:
        if e["depth"] == 16:
            groups.setdefault((e["width"], e["colour"]), []).append(e)
    for (width, colour), group in groups.items():
        r_off = gh.offsets([e["px"].size * 2 for e in group])
        p_off = gh.offsets([e["height"] * em.row_bytes(width, 16, colour) for e in group])
        pix = torch.zeros(int(p_off[-1]), dtype=torch.uint8, device="cuda")
        st = png16.png_pack16_batch(gh.dev(np.concatenate([e["px"] for e in group]).view(np.uint8)), gh.dev(r_off), pix, gh.dev(p_off), width, colour)
        assert st.cpu().tolist() == [0] * len(group)
        h = pix.cpu().numpy()
        for k, e in enumerate(group):
            _REFERENCE[id(e)] = h[p_off[k]:p_off[k + 1]].tobytes()
    low = [e for e in todo if e["depth"] < 16]
    if low:
        r_off = gh.offsets([e["px"].size for e in low])
        p_off = gh.offsets([e["height"] * em.row_bytes(e["width"], e["depth"], e["colour"]) for e in low])
        info = gh.words(np.asarray([mm.words(mm.record(e["width"], e["height"], e["depth"], e["colour"])) for e in low], dtype=np.uint32))
        pal = gh.words(np.asarray([e.get("pal") or [0xFF000000] * 256 for e in low], dtype=np.uint32))
        col = gh.words(np.asarray([[e.get("count", 256), 0, 0, 0] for e in low], dtype=np.uint32))
        pix = torch.zeros(int(p_off[-1]), dtype=torch.uint8, device="cuda")
        st = fd.png_pack_mixed_batch(gh.dev(np.concatenate([high8(e["px"]) for e in low])), gh.dev(r_off), pix, gh.dev(p_off), info, pal=pal, colour=col)
        assert st.cpu().tolist() == [0] * len(low)
        h = pix.cpu().numpy()
        for k, e in enumerate(low):
            _REFERENCE[id(e)] = h[p_off[k]:p_off[k + 1]].tobytes()
    return _REFERENCE


@pytest.mark.parametrize("order", [0, 1])
def test_pack16_every_pair_width_and_height_in_one_batch(order, monkeypatch):
    """All fifteen pairs, PACK_WIDTHS, heights 1, 2, 3 and BAND + 1 in ONE shuffled batch: depth-16 slots equal
    png_pack16_batch per geometry, slots below depth 16 equal png_pack_mixed_batch on the high bytes, every status 0,
    nothing outside the slots written; every seventh picture against the model; at 1 and 4 wavefronts per image."""
    import fdeflate_amd as fd
    from fdeflate_amd import png16_encode as fd16
    pictures = cross_product()
    perm = np.random.default_rng(16900 + order).permutation(len(pictures))
    chosen = [pictures[k] for k in perm]
    ref = reference(fd, chosen)
    gh.set_env(monkeypatch, FDH_PNG_PACK16_WAVES=(1, 4)[order])
    b = Packed([dict(e, align=2 * (k % 8)) for k, e in enumerate(chosen)]).run(fd16)
    for j, k in enumerate(b.real):
        e = chosen[j]
        what = (j, e["depth"], e["colour"], e["width"], e["height"])
        assert b.status[k] == 0, what
        assert b.slot(k).tobytes() == ref[id(e)], what
        if j % 7 == 0 and e["px"].size <= 4 * 600:
            want, st = e16.pack16_any(e["px"].tobytes(), e["width"], e["depth"], e["colour"], e.get("pal"), e.get("count", 256))
            assert st == 0 and b.slot(k).tobytes() == want, what


def test_pack16_one_sample_with_different_bytes_in_every_narrow_pair():
    """ONE sample whose bytes differ, at each of the positions of the analysis test, is status 13 in every one of the
    eleven pairs below depth 16; the neighbours' bytes are what they are without it."""
    import fdeflate_amd as fd
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(17000)
    width, height = 37, 9                                                    # 333 pixels: more than a wavefront's 256
    entries, spoilt = [], []
    for depth, colour in cases.NARROW_PAIRS:
        px, pal, count = cases.holds(r, width, height, depth, colour)
        good = entry(px, width, height, depth, colour, pal=pal, count=count)
        for j, at in enumerate(_spoil_positions(width, height)):
            bad = px.copy()
            bad[at] ^= 0x8000
            entries += [good, dict(good, px=bad, align=(0, 8)[j % 2])]
            spoilt += [False, True]
    ref = reference(fd, [e for e, s in zip(entries, spoilt) if not s])
    b = Packed(entries).run(fd16)
    for j, k in enumerate(b.real):
        if spoilt[j]:
            assert b.status[k] == 13, (j, entries[j]["depth"], entries[j]["colour"])
        else:
            assert b.status[k] == 0 and b.slot(k).tobytes() == ref[id(entries[j])], j


def test_pack16_statuses_and_a_wrong_image_among_good_ones():
    """Statuses 2 (either slot of the wrong size, an odd address), 3, 10 (colour type 3 without pal) and upstream; depth-16
    pictures the pair cannot hold are 13; a wrong image leaves its pix slot, its neighbours and the guards untouched."""
    import fdeflate_amd as fd
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(17100)
    width, height = 21, 5
    px, _, _ = cases.holds(r, width, height, 8, 6)
    good = entry(px, width, height, 8, 6)
    wide = entry(cases.wide_picture(r, width, height, 6), width, height, 16, 6)
    pal_px, pal, count = cases.holds(r, width, height, 4, 3)
    palette = entry(pal_px, width, height, 4, 3, pal=pal, count=count)
    rb = em.row_bytes(width, 8, 6)
    bad = [(dict(good, size=px.size * 2 - 8), 2), (dict(good, size=px.size * 2 + 2), 2), (dict(good, pix_size=height * rb - 1), 2),
           (dict(good, pix_size=height * rb + 1), 2), (dict(good, align=5), 2), (dict(wide, align=7), 2), (dict(good, depth=0, colour=0), 3),
           (dict(good, width=0), 3), (dict(good, interlace=1), 3), (dict(good, status=6), 3), (dict(good, upstream=11), 11),
           (dict(wide, depth=16, colour=2), 13), (dict(wide, depth=16, colour=4), 13), (dict(wide, depth=8, colour=6), 13)]
    entries = []
    for e, _ in bad:
        entries += [good, e, wide, palette]
    ref = reference(fd, [good, wide, palette])
    b = Packed(entries).run(fd16)
    for j, k in enumerate(b.real):
        e = entries[j]
        if j % 4 == 1:
            want = bad[j // 4][1]
            assert b.status[k] == want, (j, want)
            if want != 13:
                assert (b.slot(k) == GUARD).all(), j                          # nothing is written
        else:
            assert b.status[k] == 0 and b.slot(k).tobytes() == ref[id(e)], j
    # without pal: colour type 3 is status 10, everything else as before; without upstream the guards are records like any
    b = Packed([good, palette, wide]).run(fd16, pal=False)
    assert [b.status[k] for k in b.real] == [0, 10, 0] and (b.slot(b.real[1]) == GUARD).all()
    assert b.slot(b.real[0]).tobytes() == ref[id(good)] and b.slot(b.real[2]).tobytes() == ref[id(wide)]


# ---- plan16 on the device ----

@pytest.mark.parametrize("allowed", cases.MASKS)
def test_plan16_on_the_device_against_the_model(allowed):
    """The records, summaries, counts and masks of tests/test_png16_encode_model.py through fdh_png_encode16_plan_batch:
    status, sizes and the records afterwards are the model's."""
    import torch
    from fdeflate_amd import png16_encode as fd16
    records, inputs = cases.plan_records(), cases.plan_inputs()[::3]
    rows = [(r, i) for r in records for i in inputs]
    info = gh.words(np.asarray([mm.words(r) for r, _ in rows], dtype=np.uint32))
    colour = gh.words(np.asarray([[i[1] or 0, 0, 0, 0] for _, i in rows], dtype=np.uint32))
    trns = gh.words([i[2] or 0 for _, i in rows])
    summary, analysed = gh.words([i[0] for _, i in rows]), gh.words([i[3] for _, i in rows])
    out = fd16.png_encode16_plan_batch(info, colour, trns, summary, analysed, allowed)
    torch.cuda.synchronize()
    pix, types, prefix, size, st = (t.cpu().tolist() for t in out)
    after = info.cpu().numpy().view(np.uint32)
    for k, (r, (summ, count, tr, a_st)) in enumerate(rows):
        want = e16.plan16(r, count or 0, tr or 0, summ, a_st, allowed)
        assert (st[k], pix[k], types[k], prefix[k], size[k]) == (want[0],) + want[3:], (k, r, summ, count, tr, a_st)
        assert after[k].tolist() == mm.words(dict(r, bit_depth=want[1], colour_type=want[2])), (k, r)


# ---- the pipeline ----

def _ragged(seed):
    r = np.random.default_rng(seed)
    out = []
    for width, height in ((37, 29), (64, 17), (5, 3), (341, 64), (1, 1), (2, 2), (1023, 3)):
        out += [(name, px, width, height, depth, colour) for name, px, depth, colour in cases.kinds16(r, width, height)]
    order = r.permutation(len(out))
    return [out[k] for k in order]


def _collection(items):
    r_off = gh.offsets([c[1].size * 2 for c in items])
    rgba16 = np.concatenate([c[1] for c in items]).astype(np.uint16).view(np.uint8)
    return gh.dev(rgba16), gh.dev(r_off), gh.words([c[2] for c in items]), gh.words([c[3] for c in items])


def _files(file, f_off, f_len):
    host, offs, lens = file.cpu().numpy(), f_off.cpu().tolist(), f_len.cpu().tolist()
    return [host[offs[k]:offs[k] + lens[k]].tobytes() for k in range(len(lens))]


def test_pipeline_ragged_collection_comes_back_and_narrow_files_are_the_rgba8_pipelines():
    """A ragged collection of every kind through png_encode_mixed_rgba16_files_batch: the chosen pairs are the model's,
    png16.png_decode_mixed_files_rgba16_batch gives the pictures back exactly, every file passes the host route and
    Pillow, and the files of narrow pictures are byte-identical to png_encode_mixed_rgba_files_batch on their high bytes."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import png16
    from fdeflate_amd import png16_encode as fd16
    items = _ragged(17200)
    rgba16, r_off, width, height = _collection(items)
    file, f_off, f_len, st, info = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(items)
    files = _files(file, f_off, f_len)
    fields = info.cpu().numpy().view(np.uint32)
    seen = set()
    for k, (name, px, w, h, _, _) in enumerate(items):
        a_st, _, a_col, a_trns, a_summ = analysis_np(px)
        _, depth, colour = e16.plan16(mm.record(w, h, 0, 0), a_col[0], a_trns, a_summ, a_st, 0)[:3]      # the model's pair
        assert fields[k, 3] == depth | colour << 8, (k, name)
        scan = fm.scan(files[k])
        assert (scan.status, scan.width, scan.height, scan.bit_depth, scan.colour_type) == (0, w, h, depth, colour), (k, name)
        if w * h <= 1100:
            m_st, _, m_depth, m_colour = e16.encode16(px.tobytes(), w, h)
            assert (m_st, m_depth, m_colour) == (0, depth, colour), (k, name)
            assert cases.host_route(files[k]) == (px.tobytes(), depth, colour), (k, name)
        cases.check_in_pillow(files[k], px, w, h, depth, colour)
        seen.add((depth, colour))
    assert seen == set(fm.PAIRS)
    back, back_off, _, status, png_status = png16.png_decode_mixed_files_rgba16_batch(file, f_off, file_len=f_len)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(items) and png_status.cpu().tolist() == [0] * len(items)
    assert torch.equal(back_off, r_off) and torch.equal(back, rgba16)
    # narrow pictures: the RGBA8 pipeline on the high bytes
    narrow = [k for k, c in enumerate(items) if c[4] < 16]
    rgba8 = gh.dev(np.concatenate([high8(items[k][1]) for k in narrow]))
    off8 = gh.dev(gh.offsets([items[k][1].size for k in narrow]))
    f8, f8_off, f8_len, st8, _ = fd.png_encode_mixed_rgba_files_batch(rgba8, off8, gh.words([items[k][2] for k in narrow]),
                                                                      gh.words([items[k][3] for k in narrow]))
    torch.cuda.synchronize()
    assert st8.cpu().tolist() == [0] * len(narrow)
    for j, (k, theirs) in enumerate(zip(narrow, _files(f8, f8_off, f8_len))):
        assert files[k] == theirs, (k, items[k][0])
    # a mask: nothing but RGB and RGBA, at the depth the picture needs
    _, _, _, st2, info2 = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height, allowed=(1 << 2) | (1 << 6))
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [0] * len(items)
    pairs = {(int(w3) & 0xFF, (int(w3) >> 8) & 0xFF) for w3 in info2.cpu().numpy().view(np.uint32)[:, 3]}
    assert pairs == {(8, 2), (8, 6), (16, 2), (16, 6)}


@pytest.mark.parametrize("colour", [0, 2, 4, 6])
def test_pipeline_forced_depth16_pairs_give_the_depth16_pipelines_bytes(colour):
    """pairs=(16, colour): the files are png16.png_encode_rgba16_files_batch's, byte for byte; a picture the pair cannot
    hold is 13 without a file, and a forced palette pair on a picture that is not narrow is the analysis' 12."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import png16
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(17300 + colour)
    width, heights = 37, (1, 5, 70, 3)
    images = [cases.wide_picture(r, width, h, colour) for h in heights]
    rgba16 = gh.dev(np.concatenate(images).view(np.uint8))
    d_off = gh.dev(gh.offsets([im.size * 2 for im in images]))
    w, h = gh.words([width] * 4), gh.words(list(heights))
    file, f_off, f_len, st, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba16, d_off, w, h, pairs=(16, colour))
    u_off = gh.file_slots(fd, heights, width, 16, colour)
    u_file = torch.full((int(u_off[-1]) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    u_len, u_st = png16.png_encode_rgba16_files_batch(rgba16, d_off, u_file, gh.dev(u_off), width, colour)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 4 and u_st.cpu().tolist() == [0] * 4
    u_host, u_lens = u_file.cpu().numpy(), u_len.cpu().tolist()
    for k, mine in enumerate(_files(file, f_off, f_len)):
        assert mine == u_host[u_off[k]:u_off[k] + u_lens[k]].tobytes(), (colour, k)
    if colour != 6:
        _, _, l2, s2, _ = fd16.png_encode_mixed_rgba16_files_batch(gh.dev(np.concatenate([cases.wide_picture(r, width, x, 6) for x in heights]).view(np.uint8)),
                                                                   d_off, w, h, pairs=(16, colour))
        torch.cuda.synchronize()
        assert s2.cpu().tolist() == [13] * 4 and l2.cpu().tolist() == [0] * 4
    _, _, l3, s3, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba16, d_off, w, h, pairs=(8, 3))
    _, _, l4, s4, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba16, d_off, w, h, pairs=(8, 6))
    torch.cuda.synchronize()
    assert s3.cpu().tolist() == [12] * 4 and l3.cpu().tolist() == [0] * 4
    assert s4.cpu().tolist() == [13] * 4 and l4.cpu().tolist() == [0] * 4


def test_pipeline_many_images_one_and_none():
    """5000 small pictures (above the launch thresholds: the launch shapes change), one picture, no picture."""
    import torch
    from fdeflate_amd import png16
    from fdeflate_amd import png16_encode as fd16
    r = np.random.default_rng(17400)
    few = []
    for (depth, colour), w, h in zip(fm.PAIRS, (1, 2, 3, 5, 7, 8, 9, 11, 13, 16, 17, 4, 6, 10, 12), (1, 2, 3) * 5):
        few.append(("few", cases.holds(r, w, h, depth, colour)[0], w, h))
    items = [few[k % len(few)] for k in range(5000)]
    rgba16, r_off, width, height = _collection(items)
    file, f_off, f_len, st, info = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 5000
    files = _files(file, f_off, f_len)
    for k in range(len(few), 5000):
        assert files[k] == files[k % len(few)], k
    back, back_off, _, status, png_status = png16.png_decode_mixed_files_rgba16_batch(file, f_off, file_len=f_len)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(png_status.abs().sum()) == 0 and torch.equal(back, rgba16) and torch.equal(back_off, r_off)
    one = _collection(few[7:8])
    f1, o1, l1, s1, _ = fd16.png_encode_mixed_rgba16_files_batch(*one)
    torch.cuda.synchronize()
    assert s1.cpu().tolist() == [0] and _files(f1, o1, l1)[0] == files[7]
    # n == 0: success, nothing touched
    e64, e32 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    e8 = torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert fd16.png_pack16_mixed_batch(e8, e64, e8, e64, e32, png_status=e32).numel() == 0
    assert fd16.png_analyse16_mixed_batch(e8, e64, e32, colour=e32, trns_len=e32, summary=e32, png_status=e32, with_pal=False)[4].numel() == 0
    assert fd16.png_encode16_plan_batch(e32, png_status=e32)[4].numel() == 0
    out = fd16.png_encode_mixed_rgba16_files_batch(e8[:0], e64, e32, e32)
    assert out[2].numel() == 0 and out[3].numel() == 0


def test_pipeline_caller_slots_that_are_too_small_and_bad_records():
    import torch
    from fdeflate_amd import png16_encode as fd16
    items = _ragged(17500)[:12]
    rgba16, r_off, width, height = _collection(items)
    file, f_off, f_len, st, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height)
    torch.cuda.synchronize()
    lens = f_len.cpu().numpy().astype(np.int64)
    sizes = lens.copy()
    sizes[3] -= 1
    sizes[8] = 20
    own_off = gh.offsets(sizes, 6)
    own = torch.full((int(own_off[-1]) + 9,), GUARD, dtype=torch.uint8, device="cuda")
    _, _, own_len, own_st, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height, file=own, file_off=gh.dev(own_off))
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
    # width 0: 3; a slot that is not the picture's size: 2; both without a file, the neighbours as before
    three = [("a", cases.wide_picture(np.random.default_rng(17501), 40, 40, 6), 40, 40)] * 3
    rgba2, off2, _, _ = _collection(three)
    _, _, l2, s2, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba2, off2, gh.words([40, 40, 40]), gh.words([40, 40, 40]))
    _, _, l3, s3, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba2, off2, gh.words([40, 0, 40]), gh.words([40, 40, 40]))
    _, _, l4, s4, _ = fd16.png_encode_mixed_rgba16_files_batch(rgba2, off2, gh.words([40, 40, 40]), gh.words([40, 41, 40]))
    torch.cuda.synchronize()
    assert s2.cpu().tolist() == [0, 0, 0]
    assert s3.cpu().tolist() == [0, 3, 0] and l3.cpu().tolist()[1] == 0
    assert s4.cpu().tolist() == [0, 2, 0] and l4.cpu().tolist()[1] == 0 and l4.cpu().tolist()[0] == l2.cpu().tolist()[0]


def test_pipeline_one_read_back_of_at_most_64_bytes(monkeypatch):
    """Everything that leaves the device before the last kernel is enqueued goes through api._read_back, once, with at
    most 64 bytes; no .cpu(), .tolist(), .item() or .numpy() on a device tensor anywhere else in the pipeline (counted as
    tests/test_gpu_png_encode_mixed.py counts it)."""
    import torch
    from fdeflate_amd import api
    from fdeflate_amd import png16_encode as fd16
    items = _ragged(17600)[:20]
    rgba16, r_off, width, height = _collection(items)
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
    out = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height)
    forced = fd16.png_encode_mixed_rgba16_files_batch(rgba16, r_off, width, height, pairs=(16, 6))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(moved) == 2 and max(moved) <= 64 and stray == [], (moved, stray)
    assert out[3].cpu().tolist() == [0] * 20 and forced[3].cpu().tolist() == [0] * 20
