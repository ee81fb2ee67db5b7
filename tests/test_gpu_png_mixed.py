"""-m gpu: PNG decode of mixed batches -- fdh_png_plan_batch, fdh_png_gather_idat_mixed_batch, fdh_png_colour_mixed_batch,
fdh_png_unfilter_mixed_batch, fdh_png_expand_mixed_batch, png_decode_mixed_files_batch / png_decode_mixed_files_rgba_batch.

Expected bytes never come from the calls under test: they are what the per-geometry calls (png_unfilter_interlaced_batch,
png_expand_batch, png_colour_batch, png_decode_files_rgba_batch) give for the same images grouped by geometry, what
tests/png_adam7_model.py and tests/png_expand_model.py (plain integers) make of them, and Pillow's pictures.  Everything
is byte for byte.

A guard in this file is an image the call must skip (upstream != 0) whose slots hold 0x5A and have odd sizes: one sits in
front of, between and behind the images, so every image starts at an odd address next to bytes that must stay as they are.
"""
import io
import zlib

import numpy as np
import pytest

import png_adam7_model as am
import png_corpus as pc
import png_expand_model as em
import png_file_model as fm
import png_gpu_harness as gh
import png_mixed_model as mm
import png_model as pm

pytestmark = pytest.mark.gpu

GUARD = 0x5A
PASSED_ON = 77
WIDTHS = gh.EXPAND_WIDTHS
HEIGHTS = (1, 2, 3, 9, 65)                                                        # 65: one band of 64 rows plus a row
PALETTE_SIZES = (1, 2, 16, 17, 255, 256)


# ---- images ----

class Img:
    """One image of a call: its record, the bytes of its filt slot (a decoded IDAT stream), its palette and colour words."""

    def __init__(self, rec, filt=b"", pal=None, col=(256, 0, 0, 0), upstream=0, pix_size=None, rgba_size=None, upstream_len=None):
        self.rec = rec
        self.filt = np.frombuffer(bytes(filt), dtype=np.uint8) if not isinstance(filt, np.ndarray) else filt
        self.pal = pal                    # uint32 [256] or None
        self.col = list(col)
        self.upstream = upstream
        st, _, f, p, q = mm.plan(rec)
        self.pix_size = p if pix_size is None else pix_size
        self.rgba_size = q if rgba_size is None else rgba_size
        self.upstream_len = len(self.filt) if upstream_len is None else upstream_len
        self.geometry = (rec["width"], rec["bit_depth"], rec["colour_type"])


def type_positions(width, height, bits, method):
    """Where the filter type bytes lie in a decoded IDAT stream."""
    if method == 0:
        return np.arange(height, dtype=np.int64) * (1 + (width * bits + 7) // 8)
    out, base = [], 0
    for pw, ph in am.passes(width, height):
        if ph:
            stride = 1 + (pw * bits + 7) // 8
            out.append(base + np.arange(ph, dtype=np.int64) * stride)
            base += ph * stride
    return np.concatenate(out)


def random_image(r, width, height, depth, colour, method, k):
    """Random stream bytes with random filter types 0 .. 4 on every row of every pass; a random palette of one of the
    size classes (tRNS on some), a colour key on some grey and RGB images (the first pixel's samples cannot be told from
    a stream that is still filtered, so the key is random below depth 8 -- few values, many hits -- and rare above)."""
    bits = fm.CHANNELS[colour] * depth
    rec = mm.record(width, height, depth, colour, method, idat_bytes=9)
    size = mm.plan(rec)[2]
    filt = r.integers(0, 256, size, dtype=np.uint8)
    filt[type_positions(width, height, bits, method)] = r.integers(0, 5, am.pass_rows(width, height) if method else height)
    pal, col = None, [0, 0, 0, 0]
    if colour == 3:
        count = PALETTE_SIZES[k % len(PALETTE_SIZES)]
        words = r.integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32)
        if k % 2:
            words |= 0xFF000000           # no tRNS
        words[count:] = 0xFF000000
        pal, col = words, [count, 0, 0, 0]
    elif colour in (0, 2) and k % 3 == 0:
        key = r.integers(0, 1 << depth, 3).tolist()
        col = [0, 1, key[0] | key[1] << 16, key[2]]
    return Img(rec, filt, pal, col)


def guard_image(k, legal=True):
    rec = mm.record(3, 2, 8, 0) if legal else mm.record(0, 0, 5, 7, interlace=9, status=0)
    return Img(rec, np.full(5 + 2 * (k % 3), GUARD, dtype=np.uint8), None, upstream=PASSED_ON, pix_size=7 + 2 * (k % 2), rgba_size=9 + 2 * (k % 4))


def with_guards(images):
    seq = [guard_image(0)]
    for k, e in enumerate(images):
        seq += [e, guard_image(k + 1, legal=k % 3 != 0)]
    return seq


class Call:
    """The buffers of one call over `seq`: slots back to back from an odd byte on, guard bytes behind the last one."""

    def __init__(self, seq, front=3):
        self.seq, self.n = seq, len(seq)
        self.f_off = np.concatenate([[front], front + np.cumsum([len(e.filt) for e in seq], dtype=np.int64)]).astype(np.int64)
        self.p_off = np.concatenate([[front], front + np.cumsum([e.pix_size for e in seq], dtype=np.int64)]).astype(np.int64)
        self.r_off = np.concatenate([[front], front + np.cumsum([e.rgba_size for e in seq], dtype=np.int64)]).astype(np.int64)
        self.filt = np.full(int(self.f_off[-1]) + 9, GUARD, dtype=np.uint8)
        for o, e in zip(self.f_off[:-1], seq):
            self.filt[int(o):int(o) + len(e.filt)] = e.filt
        self.info = gh.words([mm.words(e.rec) for e in seq]).view(-1, 8) if seq else gh.words(np.zeros((0, 8)))
        self.pal = np.full((self.n, 256), 0x5A5A5A5A, dtype=np.uint32)
        for k, e in enumerate(seq):
            if e.pal is not None:
                self.pal[k] = e.pal
        self.col = np.array([e.col for e in seq], dtype=np.uint32).reshape(self.n, 4)

    def unfilter(self, fd, gates=True):
        """-> (status list, pix buffer on the host); checks the guard bytes around the slots and the status array's."""
        import torch
        d_filt = gh.dev(self.filt)
        d_pix = torch.full((int(self.p_off[-1]) + 33,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        fd.png_unfilter_mixed_batch(d_filt, gh.dev(self.f_off), d_pix, gh.dev(self.p_off), self.info,
                                    upstream=gh.words([e.upstream for e in self.seq]),
                                    upstream_len=gh.words([e.upstream_len for e in self.seq]) if gates else None, png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        st, got, after = st.cpu().numpy(), d_pix.cpu().numpy(), d_filt.cpu().numpy()
        assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + self.n:] == 0x5A5A5A5A).all()
        assert (got[:int(self.p_off[0])] == GUARD).all() and (got[int(self.p_off[-1]):] == GUARD).all()
        assert (after[:int(self.f_off[0])] == GUARD).all() and (after[int(self.f_off[-1]):] == GUARD).all()
        self.filt_after = after
        return st[8:8 + self.n].tolist(), got

    def expand(self, fd, pix, pal=True, colour=True):
        """`pix`: a host buffer laid out by p_off -> (status list, rgba buffer on the host), guards checked."""
        import torch
        d_rgba = torch.full((int(self.r_off[-1]) + 33,), GUARD, dtype=torch.uint8, device="cuda")
        st = torch.full((self.n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        fd.png_expand_mixed_batch(gh.dev(pix), gh.dev(self.p_off), d_rgba, gh.dev(self.r_off), self.info,
                                  pal=gh.dev(self.pal.view(np.int32)) if pal else None, colour=gh.dev(self.col.view(np.int32)) if colour else None,
                                  upstream=gh.words([e.upstream for e in self.seq]), png_status=st[8:8 + self.n])
        torch.cuda.synchronize()
        st, got = st.cpu().numpy(), d_rgba.cpu().numpy()
        assert (st[:8] == 0x5A5A5A5A).all() and (st[8 + self.n:] == 0x5A5A5A5A).all()
        assert (got[:int(self.r_off[0])] == GUARD).all() and (got[int(self.r_off[-1]):] == GUARD).all()
        return st[8:8 + self.n].tolist(), got

    def pix_buffer(self, slots):
        """A host pix buffer with `slots[k]` (bytes or None: guard bytes) in slot k."""
        buf = np.full(int(self.p_off[-1]) + 33, GUARD, dtype=np.uint8)
        for k, s in enumerate(slots):
            if s is not None:
                buf[int(self.p_off[k]):int(self.p_off[k + 1])] = np.frombuffer(s, dtype=np.uint8)
        return buf

    def slot(self, buf, off, k):
        return buf[int(off[k]):int(off[k + 1])]


def by_geometry(fd, images):
    """What the per-geometry calls make of `images`, each group of one (width, depth, colour) in a batch of its own:
    -> [(unfilter status, pix bytes, expand status, rgba bytes)] in the order of `images`.  Images that are skipped or do not
    fit are not given to them."""
    import torch
    groups, out = {}, [None] * len(images)
    for k, e in enumerate(images):
        groups.setdefault(e.geometry, []).append(k)
    for (width, depth, colour), members in groups.items():
        es = [images[k] for k in members]
        f_off = np.concatenate([[0], np.cumsum([len(e.filt) for e in es], dtype=np.int64)]).astype(np.int64)
        p_off = np.concatenate([[0], np.cumsum([e.pix_size for e in es], dtype=np.int64)]).astype(np.int64)
        r_off = np.concatenate([[0], np.cumsum([e.rgba_size for e in es], dtype=np.int64)]).astype(np.int64)
        d_pix = torch.zeros(max(1, int(p_off[-1])), dtype=torch.uint8, device="cuda")
        d_rgba = torch.zeros(max(1, int(r_off[-1])), dtype=torch.uint8, device="cuda")
        st_u = fd.png_unfilter_interlaced_batch(gh.dev(np.concatenate([e.filt for e in es])), gh.dev(f_off), d_pix, gh.dev(p_off), width, depth, colour,
                                                method=gh.dev(np.array([e.rec["interlace"] for e in es], dtype=np.uint8)))
        pal = gh.dev(np.stack([e.pal for e in es]).view(np.int32)) if colour == 3 else None
        st_e = fd.png_expand_batch(d_pix, gh.dev(p_off), d_rgba, gh.dev(r_off), width, depth, colour, pal=pal,
                                   colour=gh.dev(np.array([e.col for e in es], dtype=np.uint32).view(np.int32)))
        torch.cuda.synchronize()
        st_u, st_e, pix, rgba = st_u.cpu().tolist(), st_e.cpu().tolist(), d_pix.cpu().numpy(), d_rgba.cpu().numpy()
        for j, k in enumerate(members):
            out[k] = (st_u[j], pix[int(p_off[j]):int(p_off[j + 1])].tobytes(), st_e[j], rgba[int(r_off[j]):int(r_off[j + 1])].tobytes())
    return out


def by_models(e):
    """The two plain-integer models on one image -> (pix bytes, expand status, rgba bytes)."""
    w, h, d, c, m = (e.rec[k] for k in ("width", "height", "bit_depth", "colour_type", "interlace"))
    rb, bpp = fm.geometry(w, d, c)
    if m:
        pix = am.deinterlace(am.unfilter_passes(e.filt.tobytes(), w, h, d, c), w, h, d, c)
    else:
        pix = pm.unfilter(e.filt.tobytes(), rb, bpp)
    pal = key = None
    if c == 3:
        pal = [(int(v) & 255, int(v) >> 8 & 255, int(v) >> 16 & 255, int(v) >> 24) for v in e.pal[:e.col[0]]]
    elif e.col[1]:
        key = (e.col[2] & 0xFFFF, e.col[2] >> 16, e.col[3])[:3 if c == 2 else 1]
    rgba, st = em.expand(pix, w, d, c, key, pal)
    return bytes(pix), st, rgba


def check_against(call, expected, st_u, pix, st_e, rgba, chained):
    """Statuses and slots of a mixed call over call.seq against `expected` (by_geometry's tuples, None for a guard)."""
    for k, (e, want) in enumerate(zip(call.seq, expected)):
        p, q = call.slot(pix, call.p_off, k), call.slot(rgba, call.r_off, k)
        if want is None:
            assert st_u[k] == 3 and st_e[k] == PASSED_ON and (p == GUARD).all() and (q == GUARD).all(), k
            continue
        assert (st_u[k], st_e[k]) == (want[0], want[2]), (k, e.rec, st_u[k], st_e[k], want[0], want[2])
        assert p.tobytes() == want[1], (k, e.rec, "pix")
        assert q.tobytes() == want[3], (k, e.rec, "rgba")
        assert call.slot(chained, call.r_off, k).tobytes() == want[3], (k, e.rec, "chained")


# ---- the cross product in one batch ----

@pytest.fixture(scope="module")
def cross():
    """Fifteen pairs x two methods x nineteen widths x five heights, shuffled, and what the per-geometry calls give."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9100)
    images, k = [], 0
    for d, c in fm.PAIRS:
        for m in (0, 1):
            for w in WIDTHS:
                for h in HEIGHTS:
                    images.append(random_image(r, w, h, d, c, m, k))
                    k += 1
    order = r.permutation(len(images)).tolist()
    images = [images[j] for j in order]
    return images, by_geometry(fd, images)


def _run_order(fd, images, expected, order):
    seq = with_guards([images[j] for j in order])
    want = [None]
    for j in order:
        want += [expected[j], None]
    call = Call(seq)
    st_u, pix = call.unfilter(fd)
    st_e, rgba = call.expand(fd, call.pix_buffer([w[1] if w else None for w in want]))
    st_c, chained = call.expand(fd, pix)
    assert st_c == st_e
    check_against(call, want, st_u, pix, st_e, rgba, chained)
    return st_u, st_e


def test_cross_product_shuffled(cross):
    """Unfilter and expand, each on its own and chained, against the per-geometry calls run group by group."""
    import fdeflate_amd as fd
    images, expected = cross
    assert len(images) == 15 * 2 * len(WIDTHS) * len(HEIGHTS)
    st_u, st_e = _run_order(fd, images, expected, list(range(len(images))))
    assert set(st_u) == {0, 3} and {0, 9, PASSED_ON} == set(st_e)      # (random indices leave small palettes)


@pytest.mark.parametrize("order", ["sorted", "reversed"])
def test_cross_product_in_another_order(cross, order):
    import fdeflate_amd as fd
    images, expected = cross
    idx = sorted(range(len(images)), key=lambda j: (images[j].rec["colour_type"], images[j].rec["bit_depth"], images[j].rec["interlace"],
                                                    images[j].rec["width"], images[j].rec["height"]))
    _run_order(fd, images, expected, idx if order == "sorted" else list(reversed(range(len(images)))))


def test_cross_product_every_seventh_image_against_the_models(cross):
    """The per-geometry calls' results -- what the mixed calls are held to above -- are the models' on a fixed subset."""
    images, expected = cross
    for k in range(0, len(images), 7):
        pix, st, rgba = by_models(images[k])
        assert expected[k] == (0, pix, st, rgba), images[k].rec


# ---- gaps in the batch ----

def _small(r, k, w=None, h=None):
    d, c = fm.PAIRS[k % 15]
    return random_image(r, w or 1 + k % 11, h or 1 + k % 5, d, c, (k // 15) % 2, k)


def test_records_that_are_not_decodable_between_good_ones():
    """Records of every scan status and hand-made illegal ones, with no upstream to announce them: status 3, no byte
    written, the neighbours exact."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9200)
    bad = mm.undecodable_records()
    good = [_small(r, k) for k in range(len(bad) + 1)]
    expected = by_geometry(fd, good)
    seq, want = [good[0]], [expected[0]]
    for k, rec in enumerate(bad):
        seq += [Img(rec, np.full(6 + k % 3, GUARD, dtype=np.uint8), None, pix_size=5 + k % 4, rgba_size=8 + k % 5), good[k + 1]]
        want += [None, expected[k + 1]]
    call = Call(seq)
    st_u, pix = call.unfilter(fd)
    st_e, rgba = call.expand(fd, call.pix_buffer([w[1] if w else None for w in want]))
    for k, w in enumerate(want):
        if w is None:
            assert st_u[k] == 3 and st_e[k] == 3, (k, seq[k].rec)
            assert (call.slot(pix, call.p_off, k) == GUARD).all() and (call.slot(rgba, call.r_off, k) == GUARD).all()
            assert np.array_equal(call.slot(call.filt_after, call.f_off, k), seq[k].filt)
        else:
            assert (st_u[k], call.slot(pix, call.p_off, k).tobytes(), st_e[k], call.slot(rgba, call.r_off, k).tobytes()) == w, (k, seq[k].rec)


def test_one_image_and_none():
    import torch
    import fdeflate_amd as fd
    r = np.random.default_rng(9300)
    e = _small(r, 22, 33, 9)
    want = by_geometry(fd, [e])[0]
    call = Call([e], front=1)
    st_u, pix = call.unfilter(fd)
    st_e, rgba = call.expand(fd, pix)
    assert (st_u[0], call.slot(pix, call.p_off, 0).tobytes(), st_e[0], call.slot(rgba, call.r_off, 0).tobytes()) == want
    # n = 0: success, nothing touched (and no pointer is looked at)
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((16,), GUARD, dtype=torch.uint8, device="cuda")
    info = torch.zeros((0, 8), dtype=torch.int32, device="cuda")
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    fd.png_unfilter_mixed_batch(buf, off, buf, off, info, png_status=none)
    fd.png_expand_mixed_batch(buf, off, buf, off, info, png_status=none)
    fd.png_gather_idat_mixed_batch(buf, off, info, buf, off, comp_len=none, png_status=none)
    fd.png_colour_mixed_batch(buf, off, info, pal=none.view(0, 256), colour=none.view(0, 4), png_status=none)
    assert fd.png_plan_batch(info)[4].numel() == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()


def test_more_images_than_the_launch_shape_thresholds():
    """4 097 images of 1 x 1 that cycle through the thirty pair / method classes: one more than the count from which the
    gather takes one wavefront per file, and past 32768 / n = 8 wavefronts per image."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9400)
    images = [_small(r, k, 1, 1) for k in range(4097)]
    expected = by_geometry(fd, images)
    for k in range(0, len(images), 7):
        pix, st, rgba = by_models(images[k])
        assert expected[k] == (0, pix, st, rgba)
    call = Call(images, front=1)
    st_u, pix = call.unfilter(fd)
    st_e, rgba = call.expand(fd, pix)
    for k, w in enumerate(expected):
        assert (st_u[k], call.slot(pix, call.p_off, k).tobytes(), st_e[k], call.slot(rgba, call.r_off, k).tobytes()) == w, k


# ---- one image wrong among good ones ----

def _among(fd, r, wrong, at=2, classes=(1, 19, 7, 25, 13)):
    """`wrong` at position `at` among good images of five classes (both methods, two palettes), with guards
    -> (call, what is expected slot by slot: None for a guard, "wrong", by_geometry's tuple, position of `wrong`)."""
    good = [_small(r, c, 5 + k, 3 + k) for k, c in enumerate(classes)]
    expected = by_geometry(fd, good)
    images = good[:at] + [wrong] + good[at:]
    want = expected[:at] + ["wrong"] + expected[at:]
    seq, full = with_guards(images), [None]
    for w in want:
        full += [w, None]
    return Call(seq), full, 2 * at + 1


def _check_others(call, want, st_u, pix, st_e=None, rgba=None):
    for k, w in enumerate(want):
        if w is None:
            assert st_u is None or st_u[k] == 3
            assert (call.slot(pix, call.p_off, k) == GUARD).all() if st_u is not None else True
            assert rgba is None or (st_e[k] == PASSED_ON and (call.slot(rgba, call.r_off, k) == GUARD).all())
        elif w != "wrong":
            if st_u is not None:
                assert (st_u[k], call.slot(pix, call.p_off, k).tobytes()) == w[:2], k
            if rgba is not None:
                assert (st_e[k], call.slot(rgba, call.r_off, k).tobytes()) == w[2:], k


def test_a_filter_type_of_five_in_the_last_row_of_pass_three():
    import fdeflate_amd as fd
    r = np.random.default_rng(9500)
    e = random_image(r, 13, 13, 8, 2, 1, 4)
    rows = [ph for _, ph in am.passes(13, 13)]
    e.filt = e.filt.copy()
    e.filt[type_positions(13, 13, 24, 1)[sum(rows[:3]) - 1]] = 5
    call, want, at = _among(fd, r, e)
    st_u, pix = call.unfilter(fd)
    assert st_u[at] == 1
    _check_others(call, want, st_u, pix)


@pytest.mark.parametrize("what", ["filt one byte short", "pix one row long", "upstream_len one more", "upstream_len one less", "upstream 15"])
def test_unfilter_refuses_one_image(what):
    """Status 2 (3 for an upstream that is not 0, the zlib decoder's status as with png_unfilter_interlaced_batch), nothing
    written, the filt slot as it was, the others exact."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9600)
    e = random_image(r, 21, 9, 16, 6, 1, 1)
    rb = fm.geometry(21, 16, 6)[0]
    if what == "filt one byte short":
        e.filt = e.filt[:-1]
        e.upstream_len = len(e.filt)
    elif what == "pix one row long":
        e.pix_size += rb
    elif what == "upstream_len one more":
        e.upstream_len += 1
    elif what == "upstream_len one less":
        e.upstream_len -= 1
    else:
        e.upstream = 15
    call, want, at = _among(fd, r, e)
    st_u, pix = call.unfilter(fd)
    assert st_u[at] == (3 if what == "upstream 15" else 2)
    assert (call.slot(pix, call.p_off, at) == GUARD).all()
    assert np.array_equal(call.slot(call.filt_after, call.f_off, at), e.filt)
    _check_others(call, want, st_u, pix)


@pytest.mark.parametrize("what", ["rgba four bytes short", "pix not whole rows", "upstream 15", "no pal for a palette image"])
def test_expand_refuses_one_image(what):
    import fdeflate_amd as fd
    r = np.random.default_rng(9700)
    e = random_image(r, 21, 9, 4, 3, 0, 2)
    want_st = 2
    if what == "rgba four bytes short":
        e.rgba_size -= 4
    elif what == "pix not whole rows":
        e.pix_size += 1
    elif what == "upstream 15":
        e.upstream, want_st = 15, 15
    else:
        want_st = 10
    no_pal = what == "no pal for a palette image"
    call, want, at = _among(fd, r, e, classes=(1, 19, 5, 26, 13) if no_pal else (1, 19, 7, 25, 13))
    assert no_pal == all(x.rec["colour_type"] != 3 for k, x in enumerate(call.seq) if k != at)   # (without pal the others are of types 0, 2, 4, 6)
    pix = call.pix_buffer([w[1] if w not in (None, "wrong") else None for w in want])
    st_e, rgba = call.expand(fd, pix, pal=not no_pal)
    assert st_e[at] == want_st and (call.slot(rgba, call.r_off, at) == GUARD).all()
    _check_others(call, want, None, pix, st_e, rgba)


def test_an_index_equal_to_the_palette_count():
    """Status 9 on that image alone, the image written in full ((0, 0, 0, 255) at the index outside)."""
    import fdeflate_amd as fd
    r = np.random.default_rng(9800)
    w, h = 19, 4
    e = random_image(r, w, h, 8, 3, 0, 5)
    count = 200
    e.col = [count, 0, 0, 0]
    e.pal = e.pal.copy()
    e.pal[count:] = 0xFF000000
    pix = r.integers(0, count, (h, w), dtype=np.uint8)
    pix[h - 1, w - 1] = count
    call, want, at = _among(fd, r, e)
    slots = [w_[1] if w_ not in (None, "wrong") else None for w_ in want]
    slots[at] = pix.tobytes()
    st_e, rgba = call.expand(fd, call.pix_buffer(slots))
    model, st = em.expand(pix.tobytes(), w, 8, 3, None, [(int(v) & 255, int(v) >> 8 & 255, int(v) >> 16 & 255, int(v) >> 24) for v in e.pal[:count]])
    assert st == 9 and st_e[at] == 9 and call.slot(rgba, call.r_off, at).tobytes() == model and model[-4:] == bytes([0, 0, 0, 255])
    _check_others(call, want, None, None, st_e, rgba)


# ---- plan on the device ----

def test_plan_on_the_device_is_the_model():
    import torch
    import fdeflate_amd as fd
    cases = mm.all_cases()
    by_limit = {}
    for rec, m in cases:
        by_limit.setdefault(m, []).append(rec)
    assert 0 in by_limit and len(by_limit) > 10
    for m, recs in by_limit.items():
        info = gh.words([mm.words(x) for x in recs]).view(-1, 8)
        want = np.array([mm.plan(x, m) for x in recs], dtype=np.uint64)
        combos = range(16) if m == 0 else (15, 5)
        for mask in combos:
            wanted = [bool(mask >> j & 1) for j in range(4)]
            outs = fd.png_plan_batch(info, m, *wanted)
            torch.cuda.synchronize()
            assert outs[4].cpu().numpy().astype(np.uint64).tolist() == want[:, 0].tolist(), (m, mask)
            for j in range(4):
                if wanted[j]:
                    assert outs[j].cpu().numpy().view(np.uint64).tolist() == want[:, 1 + j].tolist(), (m, mask, j)
                else:
                    assert outs[j] is None


# ---- files ----

def test_colour_mixed_batch_every_status():
    """The files of png_corpus.status_files, each read at ITS geometry: the model's status (0, 3, 10, 11), pal
    and colour word for word; the pal rows of files that are not of colour type 3 keep the guard pattern; upstream passes."""
    import torch
    import fdeflate_amd as fd
    cases = [c for c in pc.status_files() if c[3] != 7]
    files = [c[1] for c in cases]
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off = gh.dev(host), gh.dev(f_off)
    info = fd.png_scan_files_batch(d_file, d_off, gh.dev(f_len))
    n, seen = len(files), set()
    upstream = [15 if k == 4 else 0 for k in range(n)]
    pal = torch.full((n + 2, 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    col = torch.full((n + 2, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    fd.png_colour_mixed_batch(d_file, d_off, info, upstream=gh.words(upstream), pal=pal[1:n + 1], colour=col[1:n + 1], png_status=st[1:n + 1])
    torch.cuda.synchronize()
    pal, col, st = (t.cpu().numpy().view(np.uint32) for t in (pal, col, st))
    for t in (pal, col, st):
        assert (t[0] == 0x5A5A5A5A).all() and (t[n + 1] == 0x5A5A5A5A).all()
    for k, (what, f, own, want, _) in enumerate(cases):
        m_info = fm.scan(f, crc=zlib.crc32)
        m_st, m_pal, m_key = em.read_colour(f, m_info, m_info.width, m_info.bit_depth, m_info.colour_type)
        if upstream[k]:
            assert st[k + 1] == 15 and (pal[k + 1] == 0x5A5A5A5A).all() and (col[k + 1] == 0x5A5A5A5A).all()
            continue
        assert st[k + 1] == m_st == want, what
        seen.add(m_st)
        if m_st == 0:
            assert col[k + 1].tolist() == em.colour_words(len(m_pal) if m_pal else 0, m_key), what
            if m_info.colour_type == 3:
                assert pal[k + 1].tolist() == em.pal_words(m_pal), what
        if m_info.colour_type != 3 or m_st != 0:
            assert (pal[k + 1] == 0x5A5A5A5A).all(), what
    assert seen == {0, 3, 10, 11}
    assert np.array_equal(d_file.cpu().numpy(), host)


def _pillow_image(Image, r, mode, w, h):
    if mode == "I;16":
        return Image.fromarray(r.integers(0, 65536, (h, w), dtype=np.uint16))
    if mode == "1":
        return Image.fromarray((r.integers(0, 2, (h, w), dtype=np.uint8) * 255)).convert("1")
    ch = {"L": 1, "P": 1, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
    a = r.integers(0, 256, (h, w, ch) if ch > 1 else (h, w), dtype=np.uint8)
    im = Image.fromarray(a, "L" if mode == "P" else mode)
    if mode == "P":
        im.putpalette(r.integers(0, 256, 768, dtype=np.uint8).tobytes())
    return im


def _rewrite(f, r, method, idat_chunks, pre_extra=()):
    """A sound file written again by the project's writer: interlaced or not, the stream in `idat_chunks` IDAT chunks,
    its PLTE / tRNS kept, further chunks in front."""
    w, h, d, c, pix = am.decode(f)
    info = am.scan(f, adam7=True, crc=zlib.crc32)
    _, pal, key = em.read_colour(f, info, w, d, c)
    pre = list(pre_extra) + pc.pre_chunks(c, key, pal)
    if method:
        idat = am.stream_of(bytes(pix), w, h, d, c, r.integers(0, 5, am.pass_rows(w, h)).tolist())
    else:
        idat = info.idat
    return am.write_file(idat, w, h, d, c, pre, idat_chunks, zlib.crc32, method=method)


@pytest.fixture(scope="module")
def collection():
    """[(file, what)]: Pillow's files in every mode it writes from 1 x 1 to 300 x 200, some written again interlaced or
    in three IDAT chunks behind tEXt and pHYs, the models' files of all fifteen pairs in both methods (tRNS where the class
    has one), and between them a damaged file of every status the scan gives with PNG_FLAG_ADAM7 and one that declares
    60 000 x 60 000 pixels."""
    Image = pytest.importorskip("PIL.Image")
    r = np.random.default_rng(9900)
    out = []
    sizes = ((1, 1), (2, 3), (7, 5), (33, 9), (64, 64), (100, 65), (300, 200), (257, 3), (3, 130))
    for k, mode in enumerate(("1", "L", "P", "LA", "RGB", "RGBA", "I;16") * 2):
        w, h = sizes[(2 * k + k // 7) % len(sizes)]
        b = io.BytesIO()
        _pillow_image(Image, r, mode, w, h).save(b, "PNG")
        out.append((b.getvalue(), "pillow " + mode))
        if k % 3 == 0 and w * h < 20000:
            out.append((_rewrite(b.getvalue(), r, 1, 1 + k % 2), "pillow " + mode + " interlaced"))
        if k % 3 == 1:
            out.append((_rewrite(b.getvalue(), r, 0, 3, [(b"tEXt", b"Comment\0x"), (b"pHYs", bytes(9))]), "pillow " + mode + " three IDAT"))
    k = 0
    for d, c in fm.PAIRS:
        for method in (0, 1):
            w, h = 1 + (5 * k) % 41, 1 + (3 * k) % 11
            keyed = (d, c) in pc.KEYED or (d, c) in pc.LEFT_OUT
            pix, key, pal = pc.random_case(r, w, h, d, c, keyed and k % 2 == 0)
            types = r.integers(0, 5, am.pass_rows(w, h) if method else h).tolist()
            rb, bpp = fm.geometry(w, d, c)
            idat = am.stream_of(pix.tobytes(), w, h, d, c, types) if method else zlib.compress(pm.filter_rows(pix.reshape(h, rb), bpp, types).tobytes())
            out.append((am.write_file(idat, w, h, d, c, pc.pre_chunks(c, key, pal, text=k % 4 == 0), 1 + k % 3, zlib.crc32, method=method),
                        "model depth %d colour %d method %d" % (d, c, method)))
            k += 1
    sound = out[4][0]
    crc = bytearray(sound)
    crc[-14] ^= 1                                           # the last byte of the last IDAT's CRC
    ihdr = bytearray(sound)
    ihdr[24] = 3                                            # a depth of 3
    ihdr[29:33] = fm.be32(zlib.crc32(bytes(ihdr[12:29])) & 0xFFFFFFFF)
    huge = em.write_file(zlib.compress(bytes(100)), 60000, 60000, 1, 0, [], 1, zlib.crc32)     # 450 MB of rows, 14 GB of RGBA8
    damaged = [(b"\x89PNX" + sound[4:], "no signature", 1), (sound[:len(sound) - 20], "truncated", 2), (bytes(ihdr), "bad IHDR", 3),
               (sound[:33] + fm.chunk(b"ABCD", b"", zlib.crc32) + sound[33:], "an unknown critical chunk", 5), (bytes(crc), "CRC", 6),
               (huge, "60 000 x 60 000", 0)]
    for j, (f, what, _) in enumerate(damaged):
        out.insert(3 + 7 * j, (f, "damaged: " + what))
    return out


def test_gather_mixed_batch(collection):
    """The IDAT bodies of files of every geometry in one call, exact slots between guard bytes: the model's bytes and
    lengths; 3 for a file the scan refused, 8 for a slot one byte short, an upstream value passed on, nothing written
    for any of those."""
    import torch
    import fdeflate_amd as fd
    files = [f for f, _ in collection]
    infos = [am.scan(f, adam7=True, crc=zlib.crc32) for f in files]
    sound = [k for k, m in enumerate(infos) if m.status == 0]
    short, passed = sound[3], sound[8]
    want_st = [3 if m.status else 8 if k == short else 15 if k == passed else 0 for k, m in enumerate(infos)]
    sizes = [0 if m.status else len(m.idat) - (k == short) for k, m in enumerate(infos)]
    c_off = np.concatenate([[3], 3 + np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off = gh.dev(host), gh.dev(f_off)
    info = fd.png_scan_files_batch(d_file, d_off, gh.dev(f_len), flags=fd.PNG_FLAG_ADAM7)
    comp = torch.full((int(c_off[-1]) + 40,), GUARD, dtype=torch.uint8, device="cuda")
    comp_len, st = fd.png_gather_idat_mixed_batch(d_file, d_off, info, comp, gh.dev(c_off), upstream=gh.words([15 if k == passed else 0 for k in range(len(files))]))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == want_st and {0, 3, 8, 15} == set(want_st)
    got, lens = comp.cpu().numpy(), comp_len.cpu().tolist()
    assert (got[:3] == GUARD).all() and (got[int(c_off[-1]):] == GUARD).all()
    for k, m in enumerate(infos):
        slot = got[int(c_off[k]):int(c_off[k + 1])]
        if want_st[k] == 0:
            assert lens[k] == len(m.idat) and slot.tobytes() == m.idat, collection[k][1]
        else:
            assert lens[k] == 0 and (slot == GUARD).all(), collection[k][1]
    assert np.array_equal(d_file.cpu().numpy(), host)


def _model_of(f, what, adam7=True, max_bytes=1 << 28):
    """-> (png_status, packed pixels, rgba, (width, height)) of one file by the models."""
    info = am.scan(f, adam7=adam7, crc=zlib.crc32)
    if info.status != 0:
        return 3, b"", b"", None
    if mm.plan(mm.of_info(info), max_bytes)[0] != 0:
        return mm.plan(mm.of_info(info), max_bytes)[0], b"", b"", None
    w, h, d, c, pix = am.decode(f)
    st, pal, key = em.read_colour(f, info, w, d, c)
    assert st == 0, what
    rgba, st = em.expand(pix, w, d, c, key, pal)
    return st, bytes(pix), rgba, (w, h, d, c)


def test_files_end_to_end(collection):
    import torch
    import fdeflate_amd as fd
    files = [f for f, _ in collection]
    models = [_model_of(f, what) for f, what in collection]
    assert {m[0] for m in models} == {0, 2, 3} and sum(1 for m in models if m[0] == 0) >= 40
    for (f, what), m in zip(collection, models):                 # Pillow, where it follows the specification
        if m[0] == 0 and (m[3][2], m[3][3]) not in pc.LEFT_OUT:
            assert pc.pillow_rgba(f) == m[2], what
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off, d_len = gh.dev(host), gh.dev(f_off), gh.dev(f_len)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rgba, rgba_off, info, status, png_status = fd.png_decode_mixed_files_rgba_batch(d_file, d_off, d_len, flags=fd.PNG_FLAG_ADAM7, max_bytes=1 << 28)
    pix, pix_off, info2, status2, png_status2 = fd.png_decode_mixed_files_batch(d_file, d_off, d_len, flags=fd.PNG_FLAG_ADAM7, max_bytes=1 << 28)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 1 << 28          # nothing was allocated for what the one file declares
    assert torch.equal(info, info2) and torch.equal(status, status2)
    r_off, p_off, st, zst, st2 = rgba_off.cpu().tolist(), pix_off.cpu().tolist(), png_status.cpu().tolist(), status.cpu().tolist(), png_status2.cpu().tolist()
    got_rgba, got_pix = rgba.cpu().numpy(), pix.cpu().numpy()
    assert rgba.numel() == r_off[-1] and pix.numel() == p_off[-1]
    for k, ((f, what), m) in enumerate(zip(collection, models)):
        assert st[k] == m[0] and st2[k] == (m[0] if m[0] != 9 else 0), (what, st[k], st2[k], m[0])
        assert (zst[k] == 0) == (m[0] in (0, 9)), (what, zst[k])
        assert got_pix[p_off[k]:p_off[k + 1]].tobytes() == m[1], what
        assert got_rgba[r_off[k]:r_off[k + 1]].tobytes() == m[2], what
    # without PNG_FLAG_ADAM7 the interlaced files are 3 with empty slots, everything else is as it was
    rgba3, rgba_off3, info3, _, png_status3 = fd.png_decode_mixed_files_rgba_batch(d_file, d_off, d_len, max_bytes=1 << 28)
    torch.cuda.synchronize()
    r3, st3, got3 = rgba_off3.cpu().tolist(), png_status3.cpu().tolist(), rgba3.cpu().numpy()
    interlaced = 0
    for k, ((f, what), m) in enumerate(zip(collection, models)):
        if am.scan(f, adam7=True, crc=zlib.crc32).interlace == 1 and m[0] != 3:
            interlaced += 1
            assert st3[k] == 3 and r3[k] == r3[k + 1] and info3[k, 0].item() == 4, what
        else:
            assert st3[k] == m[0] and got3[r3[k]:r3[k + 1]].tobytes() == m[2], what
    assert interlaced >= 15


# ---- routes ----

def _uniform_batch():
    r = np.random.default_rng(9950)
    w, h, d, c = 33, 9, 8, 2
    rb, bpp = fm.geometry(w, d, c)
    files = []
    for k in range(64):
        pix = r.integers(0, 256, (h, rb), dtype=np.uint8)
        idat = zlib.compress(pm.filter_rows(pix, bpp, r.integers(0, 5, h).tolist()).tobytes())
        files.append(em.write_file(idat, w, h, d, c, [(b"tRNS", em.trns_body(tuple(int(v) for v in pix[0, :3])))] if k % 5 == 0 else [], 1 + k % 2, zlib.crc32))
    broken = bytearray(files[17])
    broken[-14] ^= 4
    files[17] = bytes(broken)
    files[40] = files[40][:50]
    return files, (w, d, c)


def test_routes_give_the_same_tensors():
    import torch
    import fdeflate_amd as fd
    files, geometry = _uniform_batch()
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off, d_len = gh.dev(host), gh.dev(f_off), gh.dev(f_len)
    for decode, parent in ((fd.png_decode_mixed_files_rgba_batch, fd.png_decode_files_rgba_batch), (fd.png_decode_mixed_files_batch, fd.png_decode_files_batch)):
        mixed = decode(d_file, d_off, d_len, route="mixed")
        uniform = decode(d_file, d_off, d_len, route="uniform")
        chosen = decode(d_file, d_off, d_len)
        old = parent(d_file, d_off, *geometry, file_len=d_len)
        torch.cuda.synchronize()
        for a, b, c in zip(mixed, uniform, chosen):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert mixed[4].cpu().tolist() == [3 if k in (17, 40) else 0 for k in range(64)]
        for a, b in zip(mixed, old):            # (the damaged files have empty slots in both, so the offsets agree as well)
            assert torch.equal(a, b)


def test_route_uniform_refuses_a_mixed_batch(collection):
    import fdeflate_amd as fd
    host, f_off, f_len = gh.batch_of([f for f, _ in collection[:12]])
    with pytest.raises(ValueError):
        fd.png_decode_mixed_files_rgba_batch(gh.dev(host), gh.dev(f_off), gh.dev(f_len), route="uniform")
    with pytest.raises(ValueError):
        fd.png_decode_mixed_files_batch(gh.dev(host), gh.dev(f_off), gh.dev(f_len), route="sideways")


# ---- the read-back ----

@pytest.mark.parametrize("route", ["mixed", "uniform"])
def test_one_read_back_of_at_most_64_bytes(route, monkeypatch):
    """Everything that leaves the device before the last kernel is enqueued goes through api._read_back, once, with at
    most 64 bytes; no .cpu(), .tolist(), .item() or .numpy() on a device tensor anywhere else in the pipeline."""
    import torch
    import fdeflate_amd as fd
    from fdeflate_amd import api
    files, _ = _uniform_batch()
    host, f_off, f_len = gh.batch_of(files)
    d_file, d_off, d_len = gh.dev(host), gh.dev(f_off), gh.dev(f_len)
    moved, stray = [], []
    inner = api._read_back

    def counted(t):
        moved.append(t.numel() * t.element_size())
        with monkeypatch.context() as m:        # (the wrapper itself may use any of them)
            for name in ("cpu", "tolist", "item", "numpy"):
                m.setattr(torch.Tensor, name, originals[name])
            return inner(t)

    originals = {name: getattr(torch.Tensor, name) for name in ("cpu", "tolist", "item", "numpy")}

    def spy(name):
        def call(self, *a, **k):
            if self.is_cuda:
                stray.append(name)
            return originals[name](self, *a, **k)
        return call

    monkeypatch.setattr(api, "_read_back", counted)
    for name in originals:
        monkeypatch.setattr(torch.Tensor, name, spy(name))
    out = fd.png_decode_mixed_files_rgba_batch(d_file, d_off, d_len, route=route)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(moved) == 1 and moved[0] <= 64 and stray == [], (moved, stray)
    assert out[4].cpu().tolist().count(0) == 62
