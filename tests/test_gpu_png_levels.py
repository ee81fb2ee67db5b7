"""-m gpu: PNG encode at a compression level (include/fdeflate_hip_png_levels.h, fdeflate_amd.png_levels).

The kernel: fdh_png_filter_mixed_batch on ONE shuffled batch whose images cover the lane-group powers of two and both
sides of one piece per lane (row sizes 1 .. 4097), the band boundaries (heights 1 .. 129), the six filter pixel sizes
and png_choose_model's image kinds.  Every image's slots in pix, types and filt stand between guard slots -- entries of
the batch with an upstream status and a record that is not encodable, which the call must not touch -- and the three
buffers are compared as wholes.  The referees are png_choose_model.choose and png_model.filter_rows; the library's own
fdh_png_choose_filters_mixed_batch and fdh_png_filter_batch are compared as well.

The pipelines: the pictures of tests/png_levels_cases.py in one mixed batch at levels 0, 1, 3, 4, 6 and 9 against the
files of the models (tests/test_png_levels_model.py checks those on the CPU).  Everything is bit-exact.
"""
import functools
import zlib

import numpy as np
import pytest

import png16_encode_cases as c16
import png_choose_model as cm
import png_corpus as pc
import png_file_model as fm
import png_gpu_harness as gh
import png_levels_cases as lc
import png_mixed_model as mm
import png_model

pytestmark = pytest.mark.gpu

GUARD = gh.GUARD
ROW_SIZES = (1, 15, 16, 17, 31, 33, 1023, 1024, 1025, 2049, 4097)
HEIGHTS = (1, 2, 63, 64, 65, 129)
PAIR_OF_BPP = {1: (8, 0), 2: (8, 4), 3: (8, 2), 4: (8, 6), 6: (16, 2), 8: (16, 6)}     # bpp -> a (depth, colour) with that pixel size


# ---- the batch of the kernel tests ----

class Batch:
    """images: [(pixels uint8 [rows, rb], bpp)].  Entry 2 k + 1 of the call is image k; the even entries are the guard
    slots: 3 + k % 5 bytes in each of the three buffers, upstream PASSED_ON, a record of width 0."""

    def __init__(self, images, upstream=None):
        self.images = images
        n = len(images)
        self.n = 2 * n + 1
        guard = [3 + k % 5 for k in range(n + 1)]
        sizes = {"pix": [], "types": [], "filt": []}
        records, self.upstream = [], []
        for e in range(self.n):
            if e % 2 == 0:
                for v in sizes.values():
                    v.append(guard[e // 2])
                records.append(mm.words(mm.record(0, 1, 8, 0)))
                self.upstream.append(gh.PASSED_ON)
            else:
                px, bpp = images[e // 2]
                rows, rb = px.shape
                depth, colour = PAIR_OF_BPP[bpp]
                sizes["pix"].append(rows * rb), sizes["types"].append(rows), sizes["filt"].append(rows * (rb + 1))
                records.append(mm.words(mm.record(rb // bpp, rows, depth, colour)))
                self.upstream.append(0 if upstream is None else upstream[e // 2])
        self.off = {k: gh.offsets(v) for k, v in sizes.items()}
        self.info = np.array(records, dtype=np.uint32)
        self.pix = np.full(int(self.off["pix"][-1]), GUARD, dtype=np.uint8)
        for k, (px, _) in enumerate(images):
            o = int(self.off["pix"][2 * k + 1])
            self.pix[o:o + px.size] = px.reshape(-1)

    def filled(self, name, per_image):
        """The buffer `name` as it must look afterwards: guard bytes, and per_image[k] in image k's slot (None: guards)."""
        out = np.full(int(self.off[name][-1]), GUARD, dtype=np.uint8)
        for k, v in enumerate(per_image):
            if v is not None:
                o = int(self.off[name][2 * k + 1])
                out[o:o + v.size] = v.reshape(-1)
        return out

    def run(self, pl, flags=0, types=None, with_types=True):
        """-> (status list of the images, status list of the guards, types buffer, filt buffer, pix buffer) from the device."""
        import torch
        d_types = gh.dev(types if types is not None else self.filled("types", [])) if with_types else None
        d_filt = gh.dev(self.filled("filt", []))
        d_pix = gh.dev(self.pix)
        st = pl.png_filter_mixed_batch(d_pix, gh.dev(self.off["pix"]), d_types, gh.dev(self.off["types"]) if with_types else None, d_filt,
                                       gh.dev(self.off["filt"]), gh.dev(self.info.view(np.int32)), upstream=gh.words(self.upstream), flags=flags)
        torch.cuda.synchronize()
        st = st.cpu().tolist()
        return st[1::2], st[0::2], d_types.cpu().numpy() if with_types else None, d_filt.cpu().numpy(), d_pix.cpu().numpy()


def _row_bytes(size, bpp):
    """The multiples of bpp next to `size`: at or below it (where there is one) and at or above it."""
    return sorted({v for v in (size // bpp * bpp, (size + bpp - 1) // bpp * bpp) if v})


@functools.lru_cache(maxsize=None)
def _shared():
    """The batch, its chosen types and the rows filtered with them, computed once: every row size at every pixel size, the
    heights and the kinds in turn so that every pixel size meets every height and every kind, shuffled."""
    r = np.random.default_rng(14100)
    shapes = [(rb, bpp) for bpp in cm_bpps() for size in ROW_SIZES for rb in _row_bytes(size, bpp)]
    images = []
    for k, (rb, bpp) in enumerate(shapes):
        rows = HEIGHTS[(k + k // len(HEIGHTS)) % len(HEIGHTS)]
        kind = cm.KINDS[k % len(cm.KINDS)]
        if kind.startswith("from") and rb > 64:          # (their serial reconstruction is slow in Python: narrow rows only)
            kind = ("hramp", "vramp", "diag", "small")[int(kind[4:]) - 1]
        images.append((cm.image(r, kind, rows, rb, bpp), bpp))
    images = [images[k] for k in r.permutation(len(images))]
    chosen = [cm.choose(px, bpp) for px, bpp in images]
    types = [t for t, _ in chosen]
    rows = [png_model.filter_rows(px, bpp, list(t)) for (px, bpp), t in zip(images, types)]
    return Batch(images), types, rows, [s for _, s in chosen]


def cm_bpps():
    return (1, 2, 3, 4, 6, 8)


def test_the_batch_covers_what_it_is_meant_to():
    batch, types, _, sums = _shared()
    shapes = {(px.shape[1], bpp) for px, bpp in batch.images}
    for bpp in cm_bpps():
        assert {px.shape[0] for px, b in batch.images if b == bpp} == set(HEIGHTS)
        for size in ROW_SIZES:
            assert any((rb, bpp) in shapes for rb in _row_bytes(size, bpp))
        assert any(rb <= 1024 for rb, b in shapes if b == bpp) and any(rb > 1024 for rb, b in shapes if b == bpp)
    assert set(ROW_SIZES) <= {rb for rb, b in shapes if b == 1}
    # every type wins somewhere, and every pair of types shares a row's minimum somewhere
    assert set(np.concatenate(types).tolist()) == {0, 1, 2, 3, 4}
    least = [s == s.min(axis=0) for s in sums]
    for a in range(5):
        for b in range(a + 1, 5):
            assert any((m[a] & m[b]).any() for m in least), (a, b)


def test_chosen_mode_whole_buffers_and_the_librarys_own_chooser():
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.png_levels as pl
    batch, types, rows, _ = _shared()
    st, guards, got_types, got_filt, got_pix = batch.run(pl)
    assert st == [0] * len(batch.images) and guards == [gh.PASSED_ON] * (len(batch.images) + 1)
    assert np.array_equal(got_pix, batch.pix)
    want_types = batch.filled("types", types)
    assert np.array_equal(got_types, want_types)
    bad = np.flatnonzero(got_filt != batch.filled("filt", rows))
    assert bad.size == 0, "first differing filt byte at %d" % bad[0]
    # fdh_png_choose_filters_mixed_batch on the same slots
    d_types = gh.dev(batch.filled("types", []))
    c_st = fd.png_choose_filters_mixed_batch(gh.dev(batch.pix), gh.dev(batch.off["pix"]), d_types, gh.dev(batch.off["types"]),
                                             gh.dev(batch.info.view(np.int32)), upstream=gh.words(batch.upstream))
    torch.cuda.synchronize()
    assert c_st.cpu().tolist()[1::2] == [0] * len(batch.images) and np.array_equal(d_types.cpu().numpy(), want_types)


def test_chosen_mode_without_a_types_buffer():
    import fdeflate_amd.png_levels as pl
    batch, _, rows, _ = _shared()
    st, guards, _, got_filt, _ = batch.run(pl, with_types=False)
    assert st == [0] * len(batch.images) and guards == [gh.PASSED_ON] * (len(batch.images) + 1)
    assert np.array_equal(got_filt, batch.filled("filt", rows))


def test_rows_equal_fdh_png_filter_batch_per_geometry():
    """Per (row_bytes, bpp): fdh_png_filter_batch, given the chosen types, writes the rows the model has."""
    import torch
    import fdeflate_amd as fd
    batch, types, rows, _ = _shared()
    shapes = sorted({(px.shape[1], bpp) for px, bpp in batch.images})
    for rb, bpp in shapes:
        ks = [k for k, (px, b) in enumerate(batch.images) if (px.shape[1], b) == (rb, bpp)]
        pix = np.concatenate([batch.images[k][0].reshape(-1) for k in ks])
        tp = np.concatenate([types[k] for k in ks])
        want = np.concatenate([rows[k].reshape(-1) for k in ks])
        heights = [batch.images[k][0].shape[0] for k in ks]
        filt = torch.full((want.size,), GUARD, dtype=torch.uint8, device="cuda")
        st = fd.png_filter_batch(gh.dev(pix), gh.dev(gh.offsets([h * rb for h in heights])), gh.dev(tp), gh.dev(gh.offsets(heights)), filt,
                                 gh.dev(gh.offsets([h * (rb + 1) for h in heights])), rb, bpp)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * len(ks) and np.array_equal(filt.cpu().numpy(), want), (rb, bpp)


@pytest.mark.parametrize("pattern", [0, 1, 2, 3, 4, "mixed"])
def test_given_types(pattern):
    import fdeflate_amd.png_levels as pl
    batch = _shared()[0]
    r = np.random.default_rng(14200)
    given = [r.integers(0, 5, px.shape[0], dtype=np.uint8) if pattern == "mixed" else np.full(px.shape[0], pattern, dtype=np.uint8)
             for px, _ in batch.images]
    rows = [png_model.filter_rows(px, bpp, list(t)) for (px, bpp), t in zip(batch.images, given)]
    types_in = batch.filled("types", given)
    st, guards, got_types, got_filt, got_pix = batch.run(pl, flags=pl.PNG_FILTER_GIVEN_TYPES, types=types_in)
    assert st == [0] * len(batch.images) and guards == [gh.PASSED_ON] * (len(batch.images) + 1)
    assert np.array_equal(got_types, types_in) and np.array_equal(got_pix, batch.pix)
    bad = np.flatnonzero(got_filt != batch.filled("filt", rows))
    assert bad.size == 0, "first differing filt byte at %d" % bad[0]


def _small(seed=14300):
    """Five images of both row kinds, a few bands."""
    r = np.random.default_rng(seed)
    return [(cm.image(r, kind, rows, rb, bpp), bpp) for kind, rows, rb, bpp in
            (("random", 5, 33, 3), ("diag", 70, 48, 4), ("small", 3, 1025, 1), ("hramp", 130, 16, 8), ("extreme", 1, 1, 1))]


def test_a_type_that_does_not_exist_is_status_1_for_its_image_alone():
    import fdeflate_amd.png_levels as pl
    images = _small()
    batch = Batch(images)
    r = np.random.default_rng(14301)
    given = [r.integers(0, 5, px.shape[0], dtype=np.uint8) for px, _ in images]
    given[1][66] = 5        # in the second band of image 1
    given[2][0] = 255       # in a looped row
    st, _, got_types, got_filt, _ = batch.run(pl, flags=pl.PNG_FILTER_GIVEN_TYPES, types=batch.filled("types", given))
    assert st == [0, 1, 1, 0, 0]
    want = batch.filled("filt", [png_model.filter_rows(px, bpp, list(t)) if k not in (1, 2) else None
                                 for k, ((px, bpp), t) in enumerate(zip(images, given))])
    for k in (0, 3, 4):         # the others are written as asked, and nothing outside a slot is touched
        o0, o1 = int(batch.off["filt"][2 * k + 1]), int(batch.off["filt"][2 * k + 2])
        assert np.array_equal(got_filt[o0:o1], want[o0:o1]), k
    for k in range(len(images) + 1):
        o0, o1 = int(batch.off["filt"][2 * k]), int(batch.off["filt"][2 * k + 1])
        assert (got_filt[o0:o1] == GUARD).all()
    assert np.array_equal(got_types, batch.filled("types", given))


@pytest.mark.parametrize("which", ["pix", "types", "filt"])
@pytest.mark.parametrize("given", [False, True], ids=["chosen", "given"])
def test_a_slot_of_the_wrong_size_is_status_2_and_nothing_is_written(which, given):
    import fdeflate_amd.png_levels as pl
    images = _small()
    batch = Batch(images)
    types = [cm.choose(px, bpp)[0] for px, bpp in images]
    rows = [png_model.filter_rows(px, bpp, list(t)) for (px, bpp), t in zip(images, types)]
    # image 1's slot grows by a byte, image 3's shrinks by one: the guard slots behind them take up the difference
    for k, d in ((1, 1), (3, -1)):
        batch.off[which][2 * k + 2] += d
    types_in = batch.filled("types", types if given else [])
    if given and which == "types":      # (the moved boundary: keep the given types where the call will read them)
        types_in = batch.filled("types", [t if k not in (1, 3) else None for k, t in enumerate(types)])
    st, guards, got_types, got_filt, got_pix = batch.run(pl, flags=pl.PNG_FILTER_GIVEN_TYPES if given else 0, types=types_in)
    assert st == [0, 2, 0, 2, 0] and guards == [gh.PASSED_ON] * 6
    keep = [v if k not in (1, 3) else None for k, v in enumerate(rows)]
    assert np.array_equal(got_filt, batch.filled("filt", keep))
    assert np.array_equal(got_types, types_in if given else batch.filled("types", [v if k not in (1, 3) else None for k, v in enumerate(types)]))
    assert np.array_equal(got_pix, batch.pix)


def test_upstream_is_passed_on_and_the_filt_slot_is_zeroed():
    import fdeflate_amd.png_levels as pl
    images = _small()
    batch = Batch(images, upstream=[0, 13, 0, 12, 9])
    types = [cm.choose(px, bpp)[0] for px, bpp in images]
    rows = [png_model.filter_rows(px, bpp, list(t)) for (px, bpp), t in zip(images, types)]
    st, guards, got_types, got_filt, _ = batch.run(pl)
    assert st == [0, 13, 0, 12, 9] and guards == [gh.PASSED_ON] * 6
    assert np.array_equal(got_filt, batch.filled("filt", [v if k in (0, 2) else np.zeros_like(v) for k, v in enumerate(rows)]))
    assert np.array_equal(got_types, batch.filled("types", [v if k in (0, 2) else None for k, v in enumerate(types)]))


@pytest.mark.parametrize("env", [{"FDH_PNG_CHOOSE_WAVES": 1}, {"FDH_PNG_CHOOSE_WAVES": 4}, {"FDH_PNG_CHOOSE_LANES": 64}],
                         ids=lambda e: "-".join("%s%d" % (k[15:].lower(), v) for k, v in e.items()))
def test_launch_shapes(monkeypatch, env):
    """One wavefront walks every band; four share them; every row gets a whole wavefront (and rows above 1024 bytes loop
    at that width): the same bytes in both modes."""
    import fdeflate_amd.png_levels as pl
    batch, types, rows, _ = _shared()
    gh.set_env(monkeypatch, **env)
    st, _, got_types, got_filt, _ = batch.run(pl)
    assert st == [0] * len(batch.images)
    assert np.array_equal(got_types, batch.filled("types", types)) and np.array_equal(got_filt, batch.filled("filt", rows))
    st, _, _, got_filt, _ = batch.run(pl, flags=pl.PNG_FILTER_GIVEN_TYPES, types=batch.filled("types", types))
    assert st == [0] * len(batch.images) and np.array_equal(got_filt, batch.filled("filt", rows))


# ---- the pipelines ----

def _collection(cases, sample_bytes=1):
    import torch
    bufs = [np.ascontiguousarray(c[1]).view(np.uint8).reshape(-1) for c in cases]
    off = gh.offsets([b.size for b in bufs])
    pairs = torch.tensor([list(c[4] or (0, 0)) for c in cases], dtype=torch.int32, device="cuda")
    return gh.dev(np.concatenate(bufs)), gh.dev(off), gh.words([c[2] for c in cases]), gh.words([c[3] for c in cases]), pairs


def _files(file, f_off, f_len):
    host, offs, lens = file.cpu().numpy(), f_off.cpu().tolist(), f_len.cpu().tolist()
    return [host[offs[k]:offs[k] + lens[k]].tobytes() for k in range(len(lens))]


def _check_against_the_model(cases, expected, out):
    file, f_off, f_len, st, info = out
    files = _files(file, f_off, f_len)
    fields = info.cpu().numpy().view(np.uint32)
    assert st.cpu().tolist() == [e[0] for e in expected] == [c[5] for c in cases]
    for k, ((name, _, w, h, pair, _), (m_st, want, depth, colour)) in enumerate(zip(cases, expected)):
        if m_st != 0:
            assert files[k] == b"", name
            continue
        assert files[k] == want, (k, name)
        assert (int(fields[k, 1]), int(fields[k, 2]), int(fields[k, 3])) == (w, h, depth | colour << 8), name
    return files


@pytest.mark.parametrize("level", lc.LEVELS)
def test_rgba8_pipeline_files_are_the_models_and_decode_back(level):
    """The case pictures in one mixed batch: files, lengths, statuses and records are the model's; the failing pictures
    (12, 13) stand among good ones and get no file; every good file decodes back on the device and in Pillow."""
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.png_levels as pl
    cases = lc.cases8()
    rgba, r_off, width, height, pairs = _collection(cases)
    out = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs)
    torch.cuda.synchronize()
    files = _check_against_the_model(cases, lc.expected8(level), out)
    good = [k for k, f in enumerate(files) if f]
    for k in good:
        assert pc.pillow_rgba(files[k]) == cases[k][1].tobytes(), cases[k][0]
    host, offs, lens = gh.batch_of([files[k] for k in good])
    back, back_off, _, status, png_status = fd.png_decode_mixed_files_rgba_batch(gh.dev(host), gh.dev(offs), file_len=gh.dev(lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(good) and png_status.cpu().tolist() == [0] * len(good)
    back, back_off = back.cpu().numpy(), back_off.cpu().tolist()
    for j, k in enumerate(good):
        assert back[back_off[j]:back_off[j + 1]].tobytes() == cases[k][1].tobytes(), cases[k][0]


@pytest.mark.parametrize("level", lc.LEVELS)
def test_rgba16_pipeline_files_are_the_models_and_narrow_ones_the_rgba8_calls(level):
    import torch
    import fdeflate_amd.png_levels as pl
    from fdeflate_amd import png16
    cases = lc.cases16()
    rgba16, r_off, width, height, pairs = _collection(cases)
    out = pl.png_encode_mixed_rgba16_files_level_batch(rgba16, r_off, width, height, level, pairs=pairs)
    torch.cuda.synchronize()
    files = _check_against_the_model(cases, lc.expected16(level), out)
    # the narrow pictures: the files of the RGBA8 call on their high bytes at the same level
    cases8 = lc.cases8()
    out8 = pl.png_encode_mixed_rgba_files_level_batch(*_collection(cases8)[:4], level, pairs=_collection(cases8)[4])
    torch.cuda.synchronize()
    files8 = dict(zip([c[0] for c in cases8], _files(out8[0], out8[1], out8[2])))
    for k, c in enumerate(cases):
        if c[0] in files8:
            assert files[k] == files8[c[0]], c[0]
    good = [k for k, f in enumerate(files) if f]
    for k in good:
        depth, colour = lc.expected16(level)[k][2:]
        c16.check_in_pillow(files[k], cases[k][1], cases[k][2], cases[k][3], depth, colour)
    host, offs, lens = gh.batch_of([files[k] for k in good], front=6, slack=2)
    back, back_off, _, status, png_status = png16.png_decode_mixed_files_rgba16_batch(gh.dev(host), gh.dev(offs), file_len=gh.dev(lens))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(good) and png_status.cpu().tolist() == [0] * len(good)
    back, back_off = back.cpu().numpy(), back_off.cpu().tolist()
    for j, k in enumerate(good):
        assert back[back_off[j]:back_off[j + 1]].tobytes() == cases[k][1].tobytes(), cases[k][0]


@pytest.mark.parametrize("level", [0, 3, 6])
def test_packed_scanlines_pipeline_chosen_and_given_types(level):
    """png_encode_mixed_files_level_batch on the packed scanlines of the good pictures that need no palette: the files of
    the RGBA8 call; with the rows' types given, the model's file around those types; a dimension record is status 3."""
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.png_levels as pl
    import png_encode_mixed_model as em
    import png_pack_model as pm
    cases, expected = lc.cases8(), lc.expected8(level)
    ks = [k for k, e in enumerate(expected) if e[0] == 0 and e[3] != 3]
    packed, records, heights = [], [], []
    for k in ks:
        _, px, w, h, _, _ = cases[k]
        depth, colour = expected[k][2:]
        pix, st = pm.pack(px.tobytes(), w, depth, colour, None, 256)
        assert st == 0
        packed.append(np.frombuffer(pix, dtype=np.uint8))
        records.append(mm.words(mm.record(w, h, depth, colour)))
        heights.append(h)
    records.append(mm.words(mm.record(4, 4, 0, 0)))            # a dimension record: not this call's to take
    packed.append(np.zeros(16, dtype=np.uint8))
    heights.append(4)
    pix, p_off = gh.dev(np.concatenate(packed)), gh.dev(gh.offsets([p.size for p in packed]))
    info = gh.dev(np.array(records, dtype=np.uint32).view(np.int32))
    file, f_off, f_len, st, _ = pl.png_encode_mixed_files_level_batch(pix, p_off, info, level)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(ks) + [3]
    files = _files(file, f_off, f_len)
    assert files == [expected[k][1] for k in ks] + [b""]
    # the caller's types: all Sub
    types = gh.dev(np.ones(sum(heights), dtype=np.uint8))
    file, f_off, f_len, st, _ = pl.png_encode_mixed_files_level_batch(pix, p_off, info, level, types=types, types_off=gh.dev(gh.offsets(heights)))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * len(ks) + [3]
    for k, got in zip(ks, _files(file, f_off, f_len)):
        _, px, w, h, _, _ = cases[k]
        depth, colour = expected[k][2:]
        rb, bpp = fm.geometry(w, depth, colour)
        rows = np.frombuffer(pm.pack(px.tobytes(), w, depth, colour, None, 256)[0], dtype=np.uint8).reshape(h, rb)
        idat = lc.compressor(level)(png_model.filter_rows(rows, bpp, [1] * h).tobytes())
        assert got == em.write_file(idat, w, h, depth, colour), cases[k][0]


def test_callers_slots_at_the_bound_and_one_byte_short():
    """Slots exactly at the bound hold every file; a slot one byte under prefix + 16 is status 2 with file_len 0, and so is
    one that is a byte too small for its stream; nothing is written to either, nor outside the slots."""
    import torch
    import fdeflate_amd.png_levels as pl
    level = 6
    cases, expected = lc.cases8(), lc.expected8(level)
    rgba, r_off, width, height, pairs = _collection(cases)
    _, d_off, d_len, _, _ = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs)
    torch.cuda.synchronize()
    bound = np.diff(d_off.cpu().numpy())
    for k, (st, f, depth, colour) in enumerate(expected):
        rb = fm.geometry(cases[k][2], depth, colour)[0]
        if st == 0:
            prefix = f.index(b"IDAT") + 4
            assert bound[k] == pl.level_file_bound(cases[k][3], rb, level, prefix) >= len(f), cases[k][0]
        elif st == 12:      # refused by the plan: no slot
            assert bound[k] == 0
        else:               # 13 is the packer's finding, behind the plan: the slot of the forced pair
            assert st == 13 and bound[k] == pl.level_file_bound(cases[k][3], rb, level)
    good = [k for k, e in enumerate(expected) if e[0] == 0]
    short, tight = good[1], good[3]
    sizes = bound.copy()
    sizes[short] = expected[short][1].index(b"IDAT") + 4 + 16 - 1
    sizes[tight] = len(expected[tight][1]) - 1
    own_off = gh.offsets(sizes, 7)
    own = torch.full((int(own_off[-1]) + 11,), GUARD, dtype=torch.uint8, device="cuda")
    _, _, own_len, own_st, _ = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs, file=own,
                                                                          file_off=gh.dev(own_off))
    torch.cuda.synchronize()
    want_st = [2 if k in (short, tight) else e[0] for k, e in enumerate(expected)]
    assert own_st.cpu().tolist() == want_st
    assert own_len.cpu().tolist() == [0 if s else len(e[1]) for s, e in zip(want_st, expected)]
    host = own.cpu().numpy()
    assert (host[:7] == GUARD).all() and (host[own_off[-1]:] == GUARD).all()
    for k, e in enumerate(expected):
        slot = host[own_off[k]:own_off[k + 1]]
        if want_st[k] == 0:
            assert slot[:len(e[1])].tobytes() == e[1], cases[k][0]
        elif k == short or e[0] != 0:
            assert (slot == GUARD).all(), cases[k][0]
    # exact slots: every file's own length, and none for the pictures that fail
    sizes = np.array([len(e[1]) if e[0] == 0 else 0 for e in expected], dtype=np.int64)
    own_off = gh.offsets(sizes, 3)
    own = torch.full((int(own_off[-1]) + 5,), GUARD, dtype=torch.uint8, device="cuda")
    _, _, own_len, own_st, _ = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs, file=own,
                                                                          file_off=gh.dev(own_off))
    torch.cuda.synchronize()
    # (a picture the plan accepts and the packer would refuse: its empty slot is found first, 2 in front of 13)
    assert own_st.cpu().tolist() == [2 if e[0] == 13 else e[0] for e in expected]
    host = own.cpu().numpy()
    assert host[3:own_off[-1]].tobytes() == b"".join(e[1] or b"" for e in expected) and (host[own_off[-1]:] == GUARD).all()


@functools.lru_cache(maxsize=None)
def _bench_pictures():
    """64 pictures of 341 x 64 RGB8: the bench's synthetic streams 0..63 (fdeflate_amd.synth, 64 filtered rows of 1 + 1023
    bytes each) unfiltered into pixels.  -> [(RGBA8 bytes with alpha 255, the rows the encoder must filter and compress)],
    the rows' types chosen by png_choose_model and applied by png_model."""
    import oracle_binding as ob
    from fdeflate_amd import synth
    out = []
    for i in range(64):
        st, pix = ob.png_unfilter(synth.gen_stream_np(i, 65536).tobytes(), 1023, 3)
        assert st == 0 and len(pix) == 64 * 1023
        rows = np.frombuffer(pix, dtype=np.uint8).reshape(64, 1023)
        rgba = np.full((64 * 341, 4), 255, dtype=np.uint8)
        rgba[:, :3] = rows.reshape(-1, 3)
        filt = png_model.filter_rows(rows, 3, lc.choose(rows, 3))
        out.append((rgba.reshape(-1), np.ascontiguousarray(filt).tobytes()))
    return out


@pytest.mark.parametrize("level", [1, 3, 6, 9])
def test_realistic_pictures_idat_is_the_oracles_stream(level):
    """The pipeline at the workload's shape -- the case pictures above are 48 x 40 and smaller --: 64 pictures of
    341 x 64 RGB8 (66 KB of filtered rows each) in one batch; every file's IDAT payload is the oracle's stream at that
    level of the rows the models filter, and the file is the model's around it."""
    import torch
    import fdeflate_amd.png_levels as pl
    import oracle_binding as ob
    import png_encode_mixed_model as em
    pictures = _bench_pictures()
    cases = [("bench-%d" % i, rgba, 341, 64, (8, 2), 0) for i, (rgba, _) in enumerate(pictures)]
    rgba, r_off, width, height, pairs = _collection(cases)
    file, f_off, f_len, st, _ = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * 64
    for i, (got, (_, filt)) in enumerate(zip(_files(file, f_off, f_len), pictures)):
        want = ob.compress_level(filt, level)
        idat = lc.idat_of(got)
        assert idat == want, (level, i, len(idat), len(want))
        assert got == em.write_file(want, 341, 64, 8, 2, crc=zlib.crc32), (level, i)
        assert lc.inflate(idat) == filt


def test_levels_that_do_not_exist_and_the_empty_batch():
    import torch
    import fdeflate_amd.png_levels as pl
    cases = lc.cases8()[:2]
    rgba, r_off, width, height, pairs = _collection(cases)
    for level in (10, True, "6", -1, None):
        with pytest.raises(ValueError):
            pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level)
        with pytest.raises(ValueError):
            pl.png_encode_mixed_rgba16_files_level_batch(rgba, r_off, width, height, level)
        with pytest.raises(ValueError):
            pl.png_encode_mixed_files_level_batch(rgba, r_off, pairs, level)
    e8 = torch.empty(0, dtype=torch.uint8, device="cuda")
    e32 = torch.empty(0, dtype=torch.int32, device="cuda")
    e64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for out in (pl.png_encode_mixed_rgba_files_level_batch(e8, e64, e32, e32, 6), pl.png_encode_mixed_rgba16_files_level_batch(e8, e64, e32, e32, 6),
                pl.png_encode_mixed_files_level_batch(e8, e64, e32.view(0, 8), 6)):
        assert out[2].numel() == 0 and out[3].numel() == 0 and out[1].tolist() == [0]
    assert pl.png_filter_mixed_batch(e8, e64, e8, e64, e8, e64, e32, png_status=e32).numel() == 0


def test_size_condition_against_the_ultrafast_pipeline():
    """The tiled RGB picture: the file at each of levels 1, 3, 6 and 9 is under one tenth of the file
    api.png_encode_mixed_rgba_files_batch writes for it."""
    import torch
    import fdeflate_amd as fd
    import fdeflate_amd.png_levels as pl
    case = [c for c in lc.cases8() if c[0] == lc.TILED]
    rgba, r_off, width, height, pairs = _collection(case)
    _, _, fast_len, fast_st, _ = fd.png_encode_mixed_rgba_files_batch(rgba, r_off, width, height, pairs=pairs)
    torch.cuda.synchronize()
    assert fast_st.cpu().tolist() == [0]
    fast = int(fast_len[0])
    for level in lc.SIZE_LEVELS:
        _, _, f_len, st, _ = pl.png_encode_mixed_rgba_files_level_batch(rgba, r_off, width, height, level, pairs=pairs)
        torch.cuda.synchronize()
        print("level %d: %d bytes; ultra-fast %d" % (level, int(f_len[0]), fast))
        assert st.cpu().tolist() == [0] and 10 * int(f_len[0]) < fast, (level, int(f_len[0]), fast)
