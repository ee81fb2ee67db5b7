"""The referee of the filter-selection tests, checked on the CPU: tests/png_choose_model.py against
the oracle's png_filter (the filtered bytes the sums are taken over), the tie order, the cost of the
wrap-around bytes, and the coverage that tests/test_gpu_png_choose.py relies on for the images both
share.  Everything here tests the model, not fdh_png_choose_filters_batch: it needs no GPU.
"""
import numpy as np
import pytest

import oracle_binding as ob
import png_choose_model as cm
import png_model

BPPS = (1, 2, 3, 4, 6, 8)


def _oracle_sums(img, bpp):
    rows, rb = img.shape
    sums = np.zeros((5, rows), dtype=np.int64)
    for t in cm.TYPES:
        st, filt = ob.png_filter(img.reshape(-1), rb, bpp, np.full(rows, t, dtype=np.uint8))
        assert st == 0
        f = np.frombuffer(filt, dtype=np.uint8).reshape(rows, rb + 1)
        assert (f[:, 0] == t).all()
        v = f[:, 1:].astype(np.int64)
        sums[t] = np.where(v < 128, v, 256 - v).sum(axis=1)
    return sums


@pytest.mark.parametrize("bpp", BPPS)
def test_sums_are_the_sums_over_the_oracles_filtered_bytes(bpp):
    """Every kind of image (the four png_model.DATA_KINDS, noise, ramps along x and y, diagonal
    gradients, images reconstructed from small residuals of each type), narrow and wide rows, 1 to 9
    rows: the model's 5 x rows table equals the sums over ob.png_filter's bytes for each fixed type,
    the choice is the first minimum of every column, and row 0 is never Up or Paeth."""
    r = np.random.default_rng(5100 + bpp)
    for k, kind in enumerate(cm.KINDS):
        for rb in (bpp, 5 * bpp, 48 // bpp * bpp + bpp, 1032 // bpp * bpp):
            rows = 1 + (k + rb) % 9
            img = cm.image(r, kind, rows, rb, bpp)
            assert img.shape == (rows, rb) and img.dtype == np.uint8
            types, sums = cm.choose(img, bpp)
            want = _oracle_sums(img, bpp)
            assert np.array_equal(sums, want), (kind, rb)
            assert types.tolist() == [int(np.argmin(want[:, y])) for y in range(rows)], (kind, rb)
            assert int(types[0]) in (0, 1, 3), (kind, rb, int(types[0]))
            assert sums[0, 0] == sums[2, 0] and sums[1, 0] == sums[4, 0]


# For every pair of types a two-row image (bpp 1) whose second row has exactly those two at the minimum.
TIES = {
    (0, 1): [[1, 3, 127, 4], [6, 3, 1, 4]],
    (0, 2): [[1, 255, 0, 6], [0, 2, 127, 4]],
    (0, 3): [[254, 1, 128, 2], [127, 254, 3, 2]],
    (0, 4): [[1, 0, 0, 254], [255, 4, 8, 0]],
    (1, 2): [[255, 3], [2, 8]],
    (1, 3): [[3, 0], [2, 2]],
    (1, 4): [[0, 0], [1, 128]],
    (2, 3): [[2, 1, 6, 4], [6, 3, 6, 6]],
    (2, 4): [[6, 255, 3], [8, 255, 127]],
    (3, 4): [[2, 3, 0, 4], [4, 4, 1, 254]],
}


def test_a_tie_of_every_pair_goes_to_the_lower_type():
    assert sorted(TIES) == [(i, j) for i in range(5) for j in range(i + 1, 5)]
    for (lo, hi), rows in TIES.items():
        img = np.array(rows, dtype=np.uint8)
        types, sums = cm.choose(img, 1)
        assert np.array_equal(sums, _oracle_sums(img, 1))
        col = sums[:, 1]
        assert col[lo] == col[hi] == col.min(), ((lo, hi), col.tolist())
        assert sorted(np.nonzero(col == col.min())[0].tolist()) == [lo, hi], ((lo, hi), col.tolist())
        assert int(types[1]) == lo
    # all five equal: a row of zeros under a row of zeros
    types, sums = cm.choose(np.zeros((2, 4), dtype=np.uint8), 1)
    assert (sums == 0).all() and types.tolist() == [0, 0]


def test_cost_of_the_wrap_around_bytes():
    """128 costs 128; 0xFF counts 1, not 255, also where it comes from 0x00 - 0x01 or 0x00 - 0xFF."""
    assert cm.cost(np.arange(256)).tolist() == list(range(128)) + [256 - v for v in range(128, 256)]
    assert int(cm.cost(128)) == 128 and int(cm.cost(255)) == 1 and int(cm.cost(129)) == 127 and int(cm.cost(0)) == 0
    _, s = cm.choose(np.array([[128]], dtype=np.uint8), 1)
    assert s[:, 0].tolist() == [128, 128, 128, 128, 128]
    _, s = cm.choose(np.array([[0xFF, 0x00], [0x00, 0xFF]], dtype=np.uint8), 1)
    # row 0: None FF 00 -> 1; Sub FF, 00 - FF = 01 -> 2.  row 1: Up 00 - FF = 01, FF - 00 = FF -> 2
    assert s[0].tolist() == [1, 1] and s[1, 0] == 2 and s[2].tolist() == [1, 2]
    # Sub in row 1: 00, FF - 00 = FF -> 1; Average: 00 - floor(FF / 2) = 81 -> 127, FF - floor((00 + 00) / 2) = FF -> 1
    assert s[1, 1] == 1 and s[3, 1] == 128
    _, s = cm.choose(np.array([[0x01, 0x00]], dtype=np.uint8), 1)
    assert s[1, 0] == 2             # Sub: 01, 00 - 01 = FF -> 1 + 1
    t, s = cm.choose(np.array([[0x80, 0x00]], dtype=np.uint8), 1)
    assert s[:, 0].tolist() == [128, 256, 128, 192, 256] and t.tolist() == [0]


@pytest.mark.parametrize("bpp", BPPS)
def test_coverage_of_the_shared_images(bpp):
    """What the GPU tests rely on, for the images of png_choose_model.choose_images (here at the two
    widths of 1, 2, 9, 64 and 65 chunks; the GPU test asserts the same over all its widths): each of
    the five types is chosen at least once, and at least one row in ten has a tied minimum."""
    count, ties, total = np.zeros(5, dtype=np.int64), 0, 0
    r = np.random.default_rng(5200 + bpp)
    k = 0
    for n in (1, 2, 9, 64, 65):
        lo, hi = 16 * (n - 1), 16 * n
        for rb in ((lo // bpp + 1) * bpp, hi // bpp * bpp):
            imgs = cm.choose_images(r, rb, bpp, shift=k)
            k += 1
            assert [im.shape for im in imgs] == [(nr, rb) for nr in cm.ROWS]
            for im in imgs:
                types, sums = cm.choose(im, bpp)
                count += np.bincount(types, minlength=5)
                ties += int(cm.tied(sums).sum())
                total += types.size
                if types.size:
                    assert int(types[0]) in (0, 1, 3)
    assert (count > 0).all(), count.tolist()
    assert 10 * ties >= total, (ties, total)
