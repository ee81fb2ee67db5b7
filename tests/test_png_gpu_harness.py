"""The layout helpers of tests/png_gpu_harness.py that many GPU tests trust, checked with numpy alone."""
import numpy as np

import png_gpu_harness as gh


def test_batch_of_lays_files_out_between_fill_bytes():
    """Files of 1, 0 and 7 bytes from byte 5 with 3 bytes of slack each: the offsets, the lengths, every byte outside
    the files is the fill byte, and 16 fill bytes follow the last slot."""
    files = [b"\x01", b"", bytes(range(10, 17))]
    for fill in (0xEE, 0x5A):
        host, f_off, f_len = gh.batch_of(files, front=5, slack=3, fill=fill)
        assert f_off.dtype == np.int64 and f_off.tolist() == [5, 9, 12, 22]
        assert f_len.dtype == np.int32 and f_len.tolist() == [1, 0, 7]
        assert host.dtype == np.uint8 and host.size == 22 + 16
        inside = np.zeros(host.size, dtype=bool)
        for o, f in zip(f_off[:-1], files):
            assert host[o:o + len(f)].tobytes() == f
            inside[o:o + len(f)] = True
        assert inside.sum() == 8 and (host[~inside] == fill).all()
        assert (host[22:] == fill).all() and host[22:].size == 16
    assert gh.batch_of(files)[0].tobytes() == gh.batch_of(files, 5, 3, 0xEE)[0].tobytes()


def test_offsets_with_one_slack_and_with_one_per_slot():
    assert gh.offsets([4, 0, 9], 3, 2).tolist() == [3, 9, 11, 22]
    assert gh.offsets([4, 0, 9], 3, [1, 5, 0]).tolist() == [3, 8, 13, 22]
    assert gh.offsets([4, 0, 9]).tolist() == [0, 4, 4, 13] and gh.offsets([4, 0, 9], 7).tolist() == [7, 11, 11, 20]
    assert gh.offsets([], 6, 1).tolist() == [6] and gh.offsets([4], 0, [0]).dtype == np.int64
    # sizes beyond 32 bits stay exact
    assert gh.offsets([1 << 31, 1 << 31], 1, 0).tolist() == [1, (1 << 31) + 1, (1 << 32) + 1]


def test_widths_of_are_the_ends_of_the_docstrings_interval():
    """The smallest and the largest multiple of bpp in (16 (n - 1), 16 n]."""
    for bpp in (3, 6):
        for n in (1, 2):
            small, large = gh.widths_of(bpp, n)
            inside = [w for w in range(16 * (n - 1) + 1, 16 * n + 1) if w % bpp == 0]
            assert (small, large) == (inside[0], inside[-1]), (bpp, n)
    assert gh.widths_of(3, 1) == (3, 15) and gh.widths_of(3, 2) == (18, 30)
    assert gh.widths_of(6, 1) == (6, 12) and gh.widths_of(6, 2) == (18, 30)
