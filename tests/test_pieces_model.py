"""tests/pieces_model.py on the CPU: the stitched streams of the models inflate in zlib to their inputs, carry zlib's
Adler-32, equal the one-shot stream where the input is one piece, and the combine rule of the plan kernel gives
zlib.adler32 at its worst case.  The pinned inputs keep a non-last piece of two blocks in the suite."""
import zlib

import numpy as np
import pytest

import adler_payloads
import lazy_model
import level_model
import pieces_model as pm

LEVELS = tuple(range(1, 10))
PIECE_SIZES = (64, 5552, 65521, 65536)      # the smallest piece; zlib's NMAX; the modulus; the default


def small_inputs():
    r = np.random.default_rng(15000)
    text = b"".join(bytes(r.integers(97, 101, int(r.integers(3, 9)), dtype=np.uint8)) + b" " for _ in range(200))
    return [b"", b"a", b"abc", bytes(64), bytes(65), text[:257], text, bytes(r.integers(0, 256, 700, dtype=np.uint8)), bytes(range(256)) * 5]


def inflate_raw(piece, more=b""):
    d = zlib.decompressobj(-15)
    out = d.decompress(piece + more)
    return out, d


@pytest.mark.parametrize("level", LEVELS)
def test_one_piece_is_the_one_shot_stream(level):
    model = level_model if level <= 3 else lazy_model
    for data in small_inputs():
        want = model.compress(data, level)
        for piece_bytes in (max(64, len(data)), len(data) + 1 if len(data) >= 64 else 64, 65536):
            assert pm.compress(data, level, piece_bytes) == want, (len(data), piece_bytes)


@pytest.mark.parametrize("level", LEVELS)
def test_stitched_streams_inflate_and_carry_zlibs_checksum(level):
    for data in small_inputs():
        for piece_bytes in (64, 100, 257):
            got = pm.compress(data, level, piece_bytes)
            assert zlib.decompress(got) == data, (len(data), piece_bytes)
            assert got[:2] == b"\x78\x01" and int.from_bytes(got[-4:], "big") == zlib.adler32(data)
            assert len(got) <= pm.pieces_bound(len(data), piece_bytes)


def test_a_non_last_piece_ends_on_the_marker_and_has_no_final_block():
    data = small_inputs()[6]
    for level in (1, 3, 6):
        p = pm.piece(data[:300], level, False)
        assert p.endswith(pm.SYNC)
        out, d = inflate_raw(p)
        assert out == data[:300] and not d.eof                         # the stream goes on
        out, d = inflate_raw(p, pm.piece(data[300:], level, True))
        assert out == data and d.eof and d.unused_data == b""
    assert pm.piece(b"", 1, False) == b"\x00" + pm.SYNC and pm.piece(b"", 1, True) == b"\x03\x00"
    assert pm.compress(b"", 5, 64) == b"\x78\x01\x03\x00\x00\x00\x00\x01"


@pytest.mark.parametrize("level", sorted(pm.TWO_BLOCK))
def test_the_pinned_inputs_keep_two_blocks_in_a_non_last_piece(level):
    data, non_last, last, blocks = pm.two_block_pieces(level)
    assert blocks == pm.TWO_BLOCK[level][1], "the model writes %d blocks at level %d" % (blocks, level)
    assert blocks >= 2
    out, d = inflate_raw(non_last)
    assert out == data and not d.eof and non_last.endswith(pm.SYNC)
    out, d = inflate_raw(last)
    assert out == data and d.eof
    # the same bits but for BFINAL and the ends
    assert len(non_last) in (len(last) + 4, len(last) + 5)
    diff = [i for i in range(len(last) - 1) if non_last[i] != last[i]]
    assert len(diff) == 1                            # the one byte that holds the final block's BFINAL


def test_the_combine_rule_on_the_0xff_payloads():
    """adler_payloads' worst case through the rule the plan kernel uses, in plain integers."""
    data = adler_payloads.ff(300000)
    want = zlib.adler32(data)
    for piece_bytes in PIECE_SIZES:
        assert pm.adler_of_pieces(data, piece_bytes) == want, piece_bytes
    for size in (0, 1, 63, 64, 65, 5552, 5553, 65520, 65521, 65522, 131072):
        for piece_bytes in PIECE_SIZES:
            assert pm.adler_of_pieces(data[:size], piece_bytes) == zlib.adler32(data[:size]), (size, piece_bytes)
    # associative: any grouping of three runs
    runs = [(zlib.adler32(x) & 0xFFFF, zlib.adler32(x) >> 16, len(x) % pm.MOD) for x in (data[:70000], data[70000:70001], data[70001:])]
    assert pm.adler_join(pm.adler_join(runs[0], runs[1]), runs[2]) == pm.adler_join(runs[0], pm.adler_join(runs[1], runs[2]))
    assert pm.adler_join((1, 0, 0), runs[0]) == runs[0] == pm.adler_join(runs[0], (1, 0, 0))


def test_counts_and_bounds_of_the_model():
    assert [pm.pieces_count(n, 64) for n in (0, 1, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert pm.cuts(0, 64) == [(0, 0)] and pm.cuts(130, 64) == [(0, 64), (64, 128), (128, 130)]
    assert pm.pieces_bound(0, 64) == 2 + 1024 + 4 and pm.pieces_bound(130, 64) == 2 + 2 * (64 + 32 + 1024) + (2 + 1 + 1024) + 4
