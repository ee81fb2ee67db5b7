"""CPU-side checks of the fifth extension boundary: include/fdeflate_hip_pieces.h against _lib.PIECES_SIGNATURES with the
checks tests/test_abi_png_levels.py makes of the fourth, the host arithmetic against tests/pieces_model.py and its torch
mirror, the refusals that need no device, and fdeflate_amd.pieces as a module."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import abi_header
import pieces_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_pieces.h")
SYMBOLS = ("fdh_deflate_level_pieces_batch", "fdh_deflate_stitch_batch", "fdh_deflate_pieces_count", "fdh_deflate_pieces_bound",
           "fdh_png_level_pieces_file_bound")
NAMES = ("PIECE_BYTES_DEFAULT", "PIECE_BYTES_MIN", "PIECE_BYTES_MAX", "pieces_count", "pieces_bound", "pieces_file_bound",
         "deflate_level_pieces_raw_batch", "deflate_stitch_batch", "deflate_level_pieces_batch", "compress_to_vec_level_pieces",
         "png_encode_mixed_files_level_pieces_batch", "png_encode_mixed_rgba_files_level_pieces_batch",
         "png_encode_mixed_rgba16_files_level_pieces_batch")
SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 65535, 65536, 65537, 4 << 20, (1 << 30) + 1)
PIECE_SIZES = (64, 65, 1000, 4096, 65536, 1 << 30)
BAD_PIECE_SIZES = (0, 1, 63, (1 << 30) + 1, 1 << 40)


def test_header_includes_the_headers_it_extends_and_carries_the_contract():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip.h"' in text and '#include "fdeflate_hip_levels.h"' in text and "#ifndef FDEFLATE_HIP_PIECES_H" in text
    comment = text[:text.index("#ifndef")]
    for symbol in SYMBOLS:
        assert symbol in comment, symbol
    assert "no new status value" in comment and "Flush::Sync" in comment and "00 00 FF FF" in comment
    assert "fdh_compress_bound" in comment and "slack" in comment       # where the marker's five bytes fit
    assert re.search(r"#define FDH_PIECE_BYTES_MIN 64u\b", text) and re.search(r"#define FDH_PIECE_BYTES_DEFAULT 65536u\b", text)


def test_table_agrees_with_the_header():
    from fdeflate_amd import _lib
    protos = abi_header.check_table(HEADER, _lib.PIECES_SIGNATURES)
    assert set(protos) == set(SYMBOLS) and all(result in abi_header.SCALARS for result, _ in protos.values())
    # the piece encoder is fdh_deflate_level_batch with the last flags behind the offsets and the checksums behind out_len
    piece, stream = _lib.PIECES_SIGNATURES["fdh_deflate_level_pieces_batch"][1], _lib.LEVELS_SIGNATURES["fdh_deflate_level_batch"][1]
    assert piece[:2] + piece[3:6] + piece[7:] == stream and piece[2] == "1" and piece[6] == "4"


def test_library_exports_every_declared_symbol_with_its_prototype():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export " + name
        assert len(getattr(L, name).argtypes) == len(_lib.PIECES_SIGNATURES[name][1])
    assert L.fdh_deflate_level_pieces_batch.restype is ctypes.c_int and L.fdh_deflate_stitch_batch.restype is ctypes.c_int
    for name in SYMBOLS[2:]:
        assert getattr(L, name).restype is ctypes.c_uint64
    assert L.fdh_deflate_level_pieces_batch.argtypes[7:9] == [ctypes.c_uint64, ctypes.c_uint32]


@pytest.mark.parametrize("piece_bytes", PIECE_SIZES)
def test_counts_and_bounds_against_the_model_and_the_torch_mirror(piece_bytes):
    import torch
    import fdeflate_amd.pieces as pc
    import fdeflate_amd.png_levels as pl
    from fdeflate_amd import _lib
    L = _lib.lib()
    sizes = [n for n in SIZES if n // piece_bytes < 100000]         # (the model lists the pieces)
    t = torch.tensor(sizes, dtype=torch.int64)
    assert pc.pieces_count(t, piece_bytes).tolist() == [pm.pieces_count(n, piece_bytes) for n in sizes]
    for n in sizes:
        assert L.fdh_deflate_pieces_count(n, piece_bytes) == pm.pieces_count(n, piece_bytes) == pc.pieces_count(n, piece_bytes)
    for level in (0, 1, 6, 9):
        want = [pl.level_bound(n, 0) if level == 0 else pm.pieces_bound(n, piece_bytes) for n in sizes]
        assert [L.fdh_deflate_pieces_bound(n, level, piece_bytes) for n in sizes] == want
        assert [pc.pieces_bound(n, level, piece_bytes) for n in sizes] == want
        got = pc.pieces_bound(t, level, piece_bytes)
        assert got.dtype == torch.int64 and got.tolist() == want
        # one piece: the one-shot slot and the six bytes of header and trailer, which the piece does without
        for n in sizes:
            if level and n <= piece_bytes:
                assert pc.pieces_bound(n, level, piece_bytes) == pl.level_bound(n, level) + 6
        for rows, rb, prefix in ((1, 1, 41), (40, 144, 41), (64, 1023, 41), (9, 5, 56), (1024, 4096, 41)):
            want = prefix + pc.pieces_bound(rows * (rb + 1), level, piece_bytes) + 16
            assert L.fdh_png_level_pieces_file_bound(rows, rb, level, piece_bytes, prefix) == want
            assert pc.pieces_file_bound(rows, rb, level, piece_bytes, prefix) == want
    assert pc.pieces_file_bound(40, 144, 6, piece_bytes) == pc.pieces_file_bound(40, 144, 6, piece_bytes, 41)


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """A piece size below 64 or above 2^30 and a level above 9 have no count and no bound; the piece encoder refuses level
    0 and levels above 9, null metadata and n above 2^31-1, the stitch null pointers, n above 2^31-1 and one buffer for
    both sides: FDH_ERR_INVALID_ARGUMENT with a message, with no GPU; an empty batch is success."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for piece_bytes in BAD_PIECE_SIZES:
        assert L.fdh_deflate_pieces_count(1000, piece_bytes) == 0
        assert L.fdh_deflate_pieces_bound(1000, 6, piece_bytes) == 0 and L.fdh_deflate_pieces_bound(1000, 0, piece_bytes) == 0
        assert L.fdh_png_level_pieces_file_bound(4, 4, 6, piece_bytes, 41) == 0
    for level in (10, 11, 255, 0xFFFFFFFF):
        assert L.fdh_deflate_pieces_bound(1000, level, 65536) == 0 and L.fdh_png_level_pieces_file_bound(4, 4, level, 65536, 41) == 0
    meta = (ctypes.c_uint64 * 8)()      # host memory standing in for every pointer: refused before it is looked at
    p = ctypes.cast(meta, ctypes.c_void_p)
    for level in (0, 10, 255, 0xFFFFFFFF):
        for n in (0, 1):
            assert L.fdh_deflate_level_pieces_batch(*[None] * 7, n, level, None) == 1 and b"level" in L.fdh_last_error()
            assert L.fdh_deflate_level_pieces_batch(p, p, p, p, p, p, p, n, level, None) == 1 and b"level" in L.fdh_last_error()
    for level in range(1, 10):
        assert L.fdh_deflate_level_pieces_batch(*[None] * 7, 0, level, None) == 0                       # an empty batch
        for pos in (1, 2, 3, 4, 5, 6):
            args = [p] * 7
            args[pos] = None
            assert L.fdh_deflate_level_pieces_batch(*args, 3, level, None) == 1 and b"null" in L.fdh_last_error(), pos
        assert L.fdh_deflate_level_pieces_batch(*[p] * 7, 1 << 31, level, None) == 1 and b"too many" in L.fdh_last_error()
    assert L.fdh_deflate_stitch_batch(*[None] * 9, 0, None) == 0                                        # an empty batch
    q = ctypes.cast((ctypes.c_uint64 * 8)(), ctypes.c_void_p)
    good = [p, p, p, p, p, p, q, p, p]
    for pos in range(9):
        args = list(good)
        args[pos] = None
        assert L.fdh_deflate_stitch_batch(*args, 1, None) == 1 and b"null" in L.fdh_last_error(), pos
    assert L.fdh_deflate_stitch_batch(*good, 1 << 31, None) == 1 and b"too many" in L.fdh_last_error()
    same = list(good)
    same[6] = same[0]
    assert L.fdh_deflate_stitch_batch(*same, 1, None) == 1 and b"same buffer" in L.fdh_last_error()


def test_module_names_exist_and_the_package_surface_is_unchanged():
    import fdeflate_amd
    import fdeflate_amd.pieces as pc
    import fdeflate_amd.png_levels as pl
    assert sorted(pc.__all__) == sorted(NAMES)
    assert (pc.PIECE_BYTES_MIN, pc.PIECE_BYTES_DEFAULT, pc.PIECE_BYTES_MAX) == (64, 65536, 1 << 30)
    for name in pc.__all__:
        if not name.startswith("PIECE_BYTES"):
            assert callable(getattr(pc, name)) and getattr(pc, name).__doc__, name
    assert len(fdeflate_amd.__all__) == 100 and not set(NAMES) & set(fdeflate_amd.__all__)
    assert not set(NAMES) & set(pl.__all__) and len(pl.__all__) == 7
    for level in (10, -1, True, "6", 2.0, None):
        with pytest.raises(ValueError):
            pc.pieces_bound(100, level)
        with pytest.raises(ValueError):
            pc.compress_to_vec_level_pieces(b"x", level)
        for call in (pc.png_encode_mixed_files_level_pieces_batch, pc.png_encode_mixed_rgba_files_level_pieces_batch,
                     pc.png_encode_mixed_rgba16_files_level_pieces_batch):
            with pytest.raises(ValueError):         # before any argument is looked at, let alone a device
                call(None, None, None, level) if call is pc.png_encode_mixed_files_level_pieces_batch else call(None, None, None, None, level)
    for piece_bytes in BAD_PIECE_SIZES + (True, 100.0, "64", None):
        with pytest.raises(ValueError):
            pc.pieces_count(100, piece_bytes)
        with pytest.raises(ValueError):
            pc.pieces_bound(100, 6, piece_bytes)
        with pytest.raises(ValueError):
            pc.compress_to_vec_level_pieces(b"x", 6, piece_bytes)
        with pytest.raises(ValueError):
            pc.deflate_level_pieces_batch(None, None, None, None, 6, piece_bytes)
        with pytest.raises(ValueError):
            pc.png_encode_mixed_rgba_files_level_pieces_batch(None, None, None, None, 6, piece_bytes=piece_bytes)
    with pytest.raises(ValueError):
        pc.deflate_level_pieces_raw_batch(None, None, None, None, None, 0)          # level 0: no piece mode


def test_no_cpu_fallback():
    """Without a device the calls raise (with one: tests/test_gpu_pieces.py has the bytes)."""
    import torch
    import fdeflate_amd.pieces as pc
    from fdeflate_amd._lib import FdeflateHipError
    if not torch.cuda.is_available():
        for level in (0, 1, 6):
            with pytest.raises(FdeflateHipError):
                pc.compress_to_vec_level_pieces(b"x" * 200, level, 64)


def test_import_of_the_module_does_not_import_torch():
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd.pieces; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)
