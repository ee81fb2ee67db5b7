"""CPU-side checks of the fourth extension boundary: include/fdeflate_hip_png_levels.h against
_lib.PNG_LEVELS_SIGNATURES with the checks tests/test_abi_levels.py makes of the third, the bounds against their Python
mirror, the refusals that need no device, and fdeflate_amd.png_levels as a module."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_png_levels.h")
SYMBOLS = ("fdh_png_filter_mixed_batch", "fdh_png_level_bound", "fdh_png_level_file_bound")
NAMES = ("PNG_FILTER_GIVEN_TYPES", "level_bound", "level_file_bound", "png_filter_mixed_batch", "png_encode_mixed_files_level_batch",
         "png_encode_mixed_rgba_files_level_batch", "png_encode_mixed_rgba16_files_level_batch")
LENGTHS = (0, 1, 65535, 65536, 1 << 30)


def test_header_includes_the_headers_it_extends_and_carries_the_contract():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip.h"' in text and '#include "fdeflate_hip_levels.h"' in text and "#ifndef FDEFLATE_HIP_PNG_LEVELS_H" in text
    comment = text[:text.index("#ifndef")]
    for symbol in SYMBOLS:
        assert symbol in comment, symbol
    assert "no new status value" in comment and "FDH_PNG_FILTER_GIVEN_TYPES" in comment
    assert re.search(r"#define FDH_PNG_FILTER_GIVEN_TYPES 1u\b", text)


def test_table_agrees_with_the_header():
    from fdeflate_amd import _lib
    protos = abi_header.check_table(HEADER, _lib.PNG_LEVELS_SIGNATURES)
    assert set(protos) == set(SYMBOLS) and all(result in abi_header.SCALARS for result, _ in protos.values())
    # the filter call is fdh_png_filter_batch's slots with the record, the gate and the flags where that has row_bytes and bpp
    mixed, uniform = _lib.PNG_LEVELS_SIGNATURES["fdh_png_filter_mixed_batch"][1], _lib.SIGNATURES["fdh_png_filter_batch"][1]
    assert mixed[:6] == uniform[:6] and mixed[6:] == ("4", "4", "u32", "4", "u64", "stream")


def test_library_exports_every_declared_symbol_with_its_prototype():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export " + name
        assert len(getattr(L, name).argtypes) == len(_lib.PNG_LEVELS_SIGNATURES[name][1])
    assert L.fdh_png_filter_mixed_batch.restype is ctypes.c_int
    assert L.fdh_png_level_bound.restype is ctypes.c_uint64 and L.fdh_png_level_file_bound.restype is ctypes.c_uint64
    assert L.fdh_png_filter_mixed_batch.argtypes[8] is ctypes.c_uint32 and L.fdh_png_filter_mixed_batch.argtypes[10] is ctypes.c_uint64


def _stored(n):
    blocks, rest = divmod(n, 65535)
    return 2 + blocks * 65540 + (5 + rest if rest else 2) + 4


@pytest.mark.parametrize("level", [0, 1, 9])
def test_bounds_against_the_python_mirror(level):
    import fdeflate_amd as fd
    import fdeflate_amd.png_levels as pl
    from fdeflate_amd import _lib
    L = _lib.lib()
    for n in LENGTHS:
        want = _stored(n) if level == 0 else n + n // 2 + 1024
        assert L.fdh_png_level_bound(n, level) == want == pl.level_bound(n, level)
        assert want == (fd.stored_size(n) if level == 0 else fd.compress_bound(n))
    for rows, rb, prefix in ((1, 1, 41), (40, 144, 41), (64, 1023, 41), (9, 5, 56), (1, (1 << 30) - 1, 41 + 12 + 768 + 12 + 256)):
        want = prefix + pl.level_bound(rows * (rb + 1), level) + 16
        assert L.fdh_png_level_file_bound(rows, rb, level, prefix) == want == pl.level_file_bound(rows, rb, level, prefix)
    assert pl.level_file_bound(40, 144, level) == pl.level_file_bound(40, 144, level, 41)


def test_the_tensor_bound_is_the_same_arithmetic():
    import torch
    import fdeflate_amd.png_levels as pl
    sizes = torch.tensor(LENGTHS + (65534, 131070, 131071), dtype=torch.int64)
    for level in (0, 1, 9):
        got = pl.level_bound(sizes, level)
        assert got.dtype == torch.int64 and got.tolist() == [pl.level_bound(int(n), level) for n in sizes.tolist()]


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """A level above 9 has no bound; null info / pix_off / filt_off / png_status (and the other pointers the call cannot do
    without), flags it does not know, n above 2^31-1: FDH_ERR_INVALID_ARGUMENT with a message, with no GPU; an empty
    batch is success."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for level in (10, 11, 255, 0xFFFFFFFF):
        assert L.fdh_png_level_bound(100, level) == 0 and L.fdh_png_level_file_bound(4, 4, level, 41) == 0
    meta = (ctypes.c_uint64 * 8)()      # host memory standing in for every pointer: refused before it is looked at
    p = ctypes.cast(meta, ctypes.c_void_p)
    good = [p, p, p, p, p, p, p, None, 0, p, 1]      # pix, pix_off, types, types_off, filt, filt_off, info, upstream, flags, status, n
    assert L.fdh_png_filter_mixed_batch(*[None] * 8, 0, None, 0, None) == 0                     # an empty batch
    assert L.fdh_png_filter_mixed_batch(*[None] * 8, 1, None, 0, None) == 0
    for pos in (0, 1, 4, 5, 6, 9):
        args = list(good)
        args[pos] = None
        assert L.fdh_png_filter_mixed_batch(*args, None) == 1 and b"null" in L.fdh_last_error(), pos
    for types, types_off, flags in ((p, None, 0), (None, p, 0), (None, None, 1)):
        args = list(good)
        args[2], args[3], args[8] = types, types_off, flags
        assert L.fdh_png_filter_mixed_batch(*args, None) == 1 and b"null" in L.fdh_last_error()
    for flags in (2, 3, 0x80000000):
        args = list(good)
        args[8] = flags
        assert L.fdh_png_filter_mixed_batch(*args, None) == 1 and b"flags" in L.fdh_last_error()
        args[10] = 0
        assert L.fdh_png_filter_mixed_batch(*args, None) == 1                                   # ... whatever n is
    args = list(good)
    args[10] = 1 << 31
    assert L.fdh_png_filter_mixed_batch(*args, None) == 1 and b"too many" in L.fdh_last_error()


def test_module_names_exist_and_the_package_surface_is_unchanged():
    import fdeflate_amd
    import fdeflate_amd.png_levels as pl
    assert sorted(pl.__all__) == sorted(NAMES) and pl.PNG_FILTER_GIVEN_TYPES == 1
    for name in pl.__all__:
        if name != "PNG_FILTER_GIVEN_TYPES":
            assert callable(getattr(pl, name)) and getattr(pl, name).__doc__, name
    assert len(fdeflate_amd.__all__) == 100 and not set(NAMES) & set(fdeflate_amd.__all__)
    for level in (10, -1, True, "6", 2.0, None):
        with pytest.raises(ValueError):
            pl.level_bound(100, level)
        with pytest.raises(ValueError):
            pl.level_file_bound(4, 4, level)
        for call in (pl.png_encode_mixed_files_level_batch, pl.png_encode_mixed_rgba_files_level_batch,
                     pl.png_encode_mixed_rgba16_files_level_batch):
            with pytest.raises(ValueError):         # before any argument is looked at, let alone a device
                call(None, None, None, level) if call is pl.png_encode_mixed_files_level_batch else call(None, None, None, None, level)


def test_import_of_the_module_does_not_import_torch():
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd.png_levels; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)
