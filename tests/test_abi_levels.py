"""CPU-side checks of the third extension boundary: include/fdeflate_hip_levels.h against _lib.LEVELS_SIGNATURES with the
checks tests/test_abi_png16_encode.py makes of the second extension, the library's exports, the refusals that need no
device, and fdeflate_amd.levels as a module."""
import ctypes
import os
import subprocess
import sys

import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_levels.h")
SYMBOLS = ("fdh_deflate_level_batch", "fdh_compress_to_vec_level", "fdh_debug_level_plan")
NAMES = ("LEVELS_PROVIDED", "compress_to_vec_with_level", "deflate_level_batch", "level_plan")


def test_header_includes_the_main_header_and_carries_the_contract():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip.h"' in text and "#ifndef FDEFLATE_HIP_LEVELS_H" in text
    comment = text[:text.index("#ifndef")]
    for symbol in SYMBOLS:
        assert symbol in comment, symbol
    assert "no new status value" in comment and "deviates from the reference" in comment


def test_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream.  The batch call has fdh_deflate_general_batch's prototype, the one-shot
    fdh_compress_to_vec_with_level's."""
    from fdeflate_amd import _lib
    protos = abi_header.check_table(HEADER, _lib.LEVELS_SIGNATURES)
    assert set(protos) == set(SYMBOLS) and all(result in abi_header.SCALARS for result, _ in protos.values())
    assert _lib.LEVELS_SIGNATURES["fdh_deflate_level_batch"] == _lib.SIGNATURES["fdh_deflate_general_batch"]
    assert _lib.LEVELS_SIGNATURES["fdh_compress_to_vec_level"] == _lib.SIGNATURES["fdh_compress_to_vec_with_level"]


def test_library_exports_every_declared_symbol_with_its_prototype():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export " + name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(_lib.LEVELS_SIGNATURES[name][1])
    assert L.fdh_deflate_level_batch.argtypes[5:7] == [ctypes.c_uint64, ctypes.c_uint32]
    assert L.fdh_compress_to_vec_level.argtypes[1:3] == [ctypes.c_size_t, ctypes.c_uint32]
    assert L.fdh_debug_level_plan.argtypes[:3] == [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32]


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """Level 10 and above, n above 2^31-1 and null metadata: FDH_ERR_INVALID_ARGUMENT with a message, whatever the
    pointers are and with no GPU; an empty batch is success at every level."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    nulls = (None,) * 5
    meta = (ctypes.c_uint64 * 4)()      # host memory standing in for the metadata: refused before it is looked at
    for level in (10, 11, 255, 0xFFFFFFFF):
        for n in (0, 1):
            assert L.fdh_deflate_level_batch(*nulls, n, level, None) == 1
            assert b"level" in L.fdh_last_error()
        out, size = ctypes.c_void_p(), ctypes.c_size_t()
        assert L.fdh_compress_to_vec_level(b"abc", 3, level, ctypes.byref(out), ctypes.byref(size)) == 1
        assert b"level" in L.fdh_last_error() and not out.value
    for level in range(10):
        assert L.fdh_deflate_level_batch(*nulls, 0, level, None) == 0                                   # an empty batch
        assert L.fdh_deflate_level_batch(*nulls, 3, level, None) == 1 and b"null" in L.fdh_last_error()
        assert L.fdh_deflate_level_batch(None, meta, None, meta, ctypes.cast(meta, ctypes.c_void_p), 1 << 31, level, None) == 1
        assert b"too many" in L.fdh_last_error()
    # the calls of the main header refuse what they refused, and say "level"
    out, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.fdh_compress_to_vec_with_level(b"abc", 3, 4, ctypes.byref(out), ctypes.byref(size)) == 1
    assert b"level" in L.fdh_last_error() and b"fdh_compress_to_vec_level" in L.fdh_last_error()


def test_module_names_exist_and_the_package_surface_is_unchanged():
    import fdeflate_amd
    import fdeflate_amd.levels as lv
    assert sorted(lv.__all__) == sorted(NAMES)
    assert lv.LEVELS_PROVIDED == tuple(range(10)) and fdeflate_amd.api.LEVELS_PROVIDED == (0, 1, 2, 3)
    for name in lv.__all__:
        if name != "LEVELS_PROVIDED":
            assert callable(getattr(lv, name)) and getattr(lv, name).__doc__, name
    assert "deflate_level_batch" not in fdeflate_amd.__all__ and "level_plan" not in fdeflate_amd.__all__
    assert fdeflate_amd.compress_to_vec_with_level is fdeflate_amd.api.compress_to_vec_with_level is not lv.compress_to_vec_with_level
    assert len(fdeflate_amd.__all__) == 100
    for level in (10, -1, 256, True, 2.0, None):
        with pytest.raises(ValueError):
            lv.compress_to_vec_with_level(b"x", level)
        with pytest.raises(ValueError):
            lv.level_plan(100, 256, level)
    with pytest.raises(ValueError):
        lv.level_plan(100, 256, 3)      # a level, but not a lazy one: no plan
    assert lv.level_plan(100, 256, 4) == (4, 25)


def test_no_cpu_fallback():
    """Without a device every level raises; with one, every level gives a zlib stream (the bytes are
    tests/test_gpu_lazy_levels.py's business)."""
    import torch
    import fdeflate_amd.levels as lv
    from fdeflate_amd._lib import FdeflateHipError
    for level in range(10):
        if torch.cuda.is_available():
            assert lv.compress_to_vec_with_level(b"x", level)[:2] == b"\x78\x01"
        else:
            with pytest.raises(FdeflateHipError):
                lv.compress_to_vec_with_level(b"x", level)


def test_import_of_the_module_does_not_import_torch():
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd.levels; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)
