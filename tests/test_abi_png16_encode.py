"""CPU-side checks of the second extension boundary: include/fdeflate_hip_png16_encode.h against
_lib.PNG16_ENCODE_SIGNATURES with the checks tests/test_abi_png16.py makes of the first extension, the library's exports,
and fdeflate_amd.png16_encode as a module."""
import ctypes
import os
import subprocess
import sys

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_png16_encode.h")
SYMBOLS = ("fdh_png_analyse16_mixed_batch", "fdh_png_encode16_plan_one", "fdh_png_encode16_plan_batch", "fdh_png_pack16_mixed_batch")
NAMES = ("png_analyse16_mixed_batch", "png_encode16_plan_one", "png_encode16_plan_batch", "png_pack16_mixed_batch",
         "png_encode_mixed_rgba16_files_batch")


def test_header_includes_the_first_extension_and_carries_the_contract():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip_png16.h"' in text and "#ifndef FDEFLATE_HIP_PNG16_ENCODE_H" in text
    comment = text[:text.index("#ifndef")]
    for symbol in SYMBOLS:
        assert symbol in comment, symbol
    assert "no new status value" in comment


def test_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream, as test_abi_png16.test_extension_table_agrees_with_the_header checks them."""
    from fdeflate_amd import _lib
    protos = abi_header.check_table(HEADER, _lib.PNG16_ENCODE_SIGNATURES)
    assert set(protos) == set(SYMBOLS) and all(result in abi_header.SCALARS for result, _ in protos.values())
    # the two plans have the prototypes of the RGBA8 plans
    assert _lib.PNG16_ENCODE_SIGNATURES["fdh_png_encode16_plan_one"] == _lib.SIGNATURES["fdh_png_encode_plan_one"]
    assert _lib.PNG16_ENCODE_SIGNATURES["fdh_png_encode16_plan_batch"] == _lib.SIGNATURES["fdh_png_encode_plan_batch"]


def test_library_exports_every_declared_symbol_with_its_prototype():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export " + name
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_uint32 if name.endswith("_one") else ctypes.c_int)
        assert len(fn.argtypes) == len(_lib.PNG16_ENCODE_SIGNATURES[name][1])
    assert L.fdh_png_analyse16_mixed_batch.argtypes[9:11] == [ctypes.c_uint64, ctypes.c_uint32]


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """max_colours outside 1 .. 256, allowed bits of colour types that do not exist and n above 2^31-1:
    FDH_ERR_INVALID_ARGUMENT with a message, whatever the pointers are and with no GPU."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    nulls = (None,) * 9
    for max_colours in (0, 257, 0xFFFFFFFF):
        assert L.fdh_png_analyse16_mixed_batch(*nulls, 0, max_colours, None) != 0
        assert b"max_colours" in L.fdh_last_error()
    assert L.fdh_png_analyse16_mixed_batch(*nulls, 1 << 31, 256, None) != 0
    assert b"too many" in L.fdh_last_error()
    assert L.fdh_png_analyse16_mixed_batch(*nulls, 0, 1, None) == 0 and L.fdh_png_analyse16_mixed_batch(*nulls, 0, 256, None) == 0
    for allowed in (2, 32, 128, 0x5D | 0x100):
        assert L.fdh_png_encode16_plan_batch(None, None, None, None, None, allowed, None, None, None, None, None, 0, None) != 0
        assert b"allowed" in L.fdh_last_error()
    assert L.fdh_png_encode16_plan_batch(None, None, None, None, None, 0x5D, None, None, None, None, None, 1 << 31, None) != 0
    assert b"too many" in L.fdh_last_error()
    assert L.fdh_png_encode16_plan_batch(None, None, None, None, None, 0x5D, None, None, None, None, None, 0, None) == 0
    assert L.fdh_png_pack16_mixed_batch(*nulls, 1 << 31, None) != 0
    assert b"too many" in L.fdh_last_error()
    assert L.fdh_png_pack16_mixed_batch(*nulls, 0, None) == 0                                        # an empty batch
    assert L.fdh_png_pack16_mixed_batch(*nulls, 3, None) != 0 and b"null pointer" in L.fdh_last_error()


def test_module_names_exist_and_the_package_surface_is_unchanged():
    import fdeflate_amd
    import fdeflate_amd.png16 as p16
    import fdeflate_amd.png16_encode as p16e
    assert sorted(p16e.__all__) == sorted(NAMES)
    for name in p16e.__all__:
        assert callable(getattr(p16e, name)) and getattr(p16e, name).__doc__, name
        assert name not in fdeflate_amd.__all__ and name not in p16.__all__
    assert len(fdeflate_amd.__all__) == 100 and len(p16.__all__) == 6


def test_import_of_the_module_does_not_import_torch():
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd.png16_encode; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)
