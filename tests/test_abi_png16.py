"""CPU-side checks of the extension boundary: include/fdeflate_hip_png16.h against _lib.EXTENSION_SIGNATURES with the
checks tests/test_abi.py makes of the main header, the library's exports, and fdeflate_amd.png16 as a module."""
import ctypes
import os
import subprocess
import sys

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_png16.h")
SYMBOLS = ("fdh_png_expand16_batch", "fdh_png_expand16_mixed_batch", "fdh_png_pack16_batch")


def test_extension_header_includes_the_main_one():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip.h"' in text and "FDEFLATE_HIP_PNG16_H" in text


def test_extension_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream, as test_abi.test_signature_table_agrees_with_the_header checks them."""
    from fdeflate_amd import _lib
    protos = abi_header.check_table(HEADER, _lib.EXTENSION_SIGNATURES)
    assert set(protos) == set(SYMBOLS) and all(result in abi_header.SCALARS for result, _ in protos.values())


def test_library_exports_every_declared_symbol_with_its_prototype():
    from fdeflate_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export " + name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.EXTENSION_SIGNATURES[name][1])
    assert L.fdh_png_pack16_batch.argtypes[6:9] == [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """Colour type 3 (and 1, 5, 7) for pack16, an illegal pair or width for expand16: FDH_ERR_INVALID_ARGUMENT with a
    message, whatever the pointers are and with no GPU."""
    from fdeflate_amd import _lib
    L = _lib.lib()
    for colour in (3, 1, 5, 7):
        assert L.fdh_png_pack16_batch(None, None, None, None, None, None, 0, 5, colour, None) != 0
        assert b"colour type" in L.fdh_last_error()
    assert L.fdh_png_pack16_batch(None, None, None, None, None, None, 0, 0, 6, None) != 0
    assert L.fdh_png_pack16_batch(None, None, None, None, None, None, 0, 5, 6, None) == 0          # an empty batch
    assert L.fdh_png_expand16_batch(None, None, None, None, None, None, None, None, 0, 5, 16, 3, None) != 0
    assert L.fdh_png_expand16_batch(None, None, None, None, None, None, None, None, 0, 0, 16, 6, None) != 0
    assert L.fdh_png_expand16_batch(None, None, None, None, None, None, None, None, 0, 5, 16, 6, None) == 0


def test_module_names_exist_and_the_package_surface_is_unchanged():
    import fdeflate_amd
    import fdeflate_amd.png16 as p16
    assert sorted(p16.__all__) == sorted(["png_expand16_batch", "png_expand16_mixed_batch", "png_pack16_batch",
                                          "png_decode_files_rgba16_batch", "png_decode_mixed_files_rgba16_batch",
                                          "png_encode_rgba16_files_batch"])
    for name in p16.__all__:
        assert callable(getattr(p16, name)) and getattr(p16, name).__doc__, name
        assert name not in fdeflate_amd.__all__


def test_import_of_the_module_does_not_import_torch():
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd.png16; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)
