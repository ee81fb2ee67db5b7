"""CPU-side checks of the extension boundary: include/fdeflate_hip_png16.h against _lib.EXTENSION_SIGNATURES with the
checks tests/test_abi.py makes of the main header, the library's exports, and fdeflate_amd.png16 as a module."""
import ctypes
import os
import re
import subprocess
import sys

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdeflate_hip_png16.h")
SYMBOLS = ("fdh_png_expand16_batch", "fdh_png_expand16_mixed_batch", "fdh_png_pack16_batch")


def _declared_prototypes():
    """{symbol: (result, [parameter, ...])} as the extension header spells them (test_abi._declared_prototypes on it)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for result, name, params in re.findall(r"([^;{}]*?)\b(fdh_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        params = [" ".join(p.split()) for p in params.split(",")]
        protos[name] = (" ".join(result.split()).replace('extern "C"', "").strip(), [] if params == ["void"] else params)
    return protos


def test_extension_header_includes_the_main_one():
    text = open(HEADER).read()
    assert '#include "fdeflate_hip.h"' in text and "FDEFLATE_HIP_PNG16_H" in text


def test_extension_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream, as test_abi.test_signature_table_agrees_with_the_header checks them."""
    from fdeflate_amd import _lib
    protos = _declared_prototypes()
    assert set(protos) == set(_lib.EXTENSION_SIGNATURES) == set(SYMBOLS)
    for name, (result, params) in protos.items():
        t_result, t_params = _lib.EXTENSION_SIGNATURES[name]
        assert "*" not in result and t_result == abi_header.SCALARS[result], name
        assert len(t_params) == len(params), name
        for pos, (token, param) in enumerate(zip(t_params, params)):
            where = "%s, parameter %d (%s)" % (name, pos, param)
            pointee = abi_header.pointee(param)
            if pointee is None:
                assert token == abi_header.SCALARS[param.split()[0]], where
            elif token in _lib.DEVICE_WIDTH:
                assert param.count("*") == 1 and "[" not in param, where
                assert _lib.DEVICE_WIDTH[token] == abi_header.POINTEE_BYTES[pointee], where
            else:
                assert token == ("stream" if param == "void *hip_stream" else "host"), where
        assert ("stream" in t_params) == (t_params[-1:] == ("stream",)) == (params[-1:] == ["void *hip_stream"]), name


def test_no_symbol_is_in_both_tables_and_the_main_table_is_what_it_was():
    from fdeflate_amd import _lib
    assert not set(_lib.SIGNATURES) & set(_lib.EXTENSION_SIGNATURES)
    assert _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 65
    for name in SYMBOLS:
        assert _lib.signature(name) == _lib.EXTENSION_SIGNATURES[name]
    assert _lib.signature("fdh_png_expand_batch") == _lib.SIGNATURES["fdh_png_expand_batch"]


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
