"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol that
include/fdeflate_hip.h declares, and refuses to do work without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fdh_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from fdeflate_amd import _lib
    L = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(L, s), "missing export " + s
    assert set(syms) == set(_lib.EXPORTED_SYMBOLS)
    assert L.fdh_version() == 0x000100
    assert L.fdh_status_name(15) == b"WrongChecksum" and L.fdh_status_name(17) == b"OutputTooLarge"
    assert L.fdh_ultrafast_bound(0) == 60 and L.fdh_ultrafast_bound(65536) == 98364


def _declared_prototypes():
    """{symbol: (result, [parameter, ...])} as the header spells them, comments and preprocessor lines taken out."""
    text = open(os.path.join(ROOT, "include", "fdeflate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for result, name, params in re.findall(r"([^;{}]*?)\b(fdh_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        params = [" ".join(p.split()) for p in params.split(",")]
        protos[name] = (" ".join(result.split()), [] if params == ["void"] else params)
    return protos


def test_signature_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream: a miscounted table entry would be undefined behaviour at the call, not an error."""
    from fdeflate_amd import _lib
    protos = _declared_prototypes()
    assert set(protos) == set(_declared_symbols()) == set(_lib.SIGNATURES) and len(protos) == 65
    assert _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES)
    for name, (result, params) in protos.items():
        t_result, t_params = _lib.SIGNATURES[name]
        if "*" in result:
            assert t_result == ("str" if result == "const char *" else "host"), name
        else:
            assert t_result == ("void" if result == "void" else abi_header.SCALARS[result]), name
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
                assert token == ("stream" if param == "void *hip_stream" else "host"), where   # exempt from the widths
        assert ("stream" in t_params) == (t_params[-1:] == ("stream",)) == (params[-1:] == ["void *hip_stream"]), name


def test_library_prototypes_are_set_from_the_table():
    from fdeflate_amd import _lib
    L = _lib.lib()
    assert L.fdh_free.restype is None and L.fdh_free.argtypes == [ctypes.c_void_p]
    assert L.fdh_crc32_batch.restype is ctypes.c_int and len(L.fdh_crc32_batch.argtypes) == 8
    assert L.fdh_png_adam7_size.argtypes == [ctypes.c_uint32] * 4 and L.fdh_png_adam7_size.restype is ctypes.c_uint64
    assert L.fdh_decompress_to_vec_bounded.argtypes[1:3] == [ctypes.c_size_t] * 2
    assert hasattr(L, "fdh_debug_lost_records") and "fdh_debug_lost_records" not in _lib.SIGNATURES


def test_import_of_the_package_does_not_import_torch():
    import subprocess
    import sys
    subprocess.run([sys.executable, "-c", "import sys, fdeflate_amd; assert 'torch' not in sys.modules"], cwd=ROOT, check=True)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import fdeflate_amd as fd
    from fdeflate_amd._lib import FdeflateHipError
    with pytest.raises(FdeflateHipError):
        fd.decompress_to_vec(b"\x78\x01\x03\x00\x00\x00\x00\x01")
    with pytest.raises(FdeflateHipError):
        fd.compress_to_vec_ultra_fast(b"abc")


def test_product_does_not_link_or_import_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "fdeflate_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".inc")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_binding" not in text and "fdeflate_oracle" not in text and "libfdeflate_oracle" not in text, f


def test_synth_numpy_is_deterministic_and_shaped():
    from fdeflate_amd import synth
    a = synth.gen_stream_np(0, 65536)
    b = synth.gen_stream_np(0, 65536)
    assert (a == b).all() and a.size == 65536
    assert (synth.gen_stream_np(15, 4096) == 0).all()
    z = (a == 0).mean()
    assert 0.2 < z < 0.35  # model D: 27 % zeros
    assert set(a[::1024].tolist()) <= {0, 1, 2, 3, 4}  # filter-type byte per scanline
