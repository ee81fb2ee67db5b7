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


def test_signature_table_agrees_with_the_header():
    """Parameter count, the class of every parameter and of the result, the element width of every device pointer and
    the place of the stream (abi_header.check_table)."""
    from fdeflate_amd import _lib
    protos = abi_header.check_table(os.path.join(ROOT, "include", "fdeflate_hip.h"), _lib.SIGNATURES)
    assert set(protos) == set(_declared_symbols()) == set(_lib.SIGNATURES) and len(protos) == 65
    assert _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES)


HEADERS = {"fdeflate_hip.h": ("SIGNATURES", 65), "fdeflate_hip_png16.h": ("EXTENSION_SIGNATURES", 3),
           "fdeflate_hip_png16_encode.h": ("PNG16_ENCODE_SIGNATURES", 4), "fdeflate_hip_levels.h": ("LEVELS_SIGNATURES", 3),
           "fdeflate_hip_png_levels.h": ("PNG_LEVELS_SIGNATURES", 3), "fdeflate_hip_pieces.h": ("PIECES_SIGNATURES", 5)}


def test_tables_holds_every_header_of_include_with_its_named_table():
    """_lib.TABLES is the six headers in the order they were added, each with the table the tests know by name; no symbol
    is in two tables, and signature() finds every symbol in the table that owns it.  (One test, not one case per header:
    it stands for the five per-header tests of the tables' arrangement that it replaced.)"""
    from fdeflate_amd import _lib
    assert list(_lib.TABLES) == list(HEADERS)
    assert sorted(_lib.TABLES) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    names = [name for table in _lib.TABLES.values() for name in table]
    assert len(names) == len(set(names)) == 83
    assert _lib.EXPORTED_SYMBOLS == list(_lib.SIGNATURES)
    with pytest.raises(KeyError):
        _lib.signature("fdh_debug_general_plan")                    # exported, but declared by no header
    for header, (name, count) in HEADERS.items():
        table = getattr(_lib, name)
        assert _lib.TABLES[header] is table and len(table) == count, header
        assert os.path.exists(os.path.join(ROOT, "include", header)), header
        for symbol, entry in table.items():
            assert _lib.signature(symbol) is entry, symbol


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
