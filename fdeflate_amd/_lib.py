"""ctypes loader for libfdeflate_hip.so (the C ABI of include/fdeflate_hip.h).

There is no fallback: if the shared library has not been built, or no GPU is usable, the
calls raise.  Build with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C fdeflate_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDH_LIB: diagnostics only (tools/segdiag.py loads an instrumented build of the same library)
SO_PATH = os.environ.get("FDH_LIB") or os.path.join(_HERE, "libfdeflate_hip.so")

_lib = None


class FdeflateHipError(RuntimeError):
    """Infrastructure failure reported by the C ABI (not a per-stream decode error)."""


# Every prototype of include/fdeflate_hip.h, once: the result, then the parameters (tests/test_abi.py compares the
# two).  1 / 4 / 8: a pointer to DEVICE memory and the bytes of one element (1 bytes, filter types, `method`; 4 uint32
# arrays and fdh_png_info / fdh_resume_point records as int32 tensors; 8 offsets and sizes) -- api._call holds a
# tensor to that width.  host: a pointer the host dereferences, or an opaque one.  stream: the closing `void *hip_stream`.
DEVICE_WIDTH = {"1": 1, "4": 4, "8": 8}
_CTYPES = {"void": None, "int": C.c_int, "u32": C.c_uint32, "u64": C.c_uint64, "size": C.c_size_t, "str": C.c_char_p,
           **dict.fromkeys(("1", "4", "8", "host", "stream"), C.c_void_p)}
SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_version": "u32",
    "fdh_status_name": "str u32",
    "fdh_last_error": "str",
    "fdh_device_count": "int",
    "fdh_ultrafast_bound": "u64 u64",
    "fdh_stored_size": "u64 u64",
    "fdh_compress_bound": "u64 u64",
    "fdh_inflate_batch": "int 1 8 1 8 4 4 4 u64 u32 stream",
    "fdh_inflate_batch_resumable": "int 1 8 1 8 4 4 4 u64 u32 4 stream",
    "fdh_deflate_ultrafast_batch": "int 1 8 1 8 4 u64 stream",
    "fdh_deflate_stored_batch": "int 1 8 1 8 4 u64 stream",
    "fdh_deflate_general_batch": "int 1 8 1 8 4 u64 u32 stream",
    "fdh_debug_build_tables": "int 1 u32 4 4 4 stream",
    "fdh_decompress_to_vec": "int host size host host host",
    "fdh_decompress_to_vec_bounded": "int host size size host host host",
    "fdh_compress_to_vec_ultra_fast": "int host size host host",
    "fdh_compress_to_vec_stored": "int host size host host",
    "fdh_compress_to_vec": "int host size host host",
    "fdh_compress_to_vec_rle": "int host size host host",
    "fdh_compress_to_vec_with_level": "int host size u32 host host",
    "fdh_free": "void host",
    "fdh_decompressor_new": "host",
    "fdh_decompressor_free": "void host",
    "fdh_decompressor_ignore_adler32": "void host",
    "fdh_decompressor_is_done": "int host",
    "fdh_decompressor_attempts": "u64 host",
    "fdh_decompressor_decoded_bytes": "u64 host",
    "fdh_decompressor_device_bytes": "u64 host",
    "fdh_decompressor_read": "int host host size host size size host host host",
    "fdh_png_unfilter_batch": "int 1 8 1 8 4 u64 u32 u32 stream",
    "fdh_png_filter_batch": "int 1 8 1 8 1 8 4 u64 u32 u32 stream",
    "fdh_png_choose_filters_batch": "int 1 8 1 8 4 u64 u32 u32 stream",
    "fdh_png_filter_deflate_ultrafast_batch": "int 1 8 1 8 1 8 4 4 u64 u32 u32 stream",
    "fdh_inflate_png_batch": "int 1 8 1 8 4 4 4 1 8 4 u64 u32 u32 u32 stream",
    "fdh_crc32_batch": "int 1 8 4 4 4 4 u64 stream",
    "fdh_png_file_bound": "u64 u64 u64",
    "fdh_png_frame_batch": "int 1 8 4 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_scan_files_batch": "int 1 8 4 4 u64 u32 stream",
    "fdh_png_gather_idat_batch": "int 1 8 4 1 8 4 4 u64 u32 u32 u32 stream",
    "fdh_png_colour_batch": "int 1 8 4 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_expand_batch": "int 1 8 1 8 4 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_adam7_size": "u64 u32 u32 u32 u32",
    "fdh_png_unfilter_interlaced_batch": "int 1 8 1 8 1 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_plan_sizes": "u32 host u64 host",
    "fdh_png_plan_batch": "int 4 u64 8 8 8 8 4 u64 stream",
    "fdh_png_gather_idat_mixed_batch": "int 1 8 4 4 1 8 4 4 u64 stream",
    "fdh_png_colour_mixed_batch": "int 1 8 4 4 4 4 4 u64 stream",
    "fdh_png_unfilter_mixed_batch": "int 1 8 1 8 4 4 4 4 u64 stream",
    "fdh_png_expand_mixed_batch": "int 1 8 1 8 4 4 4 4 4 u64 stream",
    "fdh_png_analyse_batch": "int 1 8 4 4 4 4 4 u64 u32 u32 stream",
    "fdh_png_pack_batch": "int 1 8 1 8 4 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_palette_file_prefix": "u64 u32 u32",
    "fdh_png_frame_palette_batch": "int 1 8 4 4 4 4 4 4 4 u64 u32 u32 u32 u32 stream",
    "fdh_png_encode_plan_one": "u32 host host host u32 u32 u32 host",
    "fdh_png_encode_plan_batch": "int 4 4 4 4 4 u32 8 8 8 8 4 u64 stream",
    "fdh_png_analyse_mixed_batch": "int 1 8 4 4 4 4 4 4 4 u64 u32 stream",
    "fdh_png_pack_mixed_batch": "int 1 8 1 8 4 4 4 4 4 u64 stream",
    "fdh_png_choose_filters_mixed_batch": "int 1 8 1 8 4 4 4 u64 stream",
    "fdh_png_filter_deflate_ultrafast_mixed_batch": "int 1 8 1 8 1 8 4 4 4 4 u64 stream",
    "fdh_png_frame_mixed_batch": "int 1 8 4 4 4 4 4 4 4 u64 stream",
    "fdh_init": "int u64",
    "fdh_shutdown": "int",
    "fdh_multi_device_count": "int",
    "fdh_multi_uses_rccl": "int",
    "fdh_inflate_batch_multi": "int host u32 u32 u64",
}.items()}
EXPORTED_SYMBOLS = list(SIGNATURES)

# The prototypes of the extension headers, in the same notation (tests/test_abi_png16.py compares):
# include/fdeflate_hip_png16.h, the calls behind fdeflate_amd.png16.
EXTENSION_SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_png_expand16_batch": "int 1 8 1 8 4 4 4 4 u64 u32 u32 u32 stream",
    "fdh_png_expand16_mixed_batch": "int 1 8 1 8 4 4 4 4 4 u64 stream",
    "fdh_png_pack16_batch": "int 1 8 1 8 4 4 u64 u32 u32 stream",
}.items()}
# include/fdeflate_hip_png16_encode.h, the calls behind fdeflate_amd.png16_encode (tests/test_abi_png16_encode.py compares).
PNG16_ENCODE_SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_png_analyse16_mixed_batch": "int 1 8 4 4 4 4 4 4 4 u64 u32 stream",
    "fdh_png_encode16_plan_one": "u32 host host host u32 u32 u32 host",
    "fdh_png_encode16_plan_batch": "int 4 4 4 4 4 u32 8 8 8 8 4 u64 stream",
    "fdh_png_pack16_mixed_batch": "int 1 8 1 8 4 4 4 4 4 u64 stream",
}.items()}
# include/fdeflate_hip_levels.h, the calls behind fdeflate_amd.levels (tests/test_abi_levels.py compares).
LEVELS_SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_deflate_level_batch": "int 1 8 1 8 4 u64 u32 stream",
    "fdh_compress_to_vec_level": "int host size u32 host host",
    "fdh_debug_level_plan": "int u64 int u32 host",
}.items()}
# include/fdeflate_hip_png_levels.h, the calls behind fdeflate_amd.png_levels (tests/test_abi_png_levels.py compares).
PNG_LEVELS_SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_png_filter_mixed_batch": "int 1 8 1 8 1 8 4 4 u32 4 u64 stream",
    "fdh_png_level_bound": "u64 u64 u32",
    "fdh_png_level_file_bound": "u64 u64 u64 u32 u64",
}.items()}
# include/fdeflate_hip_pieces.h, the calls behind fdeflate_amd.pieces (tests/test_abi_pieces.py compares).
PIECES_SIGNATURES = {name: (sig.split()[0], tuple(sig.split()[1:])) for name, sig in {
    "fdh_deflate_level_pieces_batch": "int 1 8 1 1 8 4 4 u64 u32 stream",
    "fdh_deflate_stitch_batch": "int 1 8 4 4 8 8 1 8 4 u64 stream",
    "fdh_deflate_pieces_count": "u64 u64 u64",
    "fdh_deflate_pieces_bound": "u64 u64 u32 u64",
    "fdh_png_level_pieces_file_bound": "u64 u64 u64 u32 u64 u64",
}.items()}
# Every table by the header that declares its symbols, in the order the headers were added: signature() and lib() walk
# this (tests/test_abi.py holds it to include/).
TABLES = {"fdeflate_hip.h": SIGNATURES, "fdeflate_hip_png16.h": EXTENSION_SIGNATURES,
          "fdeflate_hip_png16_encode.h": PNG16_ENCODE_SIGNATURES, "fdeflate_hip_levels.h": LEVELS_SIGNATURES,
          "fdeflate_hip_png_levels.h": PNG_LEVELS_SIGNATURES, "fdeflate_hip_pieces.h": PIECES_SIGNATURES}


def signature(symbol):
    """(result, parameters) of a symbol of any table."""
    for table in TABLES.values():
        if symbol in table:
            return table[symbol]
    raise KeyError(symbol)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FdeflateHipError(
            "%s is missing: the HIP extension has not been built (make -C fdeflate_amd/csrc); "
            "fdeflate_amd has no CPU fallback" % SO_PATH)
    L = C.CDLL(SO_PATH)
    for table in TABLES.values():
        for name, (result, params) in table.items():
            fn = getattr(L, name)
            fn.restype = _CTYPES[result]
            fn.argtypes = [_CTYPES[p] for p in params]
    _lib = L
    return L


class Shard(C.Structure):
    """fdh_shard_t"""
    _fields_ = [("in_", C.c_void_p), ("in_off", C.c_void_p), ("out", C.c_void_p), ("out_off", C.c_void_p),
                ("out_len", C.c_void_p), ("status", C.c_void_p), ("adler", C.c_void_p), ("n", C.c_uint64),
                ("meta_all", C.c_void_p)]


def check(rc):
    if rc != 0:
        raise FdeflateHipError("fdeflate_hip error %d: %s" % (rc, lib().fdh_last_error().decode()))
