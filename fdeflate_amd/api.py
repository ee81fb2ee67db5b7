"""Host-side mirror of fdeflate's public API for the PNG path (reference src/lib.rs:29-36),
implemented over the C ABI (include/fdeflate_hip.h).  Same names, argument meaning and error
behaviour as the Rust crate:

    decompress_to_vec(input) -> bytes                  raises DecompressionError
    decompress_to_vec_bounded(input, maxlen) -> bytes  raises DecompressionError / OutputTooLarge
    compress_to_vec_ultra_fast(input) -> bytes

and the batched entry points the GPU exists for:

    inflate_batch(...), deflate_ultrafast_batch(...)   torch uint8/int64 tensors on the device

torch is used only as the owner of device memory and streams.
"""
import ctypes as C

from . import _lib

# what `import fdeflate_amd` offers (the package takes exactly these names); the rest of this module is reached as api.X
__all__ = [
    "Decompressor", "DecompressionError", "OutputTooLarge", "STATUS_NAMES", "FLAG_IGNORE_ADLER32",
    "FLAG_SERIAL_ONLY", "FLAG_GENERAL_ONLY", "FLAG_NO_RECHECK", "compress_to_vec_ultra_fast", "debug_build_tables", "decompress_to_vec",
    "decompress_to_vec_bounded", "deflate_ultrafast_batch", "inflate_batch", "inflate_batch_resumable", "ultrafast_bound",
    "compress_to_vec_stored", "deflate_stored_batch", "stored_size", "compress_to_vec", "compress_to_vec_rle",
    "compress_bound", "deflate_general_batch", "MODE_LEVEL1", "MODE_RLE", "MODE_LEVEL2", "MODE_LEVEL3",
    "compress_to_vec_with_level", "inflate_batch_multi", "init_devices",
    "shutdown_devices", "multi_uses_rccl", "png_unfilter_batch", "png_filter_batch", "inflate_png_batch", "png_filter_deflate_ultrafast_batch",
    "png_choose_filters_batch", "png_encode_ultrafast_batch",
    "crc32_batch", "png_file_bound", "png_geometry", "png_frame_batch", "png_encode_files_batch", "png_scan_files_batch",
    "png_info_fields", "png_gather_idat_batch", "png_decode_files_batch", "PNG_FILE_PREFIX", "PNG_FILE_SUFFIX",
    "PNG_FLAG_IGNORE_CRC", "PNG_SCAN_STATUS_NAMES", "PNG_OTHER_GEOMETRY", "PNG_COMP_SLOT_TOO_SMALL",
    "PNG_INDEX_OUTSIDE_PALETTE", "PNG_BAD_PLTE", "PNG_BAD_TRNS", "png_colour_batch", "png_expand_batch",
    "png_decode_files_rgba_batch", "PNG_FLAG_ADAM7", "png_adam7_size", "png_unfilter_interlaced_batch",
    "PNG_OK", "PNG_BAD_FILTER_TYPE", "PNG_BAD_SIZES", "PNG_SKIPPED", "PNG_SCAN_NO_SIGNATURE", "PNG_SCAN_TRUNCATED",
    "PNG_SCAN_BAD_IHDR", "PNG_SCAN_INTERLACED", "PNG_SCAN_CHUNK_STRUCTURE", "PNG_SCAN_CRC_MISMATCH",
    "PNG_TOO_MANY_COLOURS", "PNG_NOT_REPRESENTABLE", "PNG_SUMMARY_OPAQUE", "PNG_SUMMARY_GREY", "PNG_ANALYSE_HASH_MUL",
    "PNG_ANALYSE_HASH_BITS", "png_analyse_batch", "png_pack_batch", "png_palette_file_prefix", "png_frame_palette_batch",
    "png_encode_rgba_files_batch",
    "png_plan_sizes", "png_plan_batch", "png_gather_idat_mixed_batch", "png_colour_mixed_batch", "png_unfilter_mixed_batch",
    "png_expand_mixed_batch", "png_decode_mixed_files_batch", "png_decode_mixed_files_rgba_batch",
    "png_encode_plan_one", "png_encode_plan_batch", "png_analyse_mixed_batch", "png_pack_mixed_batch",
    "png_choose_filters_mixed_batch", "png_filter_deflate_ultrafast_mixed_batch", "png_frame_mixed_batch",
    "png_encode_records", "png_encode_mixed_rgba_files_batch",
]

STATUS_NAMES = [
    "Ok", "BadZlibHeader", "InsufficientInput", "InvalidBlockType",
    "InvalidUncompressedBlockLength", "InvalidHlit", "InvalidHdist", "InvalidCodeLengthRepeat",
    "BadCodeLengthHuffmanTree", "BadLiteralLengthHuffmanTree", "BadDistanceHuffmanTree",
    "InvalidLiteralLengthCode", "InvalidDistanceCode", "InputStartsWithRun", "DistanceTooFarBack",
    "WrongChecksum", "ExtraInput", "OutputTooLarge",
]
OUTPUT_TOO_LARGE = 17
FLAG_IGNORE_ADLER32 = 1
FLAG_SERIAL_ONLY = 2
FLAG_GENERAL_ONLY = 4
FLAG_NO_RECHECK = 8
FLAG_FORCE_LANES = 16
FLAG_NO_LANES = 32
FLAG_FIRST_ONLY = 64
FLAG_NO_SEGMENTS = 128
FLAG_SPANS = 256
FLAG_NO_FAST_GENERAL = 512
FLAG_NO_INTERVALS = 0x400   # tests / A-B: skip the interval kernel (inflate_seg2.h)
FLAG_INTERVALS_ONLY = 0x800  # debug: run only the interval kernel (what it leaves stays PENDING)
FLAG_NO_LANDING = 0x10000    # tests / A-B: skip the landing decoder (inflate_seg3.h)
FLAG_LANDING_ONLY = 0x20000  # debug: run only the landing decoder (what it leaves stays PENDING)
FLAG_NO_OVERLAP = 0x100000   # tests / A-B: the LZ-window kernel behind the canonical kernels, not beside them
FLAG_NO_LEAN_WRITE = 0x80000  # tests / A-B: the landing decoder always takes the interval decoder's general writing pass
FLAG_TAIL_LONG = 0x200000    # tests / A-B: behind the landing decoder always the five kernels of rounds 3-5
FLAG_TAIL_SHORT = 0x400000   # tests / A-B: behind the landing decoder always the exact kernel alone
FLAG_ORDER_ONCE = 0x800000   # tests / A-B: the streams without the ultra-fast prefix listed in one launch, in no order
FLAG_ORDER_TWICE = 0x1000000  # tests / A-B: ... in two, the long ones first


class DecompressionError(Exception):
    """Mirror of fdeflate::DecompressionError (src/decompress.rs:14-48); `.kind` is the variant."""

    def __init__(self, status):
        self.status = int(status)
        self.kind = STATUS_NAMES[self.status] if self.status < len(STATUS_NAMES) else "Unknown"
        super().__init__(self.kind)


class OutputTooLarge(Exception):
    """Mirror of BoundedDecompressionError::OutputTooLarge (src/decompress.rs:1097-1101)."""

    def __init__(self, partial_output):
        self.partial_output = partial_output
        super().__init__("OutputTooLarge")


class Decompressor:
    """Mirror of fdeflate::Decompressor (src/decompress.rs:96-342) over fdh_decompressor_*:

        d = Decompressor(); d.ignore_adler32()
        consumed, produced = d.read(input, output, output_position)   # raises DecompressionError
        d.is_done()

    `output` is a writable buffer (bytearray / numpy uint8 array); bytes are written at
    output[output_position : output_position + produced]."""

    def __init__(self):
        self._L = _lib.lib()
        self._d = self._L.fdh_decompressor_new()
        if not self._d:
            raise MemoryError("fdh_decompressor_new")

    def __del__(self):
        d, self._d = getattr(self, "_d", None), None
        if d:
            self._L.fdh_decompressor_free(d)

    def ignore_adler32(self):
        self._L.fdh_decompressor_ignore_adler32(self._d)

    def is_done(self):
        return bool(self._L.fdh_decompressor_is_done(self._d))

    def attempts(self):
        """Decode attempts made so far (introspection, fdh_decompressor_attempts)."""
        return int(self._L.fdh_decompressor_attempts(self._d))

    def decoded_bytes(self):
        """Output bytes decoded by all attempts together (introspection, fdh_decompressor_decoded_bytes)."""
        return int(self._L.fdh_decompressor_decoded_bytes(self._d))

    def device_bytes(self):
        """The most device memory the object's buffers have held together (introspection, fdh_decompressor_device_bytes)."""
        return int(self._L.fdh_decompressor_device_bytes(self._d))

    def read(self, data, output, output_position):
        """Decompressor::read (src/decompress.rs:179-337) -> (consumed, produced); raises DecompressionError.  What is
        not consumed (more than 192 KiB, or the room, waiting unread on the device) is to be offered again."""
        data = bytes(data)
        mv = memoryview(output)
        if mv.readonly or mv.itemsize != 1 or not mv.contiguous:
            raise ValueError("output must be a writable contiguous byte buffer")
        n = mv.nbytes
        obuf = (C.c_uint8 * n).from_buffer(mv) if n else None
        c, p, st = C.c_size_t(), C.c_size_t(), C.c_uint32()
        _lib.check(self._L.fdh_decompressor_read(self._d, data, len(data), obuf, n, output_position,
                                                 C.byref(c), C.byref(p), C.byref(st)))
        if st.value != 0:
            raise DecompressionError(st.value)
        return c.value, p.value


def _take(ptr, n):
    try:
        return C.string_at(ptr, n) if n else b""
    finally:
        _lib.lib().fdh_free(ptr)


def _compress(symbol, data, *level):
    """The one-shot compressors: fdh_compress_to_vec*(data, len, [level,] &out, &n) -> the stream as bytes."""
    fn = getattr(_lib.lib(), symbol)
    data = bytes(data)
    out, n = C.c_void_p(), C.c_size_t()
    _lib.check(fn(data, len(data), *level, C.byref(out), C.byref(n)))
    return _take(out, n.value)


def _decompress(symbol, data, *maxlen):
    """The one-shot decompressors: fdh_decompress_to_vec*(data, len, [maxlen,] &out, &n, &status) -> (bytes, status)."""
    fn = getattr(_lib.lib(), symbol)
    data = bytes(data)
    out, n, st = C.c_void_p(), C.c_size_t(), C.c_uint32()
    _lib.check(fn(data, len(data), *maxlen, C.byref(out), C.byref(n), C.byref(st)))
    return _take(out, n.value), st.value


def decompress_to_vec_bounded(data, maxlen):
    """fdeflate::decompress_to_vec_bounded (src/decompress.rs:1111)."""
    buf, status = _decompress("fdh_decompress_to_vec_bounded", data, maxlen)
    if status == 0:
        return buf
    if status == OUTPUT_TOO_LARGE:
        raise OutputTooLarge(buf)
    raise DecompressionError(status)


def decompress_to_vec(data):
    """fdeflate::decompress_to_vec (src/decompress.rs:1079)."""
    buf, status = _decompress("fdh_decompress_to_vec", data)
    if status != 0:
        raise DecompressionError(status)
    return buf


def compress_to_vec_ultra_fast(data):
    """fdeflate::compress_to_vec_ultra_fast (src/compress/mod.rs:313)."""
    return _compress("fdh_compress_to_vec_ultra_fast", data)


def ultrafast_bound(n):
    return int(_lib.lib().fdh_ultrafast_bound(int(n)))


def compress_to_vec_stored(data):
    """fdeflate::compress_to_vec_with_level(data, 0) (src/compress/mod.rs:299): stored blocks only."""
    return _compress("fdh_compress_to_vec_stored", data)


def compress_to_vec(data):
    """fdeflate::compress_to_vec (src/compress/mod.rs:294): level 1 in this snapshot."""
    return _compress("fdh_compress_to_vec", data)


def compress_to_vec_rle(data):
    """fdeflate::compress_to_vec_rle (src/compress/mod.rs:306)."""
    return _compress("fdh_compress_to_vec_rle", data)


LEVELS_PROVIDED = (0, 1, 2, 3)


def compress_to_vec_with_level(data, level):
    """fdeflate::compress_to_vec_with_level (src/compress/mod.rs:299): level 0 stored, levels 1-3 the
    greedy parser with the hash table (1) or the hash chains (2, 3).  Levels 4-9 (the lazy parser)
    are not provided: ValueError."""
    if isinstance(level, bool) or not isinstance(level, int) or level not in LEVELS_PROVIDED:
        raise ValueError("compression level %r is not provided (levels 0, 1, 2 and 3 are)" % (level,))
    return _compress("fdh_compress_to_vec_with_level", data, level)


def compress_bound(n):
    return int(_lib.lib().fdh_compress_bound(int(n)))


MODE_LEVEL1 = 1
MODE_RLE = 2
MODE_LEVEL2 = 3
MODE_LEVEL3 = 4


def deflate_general_batch(raw, in_off, out, out_off, mode, out_len=None):
    """Level-1 / -2 / -3 / RLE encode of n buffers (fdh_deflate_general_batch): a parser kernel (one stream
    per lane) that records the back-references, then a block-writer kernel (one stream per wavefront).
    Returns when the work has finished."""
    n = in_off.numel() - 1
    out_len = _i32(out_len, raw, n)
    _call("fdh_deflate_general_batch", raw, in_off, out, out_off, out_len, n, mode)
    return out_len


def stored_size(n):
    return int(_lib.lib().fdh_stored_size(int(n)))


# ------------------------------------------------------------------------------------------
# batched device entry points
# ------------------------------------------------------------------------------------------

_PROTOTYPES = {}   # symbol -> (function, (position, dtypes a tensor may have there) per device pointer, takes a stream)


def _prototype(symbol):
    """The entry of `symbol` in one of _lib.TABLES as _call wants it, worked out at a symbol's first call."""
    import torch
    ints = {1: (torch.uint8, torch.int8), 4: (torch.int32, getattr(torch, "uint32", None)),
            8: (torch.int64, getattr(torch, "uint64", None))}
    params = _lib.signature(symbol)[1]
    pointers = tuple((pos, ints[_lib.DEVICE_WIDTH[p]]) for pos, p in enumerate(params) if p in _lib.DEVICE_WIDTH)
    _PROTOTYPES[symbol] = (getattr(_lib.lib(), symbol), pointers, params[-1:] == ("stream",))
    return _PROTOTYPES[symbol]


def _call(symbol, *args):
    """What every batched entry point does with its C function: `args` are the prototype's parameters without the
    stream, tensors (or None) where its table entry (_lib.signature) has a device pointer.  Every tensor must be
    contiguous and live on ONE GPU; then each must have integer elements of the width the table records -- the kernel would read elements of
    another width wrongly, or past the tensor's end.  That GPU is made current for the duration of the call: the C ABI
    launches on the current device (hipGetDevice) and on the stream it is handed, so both must belong to the tensors'
    device even when another one is current.  The tensors go in as pointers, torch's current stream of their device goes
    last where the prototype takes one, and a result that is not 0 raises _lib.FdeflateHipError."""
    import torch
    fn, pointers, takes_stream = _PROTOTYPES.get(symbol) or _prototype(symbol)
    argv = list(args)
    dev = misfit = None
    for pos, dtypes in pointers:
        t = args[pos]
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("batched entry points take device tensors (HBM resident)")
        if not t.is_contiguous():
            raise ValueError("tensors must be contiguous")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("all tensors of one call must live on the same GPU (%s vs %s)" % (dev, t.device))
        if misfit is None and t.dtype not in dtypes:
            misfit = (pos, dtypes)     # (reported behind the checks above, of every tensor)
        argv[pos] = t.data_ptr()
    if dev is None:
        raise ValueError("no tensors")
    if misfit is not None:
        raise ValueError("%s: parameter %d takes a tensor of %s, not of %s"
                         % (symbol, misfit[0], " or ".join(str(d) for d in misfit[1] if d), args[misfit[0]].dtype))
    with torch.cuda.device(dev):
        if takes_stream:
            argv.append(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(fn(*argv))


def _i32(t, like, *shape):
    """The int32 output `t`, or a new one of `shape` on the device of `like` where the caller passed None."""
    import torch
    return t if t is not None else torch.empty(*shape, dtype=torch.int32, device=like.device)


def _first(a, b):
    """Per image the first status that is not 0: a where a != 0, else b."""
    import torch
    return torch.where(a != 0, a, b)


def inflate_batch(comp, in_off, out, out_off, out_len=None, status=None, adler=None, flags=0):
    """One-shot decode of n zlib streams (fdh_inflate_batch).  All tensors on the device:
    comp/out uint8, in_off/out_off int64 [n+1], out_len/status/adler int32 [n] (allocated when
    None).  Enqueued on torch's current stream; returns (out_len, status, adler)."""
    n = in_off.numel() - 1
    out_len, status, adler = _i32(out_len, comp, n), _i32(status, comp, n), _i32(adler, comp, n)
    _call("fdh_inflate_batch", comp, in_off, out, out_off, out_len, status, adler, n, flags)
    return out_len, status, adler


def inflate_batch_resumable(comp, in_off, out, out_off, resume, out_len=None, status=None, adler=None, flags=0, resume_in=False):
    """fdh_inflate_batch_resumable: as inflate_batch; `resume` (int32 [n, 4] on the device) receives, for every
    stream that ended InsufficientInput / OutputTooLarge, the place from which a later call can go on, and with
    resume_in says where each stream is taken up in this call (the slots then hold the output so far)."""
    import torch
    n = in_off.numel() - 1
    out_len, status, adler = _i32(out_len, comp, n), _i32(status, comp, n), _i32(adler, comp, n)
    assert resume.dtype == torch.int32 and resume.numel() == 4 * n and resume.is_contiguous()
    _call("fdh_inflate_batch_resumable", comp, in_off, out, out_off, out_len, status, adler, n,
          flags | (0x8000 if resume_in else 0), resume)
    return out_len, status, adler


def deflate_ultrafast_batch(raw, in_off, out, out_off, out_len=None):
    """Ultra-fast encode of n buffers (fdh_deflate_ultrafast_batch); returns out_len (int32)."""
    n = in_off.numel() - 1
    out_len = _i32(out_len, raw, n)
    _call("fdh_deflate_ultrafast_batch", raw, in_off, out, out_off, out_len, n)
    return out_len


def deflate_stored_batch(raw, in_off, out, out_off, out_len=None):
    """Level-0 (stored) encode of n buffers (fdh_deflate_stored_batch); returns out_len (int32)."""
    n = in_off.numel() - 1
    out_len = _i32(out_len, raw, n)
    _call("fdh_deflate_stored_batch", raw, in_off, out, out_off, out_len, n)
    return out_len


def png_unfilter_batch(filt, filt_off, pix, pix_off, row_bytes, bpp, png_status=None):
    """PNG scanline reconstruction of n images, one image per wavefront (fdh_png_unfilter_batch)."""
    n = filt_off.numel() - 1
    png_status = _i32(png_status, filt, n)
    _call("fdh_png_unfilter_batch", filt, filt_off, pix, pix_off, png_status, n, row_bytes, bpp)
    return png_status


def png_filter_batch(pix, pix_off, types, types_off, filt, filt_off, row_bytes, bpp, png_status=None):
    """PNG scanline filtering with the given per-row filter types (fdh_png_filter_batch)."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_filter_batch", pix, pix_off, types, types_off, filt, filt_off, png_status, n, row_bytes, bpp)
    return png_status


def png_filter_deflate_ultrafast_batch(pix, pix_off, types, types_off, out, out_off, row_bytes, bpp):
    """Filter n images with the given per-row types and ultra-fast-encode the filtered bytes in one
    kernel, no intermediate buffer (fdh_png_filter_deflate_ultrafast_batch) -> (out_len, png_status)."""
    n = pix_off.numel() - 1
    out_len, png_status = _i32(None, pix, n), _i32(None, pix, n)
    _call("fdh_png_filter_deflate_ultrafast_batch", pix, pix_off, types, types_off, out, out_off, out_len, png_status, n,
          row_bytes, bpp)
    return out_len, png_status


def png_choose_filters_batch(pix, pix_off, types, types_off, row_bytes, bpp, png_status=None):
    """One filter type per row, chosen from the pixels by the PNG specification's heuristic: the type
    whose filtered row has the smallest sum of absolute values, the lowest type number on equal sums
    (fdh_png_choose_filters_batch).  `types` (uint8) receives them at types_off (int64 [n+1], slots of
    exactly the row counts); returns png_status (0 ok, 2 sizes do not fit: nothing written)."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_choose_filters_batch", pix, pix_off, types, types_off, png_status, n, row_bytes, bpp)
    return png_status


def png_encode_ultrafast_batch(pix, pix_off, out, out_off, row_bytes, bpp, types=None, types_off=None):
    """Pixels in, IDAT payloads out: png_choose_filters_batch, then png_filter_deflate_ultrafast_batch with
    the chosen types, both enqueued on torch's current stream -> (out_len, png_status, types).
    Without `types` the buffer is allocated here and types_off is the running sum of the images' row
    counts, computed on the device (pix_off[0] and pix_off[n] are read back to size the buffer); with
    `types`, `types_off` must be given as well.  png_status[i] is the chooser's where that is not 0
    (the image is then not encoded from chosen types: disregard its slot), else the encoder's."""
    import torch
    n = pix_off.numel() - 1
    if row_bytes <= 0:
        raise ValueError("row_bytes must be positive")
    if (types is None) != (types_off is None):
        raise ValueError("types and types_off are given together or not at all")
    if types is None:
        types_off = torch.zeros(n + 1, dtype=torch.int64, device=pix.device)
        torch.cumsum((pix_off[1:] - pix_off[:-1]) // row_bytes, 0, out=types_off[1:])
        span = int(pix_off[n] - pix_off[0]) if n else 0
        types = torch.empty(max(1, span // row_bytes), dtype=torch.uint8, device=pix.device)
    chosen = png_choose_filters_batch(pix, pix_off, types, types_off, row_bytes, bpp)
    out_len, png_status = png_filter_deflate_ultrafast_batch(pix, pix_off, types, types_off, out, out_off, row_bytes, bpp)
    return out_len, _first(chosen, png_status), types


def inflate_png_batch(comp, in_off, filt, filt_off, pix, pix_off, row_bytes, bpp, flags=0):
    """Decode n IDAT-style zlib streams and reconstruct their scanlines in one call
    (fdh_inflate_png_batch) -> (out_len, status, adler, png_status)."""
    n = in_off.numel() - 1
    out_len, status, adler, png_status = (_i32(None, comp, n) for _ in range(4))
    _call("fdh_inflate_png_batch", comp, in_off, filt, filt_off, out_len, status, adler, pix, pix_off, png_status, n, flags,
          row_bytes, bpp)
    return out_len, status, adler, png_status


# ------------------------------------------------------------------------------------------
# PNG files: CRC-32, framing, container scan, IDAT gather
# ------------------------------------------------------------------------------------------

PNG_FILE_PREFIX = 41   # signature 8 + IHDR chunk 25 + the IDAT's length and type 8
PNG_FILE_SUFFIX = 16   # the IDAT's CRC 4 + IEND chunk 12
PNG_FLAG_IGNORE_CRC = 1
PNG_FLAG_ADAM7 = 2     # the scan accepts interlace method 1; the decode pipelines take such files to pixels
# The per-image status values, named as include/fdeflate_hip.h names them (FDH_PNG_STATUS_*).
# png_status of the row calls (reconstruction, filtering, selection, the fused encoder, framing, Adam7):
PNG_OK = 0
PNG_BAD_FILTER_TYPE = 1
PNG_BAD_SIZES = 2
PNG_SKIPPED = 3
# info.status of png_scan_files_batch; png_status 7 / 8 of png_gather_idat_batch
PNG_SCAN_NO_SIGNATURE = 1
PNG_SCAN_TRUNCATED = 2
PNG_SCAN_BAD_IHDR = 3
PNG_SCAN_INTERLACED = 4
PNG_SCAN_CHUNK_STRUCTURE = 5
PNG_SCAN_CRC_MISMATCH = 6
PNG_SCAN_STATUS_NAMES = ["Ok", "NoSignature", "Truncated", "BadIhdr", "Interlaced", "ChunkStructure", "CrcMismatch"]
PNG_OTHER_GEOMETRY = 7
PNG_COMP_SLOT_TOO_SMALL = 8
# png_status 9 of png_expand_batch, 10 / 11 of png_colour_batch
PNG_INDEX_OUTSIDE_PALETTE = 9
PNG_BAD_PLTE = 10
PNG_BAD_TRNS = 11
# png_status 12 of png_analyse_batch, 13 of png_pack_batch
PNG_TOO_MANY_COLOURS = 12
PNG_NOT_REPRESENTABLE = 13
# summary of png_analyse_batch: bit 0 every A is 255, bit 1 every pixel is grey, bits 8 .. 15 the sample depth that suffices
PNG_SUMMARY_OPAQUE = 1
PNG_SUMMARY_GREY = 2
# The analysis kernel's LDS table (csrc/png_pack.hip: kColourHashMul, kAnalyseSlotBits): the pixel word w = R | G << 8 |
# B << 16 | A << 24 starts probing at slot ((w * MUL) mod 2^32) >> (32 - BITS).  Named here for tests that build collisions.
PNG_ANALYSE_HASH_MUL = 0x9E3779B1
PNG_ANALYSE_HASH_BITS = 11
# fdh_png_info as eight int32 words: status, width, height, depth | colour << 8 | interlace << 16, idat_bytes,
# idat_chunks, first_idat, chunks
PNG_INFO_WORDS = 8
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_PNG_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


def png_file_bound(rows, row_bytes):
    """A file slot that always suffices for png_encode_files_batch: ultrafast_bound(rows * (row_bytes + 1)) + 57."""
    return int(_lib.lib().fdh_png_file_bound(int(rows), int(row_bytes)))


def png_geometry(width, bit_depth, colour_type):
    """(row_bytes, bpp) of the packed scanlines of a PNG image: row_bytes = ceil(width * channels * depth / 8),
    bpp = max(1, channels * depth / 8) -- always one of 1, 2, 3, 4, 6, 8.  ValueError for a pair that is not one of
    the specification's fifteen."""
    if colour_type not in _PNG_DEPTHS or bit_depth not in _PNG_DEPTHS[colour_type]:
        raise ValueError("bit depth %r / colour type %r is not one of the PNG specification's fifteen pairs" % (bit_depth, colour_type))
    if not 0 < width < (1 << 31):
        raise ValueError("width must be 1 .. 2^31-1")
    bits = _PNG_CHANNELS[colour_type] * bit_depth
    return (width * bits + 7) // 8, max(1, bits // 8)


def crc32_batch(data, off, length=None, seed=None, crc=None, status=None):
    """CRC-32 (PNG / zlib) of n ranges of `data` (fdh_crc32_batch): range i starts at off[i] (int64 [n+1]) and is
    length[i] bytes long (int32, e.g. an encoder's out_len), or the whole slot without `length`; seed[i] (int32) is the
    CRC of what came before.  -> (crc, status), int32 [n] (bit patterns of the unsigned values); status 2 and crc 0
    where length[i] exceeds the slot or is 0xFFFFFFFF.  Enqueued on torch's current stream."""
    n = off.numel() - 1
    crc, status = _i32(crc, data, n), _i32(status, data, n)
    _call("fdh_crc32_batch", data, off, length, seed, crc, status, n)
    return crc, status


def _enc_off(file_off, prefix):
    """The ONE offsets array the fused encoders are given for file slots: enc_off[i] = file_off[i] + prefix, an int or a
    tensor of one prefix per image, and the last slot ends PNG_FILE_SUFFIX bytes in front of its file slot's end, though
    not in front of its own start: enc_off[n] = max(file_off[n] - 16, enc_off[n - 1]).  n is at least 1."""
    import torch
    n = file_off.numel() - 1
    enc_off = torch.empty_like(file_off)
    torch.add(file_off[:n], prefix, out=enc_off[:n])
    enc_off[n] = torch.maximum(file_off[n] - PNG_FILE_SUFFIX, enc_off[n - 1])
    return enc_off


def png_frame_batch(file, file_off, idat_len, height, width, bit_depth, colour_type, file_len=None, png_status=None):
    """Signature, IHDR and the IDAT's head in front of the zlib streams that lie PNG_FILE_PREFIX bytes into their file
    slots, the IDAT's CRC and IEND behind them (fdh_png_frame_batch) -> (file_len, png_status)."""
    n = file_off.numel() - 1
    file_len, png_status = _i32(file_len, file, n), _i32(png_status, file, n)
    _call("fdh_png_frame_batch", file, file_off, idat_len, height, file_len, png_status, n, width, bit_depth, colour_type)
    return file_len, png_status


def png_encode_files_batch(pix, pix_off, file, file_off, width, bit_depth, colour_type):
    """Pixels in, PNG files out, on torch's current stream and without a round trip: the rows' filter types chosen
    (png_choose_filters_batch), filtering + ultra-fast encode to file_off + 41 (png_filter_deflate_ultrafast_batch), the
    framing around the streams (png_frame_batch).  Image i is pix[pix_off[i] .. pix_off[i+1]), whole packed scanlines of
    the given geometry; its file goes to the slot file[file_off[i] .. file_off[i+1]) -- png_file_bound(rows, row_bytes)
    always suffices.  -> (file_len, png_status, types) -- `types` holds the chosen filter types, one per row, the
    images' back to back --; png_status[i] is the encoder's where that is not 0, else the
    framing's (2: the file does not fit its slot -- file_len[i] = 0).
    The encoders take ONE offsets array, so the encoder's slot for image i reaches 41 bytes into slot i + 1 (the last one
    ends 16 bytes in front of its slot's end): the bytes that image i + 1's own prefix is written to afterwards.  A stream
    that does not fit its file slot can therefore leave bytes in the first 41 of the next slot; they stay there only if
    that next image fails as well."""
    import torch
    row_bytes, bpp = png_geometry(width, bit_depth, colour_type)
    n = pix_off.numel() - 1
    dev = pix.device
    if n == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return e, e.clone(), torch.empty(0, dtype=torch.uint8, device=dev)
    height = ((pix_off[1:] - pix_off[:-1]) // row_bytes).clamp(max=0xFFFFFFFF).to(torch.int32)   # (bit pattern of the u32)
    enc_off = _enc_off(file_off, PNG_FILE_PREFIX)
    # one type per row; the buffer is sized by what `pix` could hold at most, so nothing is read back
    types_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum((pix_off[1:] - pix_off[:-1]) // row_bytes, 0, out=types_off[1:])
    types = torch.empty(max(1, pix.numel() // row_bytes), dtype=torch.uint8, device=dev)
    idat_len, enc_status, types = png_encode_ultrafast_batch(pix, pix_off, file, enc_off, row_bytes, bpp, types=types,
                                                             types_off=types_off)
    file_len, png_status = png_frame_batch(file, file_off, idat_len, height, width, bit_depth, colour_type)
    return file_len, _first(enc_status, png_status), types


def png_scan_files_batch(file, file_off, file_len=None, info=None, flags=0):
    """Walks the chunks of n PNG files and verifies every chunk's CRC (fdh_png_scan_files_batch) -> info, int32
    [n, PNG_INFO_WORDS] on the device (png_info_fields names the columns of a host copy); info[:, 0] is the status."""
    import torch
    n = file_off.numel() - 1
    info = _i32(info, file, n, PNG_INFO_WORDS)
    assert info.dtype == torch.int32 and info.numel() == PNG_INFO_WORDS * n
    _call("fdh_png_scan_files_batch", file, file_off, file_len, info, n, flags)
    return info


def png_info_fields(info):
    """A host copy of `info` as a dict of int64 numpy arrays named like the fields of fdh_png_info."""
    w = info.detach().cpu().numpy().reshape(-1, PNG_INFO_WORDS).view("uint32").astype("int64")
    return {"status": w[:, 0], "width": w[:, 1], "height": w[:, 2], "bit_depth": w[:, 3] & 0xFF,
            "colour_type": (w[:, 3] >> 8) & 0xFF, "interlace": (w[:, 3] >> 16) & 0xFF, "idat_bytes": w[:, 4],
            "idat_chunks": w[:, 5], "first_idat": w[:, 6], "chunks": w[:, 7]}


def png_gather_idat_batch(file, file_off, info, comp, comp_off, width, bit_depth, colour_type, comp_len=None, png_status=None):
    """The IDAT bodies of every file one behind the other at comp_off (fdh_png_gather_idat_batch) -> (comp_len,
    png_status): 0 ok, 3 info says the file is not sound, 7 another geometry than the call's, 8 comp slot too small."""
    n = file_off.numel() - 1
    comp_len, png_status = _i32(comp_len, file, n), _i32(png_status, file, n)
    _call("fdh_png_gather_idat_batch", file, file_off, info, comp, comp_off, comp_len, png_status, n, width, bit_depth,
          colour_type)
    return comp_len, png_status


# Adam7 (PNG specification 8.2): first column and row of pass p = 0 .. 6, column and row steps
_ADAM7_X0, _ADAM7_Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
_ADAM7_DX, _ADAM7_DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)


def png_adam7_size(width, height, bit_depth, colour_type):
    """The number of bytes the IDAT stream of an Adam7-interlaced width x height image decodes to
    (fdh_png_adam7_size's arithmetic, on the host, no device call): over the seven passes, ph * (1 + ceil(pw * bits / 8))
    with pw = ceil((width - x0) / dx), ph = ceil((height - y0) / dy), nothing for a pass with pw = 0 or ph = 0.  0 for
    an illegal depth / colour pair or a zero dimension.  `height` may be a numpy array (-> int64 array)."""
    import numpy as np
    h = np.asarray(height, dtype=np.int64)
    total = np.zeros_like(h)
    if colour_type in _PNG_DEPTHS and bit_depth in _PNG_DEPTHS[colour_type] and width > 0:
        bits = _PNG_CHANNELS[colour_type] * bit_depth
        for x0, y0, dx, dy in zip(_ADAM7_X0, _ADAM7_Y0, _ADAM7_DX, _ADAM7_DY):
            pw = max(0, (width - x0 + dx - 1) // dx)
            ph = np.maximum(0, (h - y0 + dy - 1) // dy)
            if pw:
                total = total + ph * (1 + (pw * bits + 7) // 8)
        total = np.where(h > 0, total, 0)
    return total if total.ndim else int(total)


def png_unfilter_interlaced_batch(filt, filt_off, pix, pix_off, width, bit_depth, colour_type, method=None, upstream=None,
                                  upstream_len=None, png_status=None):
    """Decoded IDAT streams to packed scanlines, Adam7-interlaced images and progressive ones in one batch
    (fdh_png_unfilter_interlaced_batch): image i, filt[filt_off[i] .. filt_off[i+1]) -- png_adam7_size(...) bytes, or
    height * (row_bytes + 1) where method[i] is 0 --, goes to pix[pix_off[i] .. pix_off[i+1]), height_i rows of row_bytes
    as png_unfilter_batch leaves them.  method: uint8 [n], 0 progressive, 1 Adam7 (None: all Adam7); upstream /
    upstream_len: the decoder's status and out_len (int32 [n]).  `filt` is reconstructed in place: its contents
    afterwards are not specified.  -> png_status: 0 ok, 1 a filter type above 4, 2 sizes do not fit, 3 upstream != 0."""
    import torch
    n = filt_off.numel() - 1
    png_status = _i32(png_status, filt, n)
    assert method is None or (method.dtype == torch.uint8 and method.numel() == n and method.is_contiguous())
    _call("fdh_png_unfilter_interlaced_batch", filt, filt_off, pix, pix_off, method, upstream, upstream_len, png_status, n,
          width, bit_depth, colour_type)
    return png_status


def _png_uniform_steps(file, file_off, info, comp, comp_off, filt, filt_off, pix, pix_off, geometry, rgba, png_status=None,
                       adam7=False):
    """The decode steps of a batch of ONE geometry = (width, bit_depth, colour_type), behind the scan and the allocation:
    png_gather_idat_batch, with `rgba` png_colour_batch, then inflate_png_batch -- or, with `adam7`, inflate_batch and
    png_unfilter_interlaced_batch.  png_status: what an earlier step (the plan) found, or None.
    -> (status, png_status, pal, colour); png_status is the first that is not 0 in that order."""
    import torch
    row_bytes, bpp = png_geometry(*geometry)
    _, gathered = png_gather_idat_batch(file, file_off, info, comp, comp_off, *geometry)
    png_status = gathered if png_status is None else _first(png_status, gathered)
    pal = colour = None
    if rgba:
        pal, colour, coloured = png_colour_batch(file, file_off, info, *geometry)
        png_status = _first(png_status, coloured)
    if adam7:
        method = info.view(torch.uint8).view(-1, 4 * PNG_INFO_WORDS)[:, 14].contiguous()    # info.interlace, on the device
        out_len, status, _ = inflate_batch(comp, comp_off, filt, filt_off, flags=0)
        unfiltered = png_unfilter_interlaced_batch(filt, filt_off, pix, pix_off, *geometry, method=method, upstream=status,
                                                   upstream_len=out_len)
    else:
        _, status, _, unfiltered = inflate_png_batch(comp, comp_off, filt, filt_off, pix, pix_off, row_bytes, bpp, flags=0)
    return status, _first(png_status, unfiltered), pal, colour


def _png_pixels_to_rgba(decoded, sample_bytes=1, expand=None, expand_mixed=None):
    """The end of the RGBA pipelines; `decoded` is what _png_files_to_pixels or _png_mixed_files_to_pixels returns.  The
    RGBA buffer, then png_expand_batch at the batch's one geometry or png_expand_mixed_batch where there is none, with
    everything found so far as upstream.  sample_bytes 2 (fdeflate_amd.png16): the RGBA8 offsets and total doubled, the
    offsets on the device, and `expand` / `expand_mixed` in the two calls' places.
    -> (rgba, rgba_off, info, status, png_status)."""
    import torch
    pix, pix_off, info, status, png_status, rgba_off, pal, colour, _, total, geometry = decoded
    if sample_bytes != 1:
        rgba_off, total = rgba_off * sample_bytes, total * sample_bytes
    rgba = torch.empty(max(1, total), dtype=torch.uint8, device=pix.device)
    if pix_off.numel() > 1:
        upstream = _first(png_status, status)   # (a zlib status reaches expand as "not 0")
        if geometry is not None:
            expanded = (expand or png_expand_batch)(pix, pix_off, rgba, rgba_off, *geometry, pal=pal, colour=colour, upstream=upstream)
        else:
            expanded = (expand_mixed or png_expand_mixed_batch)(pix, pix_off, rgba, rgba_off, info, pal=pal, colour=colour,
                                                                upstream=upstream)
        png_status = _first(png_status, expanded)
    return rgba[:total], rgba_off, info, status, png_status


def _png_files_to_pixels(file, file_off, width, bit_depth, colour_type, file_len, flags, rgba):
    """What png_decode_files_batch and png_decode_files_rgba_batch share: the scan, the ONE read-back of `info` that sizes
    every buffer (with `rgba` the RGBA slots as well), gather, with `rgba` png_colour_batch, then inflate_png_batch -- or,
    with PNG_FLAG_ADAM7 and at least one good interlaced file in the batch, inflate_batch and
    png_unfilter_interlaced_batch.
    -> (pix, pix_off, info, status, png_status, rgba_off, pal, colour, total pixel bytes, total RGBA bytes, the call's
    geometry); png_status is the first that is not 0 in that order."""
    import numpy as np
    import torch
    row_bytes, _ = png_geometry(width, bit_depth, colour_type)
    n = file_off.numel() - 1
    dev = file.device
    info = png_scan_files_batch(file, file_off, file_len, flags=flags)
    f = png_info_fields(info)                                   # the one read-back
    good = (f["status"] == 0) & (f["width"] == width) & (f["bit_depth"] == bit_depth) & (f["colour_type"] == colour_type)
    sizes = np.zeros((4, n + 1), dtype=np.int64)
    sizes[0, 1:] = np.where(good, f["idat_bytes"], 0)
    sizes[1, 1:] = np.where(good, f["height"] * (row_bytes + 1), 0)
    adam7 = good & (f["interlace"] == 1)        # (only the scan with PNG_FLAG_ADAM7 leaves such a file at status 0)
    if adam7.any():
        sizes[1, 1:] = np.where(adam7, png_adam7_size(width, f["height"], bit_depth, colour_type), sizes[1, 1:])
    sizes[2, 1:] = np.where(good, f["height"] * row_bytes, 0)
    if rgba:
        sizes[3, 1:] = np.where(good, f["height"] * (width * 4), 0)
    offs = torch.from_numpy(np.cumsum(sizes, axis=1)).to(dev)
    comp_off, filt_off, pix_off = offs[0], offs[1], offs[2]
    total = offs[:, n].tolist() if n else [0, 0, 0, 0]
    comp = torch.empty(max(1, total[0]), dtype=torch.uint8, device=dev)
    filt = torch.empty(max(1, total[1]), dtype=torch.uint8, device=dev)
    pix = torch.empty(max(1, total[2]), dtype=torch.uint8, device=dev)
    geometry = (width, bit_depth, colour_type)
    status, png_status, pal, colour = _png_uniform_steps(file, file_off, info, comp, comp_off, filt, filt_off, pix, pix_off, geometry,
                                                         rgba, adam7=adam7.any())
    return pix, pix_off, info, status, png_status, offs[3], pal, colour, total[2], total[3], geometry


def png_decode_files_batch(file, file_off, width, bit_depth, colour_type, file_len=None, flags=0):
    """PNG files in, packed scanlines out: png_scan_files_batch, ONE read-back of `info` to size the buffers (exact
    comp / filtered / pixel slots; empty ones for files that are not sound or not of the call's geometry),
    png_gather_idat_batch, inflate_png_batch.  `flags`: PNG_FLAG_IGNORE_CRC, PNG_FLAG_ADAM7 -- with the latter
    Adam7-interlaced files are decoded too (a batch that holds one goes through inflate_batch and
    png_unfilter_interlaced_batch; one that holds none takes the same calls as without the flag); without it such a
    file is info.status 4 / png_status 3 with empty slots.
    -> (pix, pix_off, info, status, png_status): pix uint8 with image i at pix_off[i] .. pix_off[i+1] (height_i rows of
    row_bytes, the PNG's own packed samples: palette indices, bit-packed and big-endian samples as they are, no tRNS --
    png_decode_files_rgba_batch goes on to [H, W, 4] uint8 pictures; neither applies gamma); info as png_scan_files_batch;
    status the zlib decoder's (of an empty stream for a file that was skipped); png_status the gather's where that is not
    0 (3, 7), else inflate_png_batch's."""
    pix, pix_off, info, status, png_status, _, _, _, total, _, _ = _png_files_to_pixels(file, file_off, width, bit_depth, colour_type,
                                                                                       file_len, flags, False)
    return pix[:total], pix_off, info, status, png_status


def png_colour_batch(file, file_off, info, width, bit_depth, colour_type, pal=None, colour=None, png_status=None):
    """PLTE and tRNS of n scanned files (fdh_png_colour_batch) -> (pal, colour, png_status): pal int32 [n, 256], the
    words R | G << 8 | B << 16 | A << 24 (None unless colour_type is 3), colour int32 [n, 4] (PLTE entry count, bit 0 =
    a colour key is present, key R or grey | G << 16, key B); png_status 0 ok, 3 / 7 as the gather's,
    PNG_BAD_PLTE (10), PNG_BAD_TRNS (11)."""
    n = file_off.numel() - 1
    if colour_type == 3:
        pal = _i32(pal, file, n, 256)
    colour, png_status = _i32(colour, file, n, 4), _i32(png_status, file, n)
    _call("fdh_png_colour_batch", file, file_off, info, pal, colour, png_status, n, width, bit_depth, colour_type)
    return pal, colour, png_status


def png_expand_batch(pix, pix_off, rgba, rgba_off, width, bit_depth, colour_type, pal=None, colour=None, upstream=None,
                     png_status=None):
    """Packed scanlines to RGBA8 (fdh_png_expand_batch): image i, whole rows at pix_off[i] .. pix_off[i+1], goes to the
    slot rgba[rgba_off[i] .. rgba_off[i+1]) of exactly rows * width * 4 bytes.  pal / colour as png_colour_batch writes
    them (pal is needed for colour type 3; without colour there is no key and every palette index counts as inside);
    upstream (int32 [n]): where not 0 the image is skipped and its png_status is that value.  -> png_status: 0 ok, 2 the
    slots do not fit (nothing written), PNG_INDEX_OUTSIDE_PALETTE (9: such pixels are (0, 0, 0, 255))."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_expand_batch", pix, pix_off, rgba, rgba_off, pal, colour, upstream, png_status, n, width, bit_depth,
          colour_type)
    return png_status


def png_decode_files_rgba_batch(file, file_off, width, bit_depth, colour_type, file_len=None, flags=0):
    """PNG files in, RGBA8 pictures out, on torch's current stream: png_decode_files_batch's steps (the same single
    read-back, which also sizes the RGBA slots: height * width * 4 bytes, empty for files that are skipped) with
    png_colour_batch behind the gather and png_expand_batch at the end; `flags` as there (PNG_FLAG_ADAM7 included).
    -> (rgba, rgba_off, info, status, png_status):
    rgba[rgba_off[i]:rgba_off[i+1]].view(h, width, 4) is picture i -- samples scaled to eight bits, palette and tRNS
    applied (PNG specification; no gamma) --; info and status as png_decode_files_batch; png_status the first that is
    not 0 of gather, colour, inflate_png_batch and expand (3, 7; 10, 11; 1 .. 3; 9)."""
    return _png_pixels_to_rgba(_png_files_to_pixels(file, file_off, width, bit_depth, colour_type, file_len, flags, True))


# ------------------------------------------------------------------------------------------
# PNG decode: mixed batches (every image's geometry from its own scan record)
# ------------------------------------------------------------------------------------------

class _PngInfoRecord(C.Structure):
    """fdh_png_info"""
    _fields_ = [("status", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8),
                ("colour_type", C.c_uint8), ("interlace", C.c_uint8), ("pad", C.c_uint8), ("idat_bytes", C.c_uint32),
                ("idat_chunks", C.c_uint32), ("first_idat", C.c_uint32), ("chunks", C.c_uint32)]


def png_plan_sizes(record, max_bytes=0):
    """What a pipeline has to allocate for one image (fdh_png_plan_sizes: host arithmetic, no device call).  `record`:
    a mapping with the fields of fdh_png_info that matter here (status, width, height, bit_depth, colour_type,
    interlace, idat_bytes; a field that is missing counts as 0).  -> (status, compressed, filtered, packed, rgba):
    status 0 ok, 3 the record is not decodable, 2 the filtered size is 2^32 or more or the largest size exceeds a
    max_bytes that is not 0; the sizes are all 0 unless the status is."""
    rec = _PngInfoRecord(**{k: int(record.get(k, 0)) for k, _ in _PngInfoRecord._fields_})
    sizes = (C.c_uint64 * 4)()
    st = _lib.lib().fdh_png_plan_sizes(C.byref(rec), int(max_bytes), sizes)
    return (int(st),) + tuple(int(v) for v in sizes)


def _wanted(like, n, *wants):
    """The size outputs of the plan calls: True -> a new int64 [n] on the device of `like`, False -> None, a tensor or None
    -> itself."""
    import torch
    return [torch.empty(n, dtype=torch.int64, device=like.device) if w is True else None if w is False else w for w in wants]


def png_plan_batch(info, max_bytes=0, comp_size=True, filt_size=True, pix_size=True, rgba_size=True, png_status=None):
    """png_plan_sizes for n scan records on the device (fdh_png_plan_batch).  Each of the four outputs is True
    (allocated), a tensor (int64 [n]) or None / False (not wanted).
    -> (comp_size, filt_size, pix_size, rgba_size, png_status), None for an output that was not wanted."""
    n = info.numel() // PNG_INFO_WORDS
    outs = _wanted(info, n, comp_size, filt_size, pix_size, rgba_size)
    png_status = _i32(png_status, info, n)
    _call("fdh_png_plan_batch", info, int(max_bytes), *outs, png_status, n)
    return (*outs, png_status)


def png_gather_idat_mixed_batch(file, file_off, info, comp, comp_off, upstream=None, comp_len=None, png_status=None):
    """png_gather_idat_batch for files of any geometry (fdh_png_gather_idat_mixed_batch) -> (comp_len, png_status):
    0 ok, 3 the record is not decodable (or does not describe the file), 8 comp slot too small, or upstream[i] where
    that is not 0."""
    n = file_off.numel() - 1
    comp_len, png_status = _i32(comp_len, file, n), _i32(png_status, file, n)
    _call("fdh_png_gather_idat_mixed_batch", file, file_off, info, upstream, comp, comp_off, comp_len, png_status, n)
    return comp_len, png_status


def png_colour_mixed_batch(file, file_off, info, upstream=None, pal=None, colour=None, png_status=None):
    """png_colour_batch with every file's own depth and colour type (fdh_png_colour_mixed_batch) -> (pal, colour,
    png_status): pal int32 [n, 256] -- row i is written only if file i has colour type 3 --, colour int32 [n, 4];
    png_status 0, 3, 10, 11, or upstream[i] where that is not 0."""
    n = file_off.numel() - 1
    pal, colour, png_status = _i32(pal, file, n, 256), _i32(colour, file, n, 4), _i32(png_status, file, n)
    _call("fdh_png_colour_mixed_batch", file, file_off, info, upstream, pal, colour, png_status, n)
    return pal, colour, png_status


def png_unfilter_mixed_batch(filt, filt_off, pix, pix_off, info, upstream=None, upstream_len=None, png_status=None):
    """png_unfilter_interlaced_batch at every image's own geometry and interlace method (fdh_png_unfilter_mixed_batch):
    the slots must be exactly the plan's filtered and packed sizes.  `filt` is reconstructed in place.
    -> png_status: 0 ok, 1 a filter type above 4, 2 sizes do not fit, 3 not decodable or upstream[i] != 0."""
    n = filt_off.numel() - 1
    png_status = _i32(png_status, filt, n)
    _call("fdh_png_unfilter_mixed_batch", filt, filt_off, pix, pix_off, info, upstream, upstream_len, png_status, n)
    return png_status


def png_expand_mixed_batch(pix, pix_off, rgba, rgba_off, info, pal=None, colour=None, upstream=None, png_status=None):
    """png_expand_batch at every image's own geometry (fdh_png_expand_mixed_batch).  pal / colour as
    png_colour_mixed_batch writes them; an image of colour type 3 without `pal` is status 10.
    -> png_status: 0 ok, 2 the slots do not fit, 3 not decodable, 9 an index outside the palette, or upstream[i]."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_expand_mixed_batch", pix, pix_off, rgba, rgba_off, info, pal, colour, upstream, png_status, n)
    return png_status


def _read_back(t):
    """The one place where the mixed pipeline moves anything from the device to the host (tests count the bytes)."""
    return t.tolist()


def _png_mixed_files_to_pixels(file, file_off, file_len, flags, max_bytes, route, rgba, sample_bytes=1):
    """What png_decode_mixed_files_batch and png_decode_mixed_files_rgba_batch share: scan, plan, the four cumulative
    sums on the device, ONE read-back of six 64-bit words (the four totals, and the smallest and largest of the keys
    width | depth << 32 | colour << 40 | interlace << 48 over the images the plan accepts), then gather, colour,
    inflate and reconstruction.  A batch whose keys are all the same and not interlaced takes the calls of
    png_decode_files_batch with that geometry, any other the mixed calls; `route` forces one.  sample_bytes 2
    (fdeflate_amd.png16) with max_bytes: a file whose RGBA16 picture exceeds max_bytes is refused like one the plan
    refuses (status 2, empty slots), on the device and in front of the sums.
    -> (pix, pix_off, info, status, png_status, rgba_off, pal, colour, total pixel bytes, total RGBA bytes, geometry of
    the uniform route or None)."""
    import torch
    if route not in (None, "mixed", "uniform"):
        raise ValueError("route must be None, 'mixed' or 'uniform'")
    n = file_off.numel() - 1
    dev = file.device
    info = png_scan_files_batch(file, file_off, file_len, flags=flags)
    comp_size, filt_size, pix_size, rgba_size, png_status = png_plan_batch(info, max_bytes)
    if sample_bytes != 1 and max_bytes:
        # the plan's limit held against the picture the caller gets (rgba_size stays the RGBA8 size: the caller scales it)
        over = (png_status == 0) & (rgba_size * sample_bytes > max_bytes)
        comp_size, filt_size, pix_size, rgba_size = (torch.where(over, 0, s) for s in (comp_size, filt_size, pix_size, rgba_size))
        png_status = torch.where(over, PNG_BAD_SIZES, png_status)
    offs = torch.zeros((4, n + 1), dtype=torch.int64, device=dev)
    torch.cumsum(torch.stack((comp_size, filt_size, pix_size, rgba_size)), 1, out=offs[:, 1:])
    words = info.view(-1, PNG_INFO_WORDS).to(torch.int64)
    key = (words[:, 1] & 0xFFFFFFFF) | ((words[:, 3] & 0xFFFFFF) << 32)
    planned = png_status == 0
    none_lo, none_hi = torch.full((1,), 1 << 62, dtype=torch.int64, device=dev), torch.full((1,), -1, dtype=torch.int64, device=dev)
    key_lo = torch.where(planned, key, none_lo).amin(0, keepdim=True) if n else none_lo
    key_hi = torch.where(planned, key, none_hi).amax(0, keepdim=True) if n else none_hi
    summary = torch.cat((offs[:, n], key_lo, key_hi))
    total_comp, total_filt, total_pix, total_rgba, key_min, key_max = _read_back(summary)   # the one read-back: 48 bytes
    uniform = key_min == key_max and (key_min >> 48) == 0
    if route == "uniform" and not uniform and key_min <= key_max:
        raise ValueError("route='uniform' on a batch whose files differ in geometry (or are interlaced)")
    uniform = uniform and route != "mixed"
    comp_off, filt_off, pix_off = offs[0], offs[1], offs[2]
    comp = torch.empty(max(1, total_comp), dtype=torch.uint8, device=dev)
    filt = torch.empty(max(1, total_filt), dtype=torch.uint8, device=dev)
    pix = torch.empty(max(1, total_pix), dtype=torch.uint8, device=dev)
    pal = colour = geometry = None
    if uniform:
        geometry = (key_min & 0xFFFFFFFF, (key_min >> 32) & 0xFF, (key_min >> 40) & 0xFF)
        status, png_status, pal, colour = _png_uniform_steps(file, file_off, info, comp, comp_off, filt, filt_off, pix, pix_off,
                                                             geometry, rgba, png_status=png_status)
    else:
        _, png_status = png_gather_idat_mixed_batch(file, file_off, info, comp, comp_off, upstream=png_status)
        if rgba:
            pal, colour, png_status = png_colour_mixed_batch(file, file_off, info, upstream=png_status)
        out_len, status, _ = inflate_batch(comp, comp_off, filt, filt_off, flags=0)
        unfiltered = png_unfilter_mixed_batch(filt, filt_off, pix, pix_off, info, upstream=_first(png_status, status), upstream_len=out_len)
        png_status = _first(png_status, unfiltered)
    return pix, pix_off, info, status, png_status, offs[3], pal, colour, total_pix, total_rgba, geometry


def png_decode_mixed_files_batch(file, file_off, file_len=None, flags=0, max_bytes=0, route=None):
    """PNG files of any width, height, depth, colour type and interlace method in, packed scanlines out, on torch's
    current stream: png_scan_files_batch, png_plan_batch, the buffers sized on the device with ONE read-back of 48
    bytes (not of `info`), png_gather_idat_mixed_batch, inflate_batch, png_unfilter_mixed_batch.  `flags` as
    png_decode_files_batch (without PNG_FLAG_ADAM7 an interlaced file is info.status 4 and png_status 3); max_bytes:
    a file one of whose buffers would be larger is png_status 2 with empty slots, before anything is allocated (0: no
    limit but the decoder's 2^32 - 1 bytes per stream).  A batch whose sound files all have one geometry and are not
    interlaced takes png_decode_files_batch's calls instead (the fused inflate_png_batch) and loses nothing;
    route="mixed" / "uniform" forces one of the two for tests (ValueError for "uniform" on a batch that is not).
    -> (pix, pix_off, info, status, png_status): image i at pix[pix_off[i]:pix_off[i+1]], height_i rows of ITS
    row_bytes (info says which); status the zlib decoder's; png_status the first that is not 0 of plan, gather,
    reconstruction (2, 3; 3, 8; 1 .. 3)."""
    pix, pix_off, info, status, png_status, _, _, _, total, _, _ = _png_mixed_files_to_pixels(file, file_off, file_len, flags, max_bytes,
                                                                                             route, False)
    return pix[:total], pix_off, info, status, png_status


def png_decode_mixed_files_rgba_batch(file, file_off, file_len=None, flags=0, max_bytes=0, route=None):
    """png_decode_mixed_files_batch with png_colour_mixed_batch behind the gather and png_expand_mixed_batch at the end
    -> (rgba, rgba_off, info, status, png_status): rgba[rgba_off[i]:rgba_off[i+1]].view(height_i, width_i, 4) is
    picture i as png_decode_files_rgba_batch makes it; png_status the first that is not 0 of plan, gather, colour,
    reconstruction and expansion (2, 3; 3, 8; 10, 11; 1 .. 3; 9)."""
    return _png_pixels_to_rgba(_png_mixed_files_to_pixels(file, file_off, file_len, flags, max_bytes, route, True))


# ------------------------------------------------------------------------------------------
# PNG encode: mixed batches (every picture's size and pair from its own record)
# ------------------------------------------------------------------------------------------

def png_encode_plan_one(record, count=None, trns_len=None, summary=0, analyse_status=0, allowed=0):
    """The encode plan of one picture (fdh_png_encode_plan_one: host arithmetic, no device call).  `record`: a mapping
    with the fields of fdh_png_info that matter here (status, width, height, bit_depth, colour_type, interlace; a field
    that is missing counts as 0); bit_depth == colour_type == 0 asks for the pair to be chosen.  count / trns_len: the
    palette's entries and how many of them have A < 255 (None: there is no palette); summary and analyse_status as
    png_analyse_batch gives them; allowed: bit c set = colour type c may be chosen, 0 = all.
    -> (status, bit_depth, colour_type, packed, types, prefix, file): status 0 ok, 3 the record is of neither kind,
    analyse_status where that is neither 0 nor 12, 13 no candidate left, 10 / 11 a palette record without a usable count /
    with trns_len above it, 2 beyond the encode steps' size limits; the sizes are all 0 unless the status is."""
    rec = _PngInfoRecord(**{k: int(record.get(k, 0)) for k, _ in _PngInfoRecord._fields_})
    have = count is not None and trns_len is not None
    c, t = C.c_uint32(int(count) if have else 0), C.c_uint32(int(trns_len) if have else 0)
    sizes = (C.c_uint64 * 4)()
    st = _lib.lib().fdh_png_encode_plan_one(C.byref(rec), C.byref(c) if have else None, C.byref(t) if have else None, int(summary),
                                            int(analyse_status), int(allowed), sizes)
    return (int(st), int(rec.bit_depth), int(rec.colour_type)) + tuple(int(v) for v in sizes)


def png_encode_records(width, height, pairs=None):
    """fdh_png_info records for n pictures to encode: int32 [n, 8] on the device of `width`.  width, height: int tensors
    [n]; pairs: None (dimension records: the plan chooses), a (bit_depth, colour_type) tuple for all, or an int tensor
    [n, 2] of them."""
    import torch
    n = width.numel()
    info = torch.zeros((n, PNG_INFO_WORDS), dtype=torch.int32, device=width.device)
    info[:, 1] = width.to(torch.int32)
    info[:, 2] = height.to(torch.int32)
    if pairs is not None:
        if not torch.is_tensor(pairs):
            pairs = torch.tensor([[int(pairs[0]), int(pairs[1])]], dtype=torch.int32, device=width.device).expand(n, 2)
        info[:, 3] = (pairs[:, 0].to(torch.int32) & 0xFF) | ((pairs[:, 1].to(torch.int32) & 0xFF) << 8)
    return info


def png_analyse_mixed_batch(rgba, rgba_off, info, max_colours=256, with_pal=True, upstream=None, pal=None, colour=None, trns_len=None,
                            summary=None, png_status=None):
    """png_analyse_batch at every picture's own width (fdh_png_analyse_mixed_batch): the slot of image i must be exactly
    height_i * width_i * 4 bytes.  info: dimension records or encodable ones (png_encode_records).
    -> (pal, colour, trns_len, summary, png_status) as png_analyse_batch; png_status also 3 (neither kind of record) or
    upstream[i] where that is not 0."""
    n = rgba_off.numel() - 1
    if with_pal:
        pal = _i32(pal, rgba, n, 256)
    colour, trns_len = _i32(colour, rgba, n, 4), _i32(trns_len, rgba, n)
    summary, png_status = _i32(summary, rgba, n), _i32(png_status, rgba, n)
    _call("fdh_png_analyse_mixed_batch", rgba, rgba_off, info, upstream, pal, colour, trns_len, summary, png_status, n,
          max_colours)
    return pal, colour, trns_len, summary, png_status


def png_encode_plan_batch(info, colour=None, trns_len=None, summary=None, analyse_status=None, allowed=0, pix_size=True,
                          types_size=True, prefix=True, file_size=True, png_status=None):
    """png_encode_plan_one for n records on the device (fdh_png_encode_plan_batch); `info` is changed in place: a dimension
    record gets its pair.  colour / trns_len / summary / analyse_status as png_analyse_mixed_batch writes them.  Each of the
    four outputs is True (allocated), a tensor (int64 [n]) or None / False (not wanted).
    -> (pix_size, types_size, prefix, file_size, png_status), None for an output that was not wanted."""
    n = info.numel() // PNG_INFO_WORDS
    outs = _wanted(info, n, pix_size, types_size, prefix, file_size)
    png_status = _i32(png_status, info, n)
    _call("fdh_png_encode_plan_batch", info, colour, trns_len, summary, analyse_status, int(allowed), *outs, png_status, n)
    return (*outs, png_status)


def png_pack_mixed_batch(rgba, rgba_off, pix, pix_off, info, pal=None, colour=None, upstream=None, png_status=None):
    """png_pack_batch at every picture's own pair and width (fdh_png_pack_mixed_batch): the slots must be exactly the plan's
    sizes.  An image of colour type 3 without `pal` is status 10.
    -> png_status: 0 ok, 2 the slots do not fit, 3 not encodable, 13 not representable, or upstream[i]."""
    n = rgba_off.numel() - 1
    png_status = _i32(png_status, rgba, n)
    _call("fdh_png_pack_mixed_batch", rgba, rgba_off, pix, pix_off, info, pal, colour, upstream, png_status, n)
    return png_status


def png_choose_filters_mixed_batch(pix, pix_off, types, types_off, info, upstream=None, png_status=None):
    """png_choose_filters_batch at every picture's own row_bytes and bpp (fdh_png_choose_filters_mixed_batch).
    -> png_status: 0 ok, 2 the slots are not the plan's, 3 not encodable, or upstream[i]."""
    n = pix_off.numel() - 1
    png_status = _i32(png_status, pix, n)
    _call("fdh_png_choose_filters_mixed_batch", pix, pix_off, types, types_off, info, upstream, png_status, n)
    return png_status


def png_filter_deflate_ultrafast_mixed_batch(pix, pix_off, types, types_off, out, out_off, info, upstream=None, out_len=None,
                                             png_status=None):
    """png_filter_deflate_ultrafast_batch at every picture's own row_bytes and bpp
    (fdh_png_filter_deflate_ultrafast_mixed_batch) -> (out_len, png_status): 0 ok, 1 a filter type above 4, 2 the slots are
    not the plan's, 3 not encodable, or upstream[i]; out_len 0xFFFFFFFF (-1) where the out slot is too small."""
    n = pix_off.numel() - 1
    out_len, png_status = _i32(out_len, pix, n), _i32(png_status, pix, n)
    _call("fdh_png_filter_deflate_ultrafast_mixed_batch", pix, pix_off, types, types_off, out, out_off, out_len, info, upstream,
          png_status, n)
    return out_len, png_status


def png_frame_mixed_batch(file, file_off, idat_len, info, pal=None, colour=None, trns_len=None, file_len=None, png_status=None):
    """png_frame_batch / png_frame_palette_batch with every file's own IHDR and, for colour type 3, a PLTE of exactly
    colour[i, 0] entries and a tRNS of exactly trns_len[i] bytes (fdh_png_frame_mixed_batch); the zlib streams lie the plan's
    prefix into their file slots.  -> (file_len, png_status): 0 ok, 3 not encodable, 2, 10, 11 as the framing calls (nothing
    written, file_len 0)."""
    n = file_off.numel() - 1
    file_len, png_status = _i32(file_len, file, n), _i32(png_status, file, n)
    _call("fdh_png_frame_mixed_batch", file, file_off, idat_len, info, pal, colour, trns_len, file_len, png_status, n)
    return file_len, png_status


def _png_encode_mixed_front(pictures, pictures_off, width, height, allowed, pairs, file, file_off, analyse, plan, pack, file_size=None):
    """What the mixed encode pipelines share in front of the filters, for RGBA8 pictures and (png16_encode) RGBA16 ones:
    the records, `analyse`, `plan`, the three running sums with the ONE read-back of 24 bytes, the file slots (the
    caller's, checked against prefix + 16, or the plan's) and `pack`.  file_size(pix_size, types_size, prefix, planned) ->
    the default file slots where they are not the plan's (png_levels).
    -> the five results of an empty batch, or (pix, offs, total_types, file, file_off, prefix, status, info, pal, colour,
    trns_len): offs[0] / offs[1] / offs[2] the offsets of the packed scanlines, the filter types and the default file slots."""
    import torch
    n = pictures_off.numel() - 1
    dev = pictures.device
    if (file is None) != (file_off is None):
        raise ValueError("file and file_off go together")
    info = png_encode_records(width, height, pairs)
    if n == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return (file if file is not None else torch.empty(0, dtype=torch.uint8, device=dev),
                file_off if file_off is not None else torch.zeros(1, dtype=torch.int64, device=dev), e, e.clone(), info)
    pal, colour, trns_len, summary, analysed = analyse(pictures, pictures_off, info)
    pix_size, types_size, prefix, file_sizes, planned = plan(info, colour, trns_len, summary, analysed, allowed)
    if pairs is not None:   # a forced palette pair with too many colours: the analysis' finding, not the plan's "no count"
        overflow = (analysed == PNG_TOO_MANY_COLOURS) & (((info[:, 3] >> 8) & 0xFF) == 3) & (planned == PNG_BAD_PLTE)
        planned = torch.where(overflow, analysed, planned)
    if file_size is not None:
        file_sizes = file_size(pix_size, types_size, prefix, planned)
    offs = torch.zeros((3, n + 1), dtype=torch.int64, device=dev)
    torch.cumsum(torch.stack((pix_size, types_size, file_sizes)), 1, out=offs[:, 1:])
    total_pix, total_types, total_file = _read_back(offs[:, n])                    # the one read-back: 24 bytes
    pix = torch.empty(max(1, total_pix), dtype=torch.uint8, device=dev)
    if file is None:
        file = torch.empty(max(1, total_file), dtype=torch.uint8, device=dev)
        file_off = offs[2]
    else:
        slot = file_off[1:] - file_off[:-1]
        planned = torch.where((planned == 0) & (slot < prefix + PNG_FILE_SUFFIX), torch.full_like(planned, PNG_BAD_SIZES), planned)
        prefix = torch.minimum(prefix, slot)
    status = pack(pictures, pictures_off, pix, offs[0], info, pal=pal, colour=colour, upstream=planned)
    return pix, offs, total_types, file, file_off, prefix, status, info, pal, colour, trns_len


def png_encode_mixed_rgba_files_batch(rgba, rgba_off, width, height, allowed=0, pairs=None, file=None, file_off=None):
    """RGBA8 pictures of any size in, PNG files out, each with the smallest of the depth / colour pairs that holds it (or with
    the pair `pairs` names, see png_encode_records), on torch's current stream: png_analyse_mixed_batch,
    png_encode_plan_batch, the buffers sized on the device with ONE read-back of 24 bytes (the three totals),
    png_pack_mixed_batch, png_choose_filters_mixed_batch, png_filter_deflate_ultrafast_mixed_batch, png_frame_mixed_batch.
    Picture i is rgba[rgba_off[i] .. rgba_off[i+1]), exactly height[i] * width[i] * 4 bytes; width, height: int tensors [n]
    on the device.  allowed: the colour types the plan may choose (bit c = colour type c, 0 = all).  file / file_off: the
    caller's file slots (both or neither); by default they are the plan's file sizes, which always suffice.
    -> (file, file_off, file_len, png_status, info): file i is file[file_off[i] : file_off[i] + file_len[i]]; info the
    records with the pairs that were written; png_status[i] the first that is not 0 of the plan (2, 3, 10, 11, 13, and 12
    for a forced palette pair with more than 256 colours), packing (2, 10, 13), filter selection, the encoder and the
    framing (2, 10, 11).  An image that fails gets file_len[i] = 0.
    The encoder takes ONE offsets array, as in png_encode_rgba_files_batch: enc_off[i] = file_off[i] + prefix_i, so the
    encoder's slot for image i reaches prefix_(i+1) bytes into slot i + 1 -- the bytes that image i + 1's own prefix is
    written to afterwards -- and the last one ends 16 bytes in front of its slot's end.  A caller's slot that is shorter
    than its prefix + 16 is status 2 before anything is written to it."""
    import torch
    front = _png_encode_mixed_front(rgba, rgba_off, width, height, allowed, pairs, file, file_off, png_analyse_mixed_batch,
                                    png_encode_plan_batch, png_pack_mixed_batch)
    if len(front) == 5:
        return front
    pix, offs, total_types, file, file_off, prefix, status, info, pal, colour, trns_len = front
    types = torch.empty(max(1, total_types), dtype=torch.uint8, device=rgba.device)
    status = png_choose_filters_mixed_batch(pix, offs[0], types, offs[1], info, upstream=status)
    enc_off = _enc_off(file_off, prefix)
    idat_len, status = png_filter_deflate_ultrafast_mixed_batch(pix, offs[0], types, offs[1], file, enc_off, info, upstream=status)
    idat_len = torch.where(status != 0, torch.zeros_like(idat_len), idat_len)     # (the framing then writes nothing)
    file_len, framed = png_frame_mixed_batch(file, file_off, idat_len, info, pal, colour, trns_len)
    return file, file_off, file_len, _first(status, framed), info


# ------------------------------------------------------------------------------------------
# PNG encode from RGBA8: analysis, packing, palette files
# ------------------------------------------------------------------------------------------

def png_analyse_batch(rgba, rgba_off, width, max_colours=256, with_pal=True, pal=None, colour=None, trns_len=None, summary=None,
                      png_status=None):
    """What n RGBA8 images are (fdh_png_analyse_batch): image i is rgba[rgba_off[i] .. rgba_off[i+1]), whole rows of
    width * 4 bytes.  -> (pal, colour, trns_len, summary, png_status): pal int32 [n, 256], the distinct pixels as words
    R | G << 8 | B << 16 | A << 24 in ascending unsigned order -- entries with A < 255 first --, 0xFF000000 behind the count
    (None with with_pal=False); colour int32 [n, 4], word 0 the count; trns_len int32 [n], the entries with A < 255;
    summary int32 [n]: PNG_SUMMARY_OPAQUE, PNG_SUMMARY_GREY, bits 8 .. 15 the smallest sample depth of 1, 2, 4, 8 that
    loses nothing; png_status 0 ok, 2 the slot is not whole rows (nothing written for the image), PNG_TOO_MANY_COLOURS
    (12: more than max_colours distinct pixels; only summary is valid)."""
    n = rgba_off.numel() - 1
    if with_pal:
        pal = _i32(pal, rgba, n, 256)
    colour, trns_len = _i32(colour, rgba, n, 4), _i32(trns_len, rgba, n)
    summary, png_status = _i32(summary, rgba, n), _i32(png_status, rgba, n)
    _call("fdh_png_analyse_batch", rgba, rgba_off, pal, colour, trns_len, summary, png_status, n, width, max_colours)
    return pal, colour, trns_len, summary, png_status


def png_pack_batch(rgba, rgba_off, pix, pix_off, width, bit_depth, colour_type, pal=None, colour=None, upstream=None,
                   png_status=None):
    """RGBA8 to packed scanlines, the inverse of png_expand_batch (fdh_png_pack_batch): image i, whole rows of width * 4
    bytes at rgba_off[i] .. rgba_off[i+1], goes to the slot pix[pix_off[i] .. pix_off[i+1]) of exactly rows * row_bytes
    bytes.  pal / colour as png_analyse_batch or png_colour_batch write them (pal is needed for colour type 3: the index
    is the lowest one whose word equals the pixel; without colour all 256 words count); upstream (int32 [n]): where not 0
    the image is skipped and its png_status is that value.  -> png_status: 0 ok, 2 the slots do not fit (nothing
    written), PNG_NOT_REPRESENTABLE (13: some pixel cannot be held by the pair without loss)."""
    n = rgba_off.numel() - 1
    png_status = _i32(png_status, rgba, n)
    _call("fdh_png_pack_batch", rgba, rgba_off, pix, pix_off, pal, colour, upstream, png_status, n, width, bit_depth,
          colour_type)
    return png_status


def png_palette_file_prefix(plte_entries, trns_entries):
    """The bytes in front of the zlib stream of a palette file with a PLTE of plte_entries entries and, where trns_entries
    is not 0, a tRNS of that many bytes: 41 + 12 + 3 E + (12 + T) (fdh_png_palette_file_prefix)."""
    v = int(_lib.lib().fdh_png_palette_file_prefix(int(plte_entries), int(trns_entries)))
    if v == 0:
        raise ValueError("plte_entries must be 1 .. 256 and trns_entries 0 .. plte_entries")
    return v


def png_frame_palette_batch(file, file_off, idat_len, height, pal, colour, trns_len, width, bit_depth, plte_entries, trns_entries,
                            file_len=None, png_status=None):
    """png_frame_batch for colour type 3 (fdh_png_frame_palette_batch): signature, IHDR, a PLTE of plte_entries entries
    (the colour[i, 0] words of pal[i], then zeros), a tRNS of trns_entries alphas where that is not 0, and the IDAT's head
    in front of the zlib streams that lie png_palette_file_prefix(plte_entries, trns_entries) bytes into their file slots;
    the IDAT's CRC and IEND behind them.  -> (file_len, png_status): 0 ok, 2 as png_frame_batch, 10 colour[i, 0] is 0 or
    above plte_entries, 11 trns_len[i] is above trns_entries (nothing written, file_len 0)."""
    n = file_off.numel() - 1
    file_len, png_status = _i32(file_len, file, n), _i32(png_status, file, n)
    _call("fdh_png_frame_palette_batch", file, file_off, idat_len, height, pal, colour, trns_len, file_len, png_status, n, width,
          bit_depth, plte_entries, trns_entries)
    return file_len, png_status


def _png_rgba_to_files(rgba, rgba_off, file, file_off, width, pixel_bytes, row_bytes, bpp, prefix, pack, frame):
    """The steps that png_encode_rgba_files_batch and png16.png_encode_rgba16_files_batch share, for pictures of
    `pixel_bytes` per pixel: pack(pix, pix_off) -> png_status fills the packed rows, the fused filter + ultra-fast encode
    writes the streams at file_off + prefix, and frame(idat_len, height) -> (file_len, png_status) writes the chunks
    around them.  -> (file_len, png_status)."""
    import torch
    n = rgba_off.numel() - 1
    dev = rgba.device
    if n == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return e, e.clone()
    rows = (rgba_off[1:] - rgba_off[:-1]) // (width * pixel_bytes)
    height = rows.clamp(max=0xFFFFFFFF).to(torch.int32)                       # (bit pattern of the u32)
    # packed rows and one filter type per row; both buffers are sized by what `rgba` could hold at most: no read-back
    pix_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(rows * row_bytes, 0, out=pix_off[1:])
    types_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(rows, 0, out=types_off[1:])
    most = max(1, rgba.numel() // (width * pixel_bytes))
    pix = torch.empty(most * row_bytes, dtype=torch.uint8, device=dev)
    types = torch.empty(most, dtype=torch.uint8, device=dev)
    packed = pack(pix, pix_off)
    enc_off = _enc_off(file_off, prefix)
    idat_len, enc_status, _ = png_encode_ultrafast_batch(pix, pix_off, file, enc_off, row_bytes, bpp, types=types, types_off=types_off)
    before = _first(packed, enc_status)
    idat_len = torch.where(before != 0, torch.zeros_like(idat_len), idat_len)     # (the framing then writes nothing)
    file_len, framed = frame(idat_len, height)
    return file_len, _first(before, framed)


def png_encode_rgba_files_batch(rgba, rgba_off, file, file_off, width, bit_depth, colour_type, plte_entries=None, trns_entries=None):
    """RGBA8 pictures in, PNG files of the given depth / colour type out, on torch's current stream and without a read-back:
    for colour type 3 png_analyse_batch (max_colours = plte_entries, by default min(256, 2^bit_depth); trns_entries is
    plte_entries by default), then png_pack_batch, the rows' filter types and the fused filter + ultra-fast encode
    (png_encode_ultrafast_batch) at file_off + the prefix, and png_frame_batch or png_frame_palette_batch around the
    streams.  Image i is rgba[rgba_off[i] .. rgba_off[i+1]), whole rows of width * 4 bytes; its file goes to the slot
    file[file_off[i] .. file_off[i+1]) -- png_file_bound(rows, row_bytes), plus png_palette_file_prefix(..) - 41 for a
    palette file, always suffices.
    -> (file_len, png_status): png_status[i] is the first that is not 0 of analyse (2, 12), pack (2, 13), the encoder and
    the framing (2, 10, 11); an image that failed in front of the framing gets no file: file_len[i] = 0, nothing is framed,
    and the contents of its file slot are not specified (the encoder has run over that image's packed slot, which pack did
    not write: disregard the slot).
    The encoders take ONE offsets array, so the encoder's slot for image i reaches `prefix` bytes into slot i + 1 (the
    last one ends 16 bytes in front of its slot's end): the bytes that image i + 1's own prefix is written to afterwards.
    A stream that does not fit its file slot can therefore leave bytes in the first `prefix` of the next slot; they stay
    there only if that next image fails as well."""
    row_bytes, bpp = png_geometry(width, bit_depth, colour_type)
    if colour_type == 3:
        if plte_entries is None:
            plte_entries = min(256, 1 << bit_depth)
        if trns_entries is None:
            trns_entries = plte_entries
        if not 1 <= plte_entries <= min(256, 1 << bit_depth) or not 0 <= trns_entries <= plte_entries:
            raise ValueError("plte_entries must be 1 .. min(256, 2^bit_depth) and trns_entries 0 .. plte_entries")
        prefix = png_palette_file_prefix(plte_entries, trns_entries)
    else:
        prefix = PNG_FILE_PREFIX
    pal = colour = trns_len = None

    def pack(pix, pix_off):
        nonlocal pal, colour, trns_len
        upstream = None
        if colour_type == 3:
            pal, colour, trns_len, _, upstream = png_analyse_batch(rgba, rgba_off, width, max_colours=plte_entries)
        return png_pack_batch(rgba, rgba_off, pix, pix_off, width, bit_depth, colour_type, pal=pal, colour=colour, upstream=upstream)

    def frame(idat_len, height):
        if colour_type == 3:
            return png_frame_palette_batch(file, file_off, idat_len, height, pal, colour, trns_len, width, bit_depth, plte_entries,
                                           trns_entries)
        return png_frame_batch(file, file_off, idat_len, height, width, bit_depth, colour_type)

    return _png_rgba_to_files(rgba, rgba_off, file, file_off, width, 4, row_bytes, bpp, prefix, pack, frame)


def inflate_batch_multi(shards, flags=0, gather=True):
    """fdh_inflate_batch_multi from one process: `shards` = one tuple (comp, in_off, out, out_off) of
    tensors per GPU selected by init_devices(); returns per shard (out_len, status, adler) and, with
    gather, the all-gathered results [n_shards, 3, stride] on every device."""
    import torch
    L = _lib.lib()
    n_sh = len(shards)
    arr = (_lib.Shard * n_sh)()
    keep, results, metas = [], [], []
    stride = max(s[1].numel() - 1 for s in shards)
    for i, (comp, in_off, out, out_off) in enumerate(shards):
        dev = comp.device
        n = in_off.numel() - 1
        ol = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        ad = torch.empty(n, dtype=torch.int32, device=dev)
        meta = torch.empty((n_sh, 3, stride), dtype=torch.int32, device=dev) if gather else None
        keep.append((comp, in_off, out, out_off))
        results.append((ol, st, ad))
        metas.append(meta)
        arr[i] = _lib.Shard(comp.data_ptr(), in_off.data_ptr(), out.data_ptr(), out_off.data_ptr(), ol.data_ptr(),
                            st.data_ptr(), ad.data_ptr(), n, meta.data_ptr() if gather else None)
    for t in keep:
        torch.cuda.synchronize(t[0].device)   # the call runs on the library's own streams
    _lib.check(L.fdh_inflate_batch_multi(C.byref(arr), n_sh, flags, stride))
    return results, metas


def init_devices(mask=0):
    """fdh_init: select the GPUs (bit mask, 0 = all visible) for inflate_batch_multi."""
    _lib.check(_lib.lib().fdh_init(mask))
    return _lib.lib().fdh_multi_device_count()


def multi_uses_rccl():
    """True if inflate_batch_multi gathers through RCCL (more than one device, or FDH_MULTI_FORCE_RCCL=1)."""
    return bool(_lib.lib().fdh_multi_uses_rccl())


def shutdown_devices():
    _lib.check(_lib.lib().fdh_shutdown())


def debug_build_tables(code_lengths, hlit):
    """Device Huffman-table builder on one set of 320 code lengths -> (status, litlen, dist, eof)."""
    import torch
    cl = torch.as_tensor(list(code_lengths), dtype=torch.uint8).cuda()
    lit = torch.empty(4096, dtype=torch.int32, device="cuda")
    dist = torch.empty(512, dtype=torch.int32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    _call("fdh_debug_build_tables", cl, hlit, lit, dist, st)
    torch.cuda.synchronize()
    s = st.cpu().tolist()
    return s[0], lit.cpu().numpy().view("uint32"), dist.cpu().numpy().view("uint32"), tuple(s[1:])
