"""fdeflate_amd -- MI355X-native batched DEFLATE codec behind fdeflate's PNG-path API.

Public surface mirrors image-rs/fdeflate (reference src/lib.rs:29-36) for the hot path:
decompress_to_vec, decompress_to_vec_bounded, compress_to_vec_ultra_fast, DecompressionError,
plus the batched device entry points.  See DESIGN.md / INTEGRATION.md.
"""
from .api import (Decompressor, DecompressionError, OutputTooLarge, STATUS_NAMES, FLAG_IGNORE_ADLER32,
                  FLAG_SERIAL_ONLY, FLAG_GENERAL_ONLY, FLAG_NO_RECHECK, compress_to_vec_ultra_fast, debug_build_tables,
                  decompress_to_vec, decompress_to_vec_bounded, deflate_ultrafast_batch,
                  inflate_batch, inflate_batch_resumable, ultrafast_bound, compress_to_vec_stored, deflate_stored_batch,
                  stored_size, compress_to_vec, compress_to_vec_rle, compress_to_vec_with_level, compress_bound,
                  deflate_general_batch, MODE_LEVEL2, MODE_LEVEL3,
                  MODE_LEVEL1, MODE_RLE, inflate_batch_multi, init_devices, shutdown_devices, multi_uses_rccl,
                  png_unfilter_batch, png_filter_batch, inflate_png_batch, png_filter_deflate_ultrafast_batch,
                  png_choose_filters_batch, png_encode_ultrafast_batch,
                  crc32_batch, png_file_bound, png_geometry, png_frame_batch, png_encode_files_batch, png_scan_files_batch,
                  png_info_fields, png_gather_idat_batch, png_decode_files_batch, PNG_FILE_PREFIX, PNG_FILE_SUFFIX,
                  PNG_FLAG_IGNORE_CRC, PNG_SCAN_STATUS_NAMES, PNG_OTHER_GEOMETRY, PNG_COMP_SLOT_TOO_SMALL,
                  PNG_INDEX_OUTSIDE_PALETTE, PNG_BAD_PLTE, PNG_BAD_TRNS, png_colour_batch, png_expand_batch,
                  png_decode_files_rgba_batch, PNG_FLAG_ADAM7, png_adam7_size, png_unfilter_interlaced_batch,
                  PNG_OK, PNG_BAD_FILTER_TYPE, PNG_BAD_SIZES, PNG_SKIPPED, PNG_SCAN_NO_SIGNATURE, PNG_SCAN_TRUNCATED,
                  PNG_SCAN_BAD_IHDR, PNG_SCAN_INTERLACED, PNG_SCAN_CHUNK_STRUCTURE, PNG_SCAN_CRC_MISMATCH,
                  PNG_TOO_MANY_COLOURS, PNG_NOT_REPRESENTABLE, PNG_SUMMARY_OPAQUE, PNG_SUMMARY_GREY, PNG_ANALYSE_HASH_MUL,
                  PNG_ANALYSE_HASH_BITS, png_analyse_batch, png_pack_batch, png_palette_file_prefix, png_frame_palette_batch,
                  png_encode_rgba_files_batch)

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
]
