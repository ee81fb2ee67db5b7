/*
 * fdeflate_hip.h -- C ABI of the MI355X-native batched DEFLATE codec (PNG path).
 *
 * Drop-in boundary for image-rs/fdeflate's public API on the PNG hot path
 * (reference: /root/reference/src/lib.rs:29-36).  The reference has no FFI of its own;
 * each entry point below names the Rust item it replaces.  A Rust shim crate binds these
 * with `extern "C"` (see INTEGRATION.md for the exact stub).
 *
 * Conventions
 *   - plain pointers and sizes, no torch / C++ types;
 *   - `*_batch` entry points take DEVICE pointers (HBM resident) and a hipStream_t passed as
 *     `void*` (NULL = the null stream); they enqueue work and return without synchronising;
 *   - function return value = infrastructure status (0 ok, non-zero = HIP / argument failure,
 *     message via fdh_last_error()); per-stream results are in `status[]`;
 *   - the library never falls back to a CPU path: without a usable GPU every entry point that
 *     does work returns FDH_ERR_NO_DEVICE.
 */
#ifndef FDEFLATE_HIP_H
#define FDEFLATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDH_VERSION 0x000100u

/* ---- library-level return codes ---------------------------------------------------- */
enum {
    FDH_SUCCESS = 0,
    FDH_ERR_INVALID_ARGUMENT = 1,
    FDH_ERR_NO_DEVICE = 2,
    FDH_ERR_HIP = 3,
    FDH_ERR_OUT_OF_MEMORY = 4
};

/* ---- per-stream status --------------------------------------------------------------
 * 0 = Ok, otherwise 1 + ordinal of `DecompressionError` (src/decompress.rs:14-48), plus one
 * ABI-only code for `BoundedDecompressionError::OutputTooLarge` (src/decompress.rs:1097-1101). */
enum {
    FDH_STREAM_OK = 0,
    FDH_BAD_ZLIB_HEADER = 1,
    FDH_INSUFFICIENT_INPUT = 2,
    FDH_INVALID_BLOCK_TYPE = 3,
    FDH_INVALID_UNCOMPRESSED_BLOCK_LENGTH = 4,
    FDH_INVALID_HLIT = 5,
    FDH_INVALID_HDIST = 6,
    FDH_INVALID_CODE_LENGTH_REPEAT = 7,
    FDH_BAD_CODE_LENGTH_HUFFMAN_TREE = 8,
    FDH_BAD_LITERAL_LENGTH_HUFFMAN_TREE = 9,
    FDH_BAD_DISTANCE_HUFFMAN_TREE = 10,
    FDH_INVALID_LITERAL_LENGTH_CODE = 11,
    FDH_INVALID_DISTANCE_CODE = 12,
    FDH_INPUT_STARTS_WITH_RUN = 13,
    FDH_DISTANCE_TOO_FAR_BACK = 14,
    FDH_WRONG_CHECKSUM = 15,
    FDH_EXTRA_INPUT = 16,
    FDH_OUTPUT_TOO_LARGE = 17
};

/* ---- flags -------------------------------------------------------------------------- */
#define FDH_FLAG_IGNORE_ADLER32 0x1u /* Decompressor::ignore_adler32, src/decompress.rs:154 */
#define FDH_FLAG_SERIAL_ONLY    0x2u /* debug/A-B: force the per-symbol wave-serial decoder */
#define FDH_FLAG_GENERAL_ONLY   0x4u /* debug/A-B: skip the shared-table kernel */
#define FDH_FLAG_NO_RECHECK     0x8u /* tests: do not re-derive non-Ok results serially */
#define FDH_FLAG_FORCE_LANES    0x10u /* tests/A-B: stream-per-lane kernel even for small batches */
#define FDH_FLAG_NO_LANES       0x20u /* tests/A-B: never use the stream-per-lane kernel */
#define FDH_FLAG_FIRST_ONLY     0x40u /* debug: run only the first kernel of the pipeline */
#define FDH_FLAG_NO_SEGMENTS    0x80u /* tests/A-B: skip the segment-parallel kernel */
#define FDH_FLAG_NO_FAST_GENERAL 0x200u /* tests/A-B: skip the small-table general kernel */
#define FDH_FLAG_NO_INTERVALS   0x400u /* tests/A-B: skip the interval kernel (segment kernel first, as in round 2) */
#define FDH_FLAG_INTERVALS_ONLY 0x800u /* debug: run only the interval kernel (what it leaves stays PENDING) */
#define FDH_FLAG_NO_LZ          0x1000u /* tests/A-B: skip the LZ-window kernel (general streams go to the tile decoders) */
#define FDH_FLAG_LZ_ONLY        0x2000u /* debug: nothing behind the LZ-window kernel runs (what it leaves stays PENDING) */
#define FDH_FLAG_RESUME_IN      0x8000u /* fdh_inflate_batch_resumable: `resume` also says where to take each stream up */
#define FDH_FLAG_NO_CHECKPOINTS 0x4000u /* tests/A-B: the exact serial decoder re-derives a doubtful result from the stream's first byte, not from the last check point */
#define FDH_FLAG_NO_LANDING     0x10000u /* tests/A-B: skip the landing decoder (the interval kernel counts for itself, as in rounds 3-4) */
#define FDH_FLAG_LANDING_ONLY   0x20000u /* debug: run only the landing decoder (what it leaves stays PENDING) */
#define FDH_FLAG_NO_LEAN_WRITE   0x80000u /* tests/A-B: the landing decoder always takes the interval decoder's general writing pass */
#define FDH_FLAG_NO_OVERLAP      0x100000u /* tests/A-B: the LZ-window kernel runs behind the canonical kernels, not beside them */
#define FDH_FLAG_TAIL_LONG       0x200000u /* tests/A-B: behind the landing decoder always the five kernels of rounds 3-5 (interval, segment, tile decoders, two exact kernels) */
#define FDH_FLAG_TAIL_SHORT      0x400000u /* tests/A-B: behind the landing decoder always the exact kernel alone (the library chooses by what recent calls left over) */
#define FDH_FLAG_ORDER_ONCE      0x800000u /* tests/A-B: stream_order_kernel lists the streams without the ultra-fast prefix in one launch, in no order */
#define FDH_FLAG_ORDER_TWICE     0x1000000u /* tests/A-B: ... always in two (the long ones first), as in rounds 4-5 (the library chooses by how many recent calls had) */
#define FDH_FLAG_LANDING_COUNT_ONLY 0x40000u /* debug: the landing decoder counts and leaves every stream PENDING */
#define FDH_FLAG_SPANS          0x100u /* experimental: segment-parallel "span" decoder inside the 12-bit general kernel */

/*
 * fdh_inflate_batch -- one-shot decode of `n` independent zlib streams, one wavefront each.
 *
 * Replaces, per stream i: `decompress_to_vec_bounded(&in[in_off[i]..in_off[i+1]],
 * out_off[i+1]-out_off[i])` (src/decompress.rs:1111-1144), i.e. a `Decompressor::new()`
 * (src/decompress.rs:123) driven by `Decompressor::read` (src/decompress.rs:179-337) until
 * `is_done()` (src/decompress.rs:340), with the slot capacity as `maxlen`.
 *
 *   in, in_off[n+1]    packed compressed bytes; stream i = in[in_off[i] .. in_off[i+1])
 *   out, out_off[n+1]  output slots; capacity of stream i = out_off[i+1] - out_off[i]
 *                      (< 4 GiB); bytes outside [out_off[i], out_off[i+1]) are never written
 *   out_len[n]         decoded length; on FDH_OUTPUT_TOO_LARGE the capacity (the slot holds the
 *                      partial output like `partial_output`); on FDH_INSUFFICIENT_INPUT the bytes
 *                      `Decompressor::read` had produced when the input ran out (they are in the
 *                      slot); unspecified for other errors
 *   status[n]          per-stream status (above)
 *   adler[n]           Adler-32 of the decoded bytes (nullable): of all out_len[i] bytes for FDH_OK,
 *                      FDH_WRONG_CHECKSUM and FDH_OUTPUT_TOO_LARGE; for any other status the value is that of a
 *                      prefix of them and not specified further (a decoder that takes back the first literal of a
 *                      cut-off pair -- src/decompress.rs:852 -- keeps the sum it had reached)
 *   flags              FDH_FLAG_*
 * All pointers are device pointers.  Truncated input reports FDH_INSUFFICIENT_INPUT exactly as
 * the one-shot wrapper does (src/decompress.rs:1135-1136); bytes after the Adler-32 trailer are
 * ignored (src/decompress.rs:185-187).
 */
int fdh_inflate_batch(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                      const uint64_t *out_off, uint32_t *out_len, uint32_t *status,
                      uint32_t *adler, uint64_t n, uint32_t flags, void *hip_stream);

/*
 * fdh_inflate_batch_resumable -- fdh_inflate_batch that can stop and go on: the device-side counterpart of
 * the reference's resumable `Decompressor` (State / BitBuffer / QueuedOutput, src/decompress.rs:84-121), for
 * callers that get a stream's input or its output room in pieces (fdh_decompressor_read is built on it).
 *
 *   resume[n]   (device) per stream, 16 bytes.  OUT: for a stream that ended FDH_INSUFFICIENT_INPUT or
 *               FDH_OUTPUT_TOO_LARGE, a place inside the stream from which decoding can go on later -- a bit
 *               position at the start of one of the reference's decoding steps, the header of the block it
 *               lies in, the number of output bytes in front of it and their Adler-32 -- or all zero (go on
 *               from the first byte).  All zero for every other status.
 *               IN, with FDH_FLAG_RESUME_IN: where to take each stream up in THIS call (all zero: at its first
 *               byte).  The stream's input must start with the same bytes as in the call that produced the
 *               record (more may have arrived behind them), and its output slot must start at the same
 *               place in the caller's data: it holds the `out_bytes` decoded so far (the LZ77 history) and
 *               may have grown.  With that flag the LZ-window kernel goes on from the record and the
 *               12-bit tile / serial decoders do the rest (the segment-parallel kernels for ultra-fast
 *               streams start at a stream's first byte and do not run).
 * Status, length and Adler-32 of a stream that was stopped and taken up again -- any number of times, at any
 * split of input and output -- equal those of one fdh_inflate_batch call on the whole of it.
 */
typedef struct fdh_resume_point {
  uint32_t header_bit; /* stream bit of the block header, | step state << 30; 0: no resume point */
  uint32_t bit;        /* stream bit to go on from */
  uint32_t out_bytes;  /* output bytes in front of it */
  uint32_t adler32;    /* their Adler-32 */
} fdh_resume_point;
int fdh_inflate_batch_resumable(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                                const uint64_t *out_off, uint32_t *out_len, uint32_t *status,
                                uint32_t *adler, uint64_t n, uint32_t flags,
                                fdh_resume_point *resume, void *hip_stream);

/*
 * fdh_deflate_ultrafast_batch -- `compress_to_vec_ultra_fast` (src/compress/mod.rs:313-317,
 * UltraFastCompressor src/compress/ultrafast.rs:9-182) of `n` buffers, one wavefront each,
 * bit-exact with the reference's byte stream.
 *   in, in_off[n+1]    raw buffers
 *   out, out_off[n+1]  output slots, capacity >= fdh_ultrafast_bound(len_i) each
 *   out_len[n]         compressed length; 0xFFFFFFFF if the slot was too small (nothing valid)
 */
int fdh_deflate_ultrafast_batch(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                                const uint64_t *out_off, uint32_t *out_len, uint64_t n,
                                void *hip_stream);

/* Worst-case size of an ultra-fast stream: 53 header bytes + ceil((5 + 12*len + 12)/8) + 4. */
uint64_t fdh_ultrafast_bound(uint64_t len);

/*
 * fdh_deflate_stored_batch -- level 0: `compress_to_vec_with_level(input, 0)`
 * (src/compress/mod.rs:299-303; `Compressor::new(.., 0, true)` :69-71, stored blocks :234-268,
 * finish :194-214), bit-exact: header 78 01, stored blocks of <= 65535 bytes, an empty fixed block
 * when the length is a multiple of 65535 (incl. 0), Adler-32.  Same argument convention as
 * fdh_deflate_ultrafast_batch; slots of at least fdh_stored_size(len_i) bytes.
 */
int fdh_deflate_stored_batch(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                             const uint64_t *out_off, uint32_t *out_len, uint64_t n,
                             void *hip_stream);
/* Exact size of the level-0 stream of a `len`-byte buffer. */
uint64_t fdh_stored_size(uint64_t len);

/*
 * fdh_deflate_general_batch -- the general encoder on `n` buffers, bit-exact (a parser kernel, one
 * stream per lane, records the back-references and block ends; a block-writer kernel, one stream
 * per wavefront, builds the Huffman codes and emits):
 *   FDH_MODE_LEVEL1  `compress_to_vec(input)` = `compress_to_vec_with_level(input, 1)`
 *                    (src/compress/mod.rs:294-303; Compressor::new(.., 1, true) :69-101 =
 *                    GreedyParser src/compress/parse/greedy.rs + HashTableMatchFinder
 *                    src/compress/matchfinder/hashtable.rs, dynamic blocks src/compress/bitstream.rs)
 *   FDH_MODE_RLE     `compress_to_vec_rle(input)` (src/compress/mod.rs:306-310; Compressor::new_rle
 *                    :107-123 = RleParser src/compress/parse/rle.rs)
 *   FDH_MODE_LEVEL2  `compress_to_vec_with_level(input, 2)` (src/compress/mod.rs:77-78: GreedyParser,
 *                    skip_ahead_shift 6, HashChainMatchFinder::<true>::new(8, 16, 64)
 *                    src/compress/matchfinder/hashchain.rs)
 *   FDH_MODE_LEVEL3  `compress_to_vec_with_level(input, 3)` (src/compress/mod.rs:79: GreedyParser,
 *                    skip_ahead_shift 6, HashChainMatchFinder::<false>::new(6, 16, 32), 4-byte
 *                    match_length src/compress/matchfinder/mod.rs:51-110)
 * Levels 4-9 (LazyParser + HybridMatchFinder, src/compress/mod.rs:80-99) are not provided by this call or by
 * fdh_compress_to_vec_with_level: the extension fdeflate_hip_levels.h has them (fdh_deflate_level_batch).  Levels 2
 * and 3 are pinned by tests/level_model.py, a restatement that is itself pinned against the oracle
 * at level 1 and RLE; the oracle has no chain finder.
 * Same argument convention as fdh_deflate_ultrafast_batch; slots of at least fdh_compress_bound(len_i)
 * bytes; out_len[i] = 0xFFFFFFFF if a slot was too small or the buffer exceeds 1 GiB.  The call
 * uses a per-device workspace (per resident stream one 256 KiB hash table at level 1, a 256 KiB head
 * table and a 128 KiB link ring at levels 2 and 3, at most 16 GiB -- so fewer streams are resident at
 * levels 2 and 3; 8 bytes per 4 input bytes for the back-reference records), reads in_off[0] and in_off[n]
 * back to size it, and returns after the kernels have finished.
 */
#define FDH_MODE_LEVEL1 1u
#define FDH_MODE_RLE 2u
#define FDH_MODE_LEVEL2 3u /* src/compress/mod.rs:77-78 */
#define FDH_MODE_LEVEL3 4u /* src/compress/mod.rs:79 */
int fdh_deflate_general_batch(const uint8_t *in, const uint64_t *in_off, uint8_t *out,
                              const uint64_t *out_off, uint32_t *out_len, uint64_t n, uint32_t mode,
                              void *hip_stream);
/* Slot size that always suffices for the general encoder: len + len / 2 + 1024. */
uint64_t fdh_compress_bound(uint64_t len);

/* ---- PNG scanline filters: the steps either side of the codec in the PNG pipeline --------
 * Not in the fdeflate crate (its reverse dependency image-rs/image-png does them, reference
 * README.md:11); the algorithm is the PNG specification's (W3C / ISO/IEC 15948, 9.2 and 9.4):
 * filter types 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth, `bpp` bytes per pixel (1, 2, 3, 4, 6, 8).
 * One image per lane.  A "filtered" image is rows x (1 + row_bytes) bytes, the type byte first (what
 * the zlib stream of an IDAT holds); a "pixel" image is rows x row_bytes.  rows_i = size_i / row size.
 *   fdh_png_unfilter_batch  reconstruction: filt -> pix
 *   fdh_png_filter_batch    filtering with the given per-row types: pix -> filt (types_off[n+1]
 *                           into `types`, one byte per row)
 *   fdh_png_choose_filters_batch  the per-row types for either of the two filtering calls, chosen
 *                           from the pixels (below)
 *   fdh_inflate_png_batch   fdh_inflate_batch into `filt` (the slots must be the exact image sizes)
 *                           followed, on the same stream, by the reconstruction into `pix` of every
 *                           stream that decoded to exactly the bytes of its slot
 * png_status[i]: 0 ok, 1 a filter type > 4, 2 sizes do not fit (fdh_inflate_png_batch: also a stream
 * that ended before its slot was full -- short IDAT data), 3 skipped (stream did not decode). */
#define FDH_PNG_STATUS_OK 0u
#define FDH_PNG_STATUS_BAD_FILTER_TYPE 1u
#define FDH_PNG_STATUS_BAD_SIZES 2u
#define FDH_PNG_STATUS_SKIPPED 3u
int fdh_png_unfilter_batch(const uint8_t *filt, const uint64_t *filt_off, uint8_t *pix,
                           const uint64_t *pix_off, uint32_t *png_status, uint64_t n,
                           uint32_t row_bytes, uint32_t bpp, void *hip_stream);
int fdh_png_filter_batch(const uint8_t *pix, const uint64_t *pix_off, const uint8_t *types,
                         const uint64_t *types_off, uint8_t *filt, const uint64_t *filt_off,
                         uint32_t *png_status, uint64_t n, uint32_t row_bytes, uint32_t bpp,
                         void *hip_stream);
/* Filter selection: which type each row is filtered with, from the pixels alone -- the heuristic of the
 * PNG specification (12.8, libpng's default, "minimum sum of absolute differences").  For every row
 * the five filtered versions are formed (row 0 has zeros above it), every filtered byte v is read as
 * signed and costs v < 128 ? v : 256 - v (so 128 costs 128), the costs of the row's row_bytes bytes are
 * summed (the type byte is not counted), and the type with the smallest sum is written to `types`, one
 * byte per row.  On equal sums the LOWEST type number wins (None < Sub < Up < Average < Paeth); row 0 is
 * therefore only ever 0, 1 or 3.  `types` / `types_off` are exactly what fdh_png_filter_batch and
 * fdh_png_filter_deflate_ultrafast_batch take: choosing and encoding are two calls on one stream with no
 * round trip between them.  No workspace, no host synchronisation.
 * png_status[i]: 0 ok; 2 the pixel slot is not a whole number of rows, or the types slot
 * types_off[i+1] - types_off[i] is not exactly the row count: nothing is written for that image.  (1 does
 * not occur.)  Bytes outside the types slots are never written.  row_bytes == 0, row_bytes >= 2^25 (the
 * sums are 32 bits wide) or a bpp outside the list: FDH_ERR_INVALID_ARGUMENT. */
int fdh_png_choose_filters_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *types,
                                 const uint64_t *types_off, uint32_t *png_status, uint64_t n,
                                 uint32_t row_bytes, uint32_t bpp, void *hip_stream);
/* Filtering fused into the ultra-fast encoder: pixel rows in (`pix`, rows_i x row_bytes), one filter
 * type per row in `types`, out the zlib stream compress_to_vec_ultra_fast(filtered image) -- what an
 * IDAT holds.  The filtered bytes exist only in registers (no intermediate buffer).  Slots of at
 * least fdh_ultrafast_bound(rows_i * (row_bytes + 1)) bytes; out_len[i] = 0 where png_status[i] != 0.
 * A slot that is too small for the stream is no PNG error: png_status[i] = 0 and out_len[i] = 0xFFFFFFFF, as
 * with fdh_deflate_ultrafast_batch (nothing valid in the slot, nothing written outside it). */
int fdh_png_filter_deflate_ultrafast_batch(const uint8_t *pix, const uint64_t *pix_off,
                                           const uint8_t *types, const uint64_t *types_off,
                                           uint8_t *out, const uint64_t *out_off, uint32_t *out_len,
                                           uint32_t *png_status, uint64_t n, uint32_t row_bytes,
                                           uint32_t bpp, void *hip_stream);
int fdh_inflate_png_batch(const uint8_t *in, const uint64_t *in_off, uint8_t *filt,
                          const uint64_t *filt_off, uint32_t *out_len, uint32_t *status,
                          uint32_t *adler, uint8_t *pix, const uint64_t *pix_off,
                          uint32_t *png_status, uint64_t n, uint32_t flags, uint32_t row_bytes,
                          uint32_t bpp, void *hip_stream);

/* ---- PNG files: CRC-32, the framing around an IDAT stream, the container scan ----------------
 * Not in the fdeflate crate either (image-rs/image-png frames and parses the container); the format is the
 * PNG specification's (5.2 signature, 5.3 chunk layout, 5.5 and annex D CRC, 11.2.2 IHDR, 5.6 ordering).
 * With these the encoders' output becomes files, and files become the decoder's input, with no host work
 * in between: nothing here allocates, synchronises or reads anything back. */

/*
 * fdh_crc32_batch -- CRC-32 as in PNG / zlib (polynomial 0xEDB88320, reflected, preset and result
 * complemented) of `n` byte ranges: crc[i] = crc32(range i, seed[i]) in zlib's sense.
 *   data, off[n+1]  range i = data[off[i] .. off[i] + L_i), L_i = len ? len[i] : off[i+1] - off[i]; any alignment
 *   len[n]          nullable; the device-resident out_len an encoder wrote, so that its output is summed
 *                   with no round trip to the host
 *   seed[n]         nullable (= 0); the CRC of the bytes that came before (a chunk's type and its body can be
 *                   two ranges)
 *   status[n]       0 ok; 2 len[i] exceeds the slot off[i+1] - off[i], len[i] == 0xFFFFFFFF (the encoders'
 *                   "slot too small"), or the slot is 4 GiB or more: crc[i] = 0
 * A range of no bytes returns its seed.  Parallel inside a range as well as across ranges: a batch of
 * fewer than 4096 ranges gives each several wavefronts (one 256 MiB range is an ordinary input), and the
 * 64 lanes of a wavefront always share its bytes.  No byte of `data` is written.
 */
int fdh_crc32_batch(const uint8_t *data, const uint64_t *off, const uint32_t *len,
                    const uint32_t *seed, uint32_t *crc, uint32_t *status, uint64_t n,
                    void *hip_stream);

/*
 * fdh_png_frame_batch -- makes PNG files of zlib streams that are already in place: one IDAT chunk each.
 * Precondition: the stream of image i lies at file[file_off[i] + FDH_PNG_FILE_PREFIX ..), idat_len[i] bytes
 * long -- put there by any of the encoders above, called with the offsets shifted by FDH_PNG_FILE_PREFIX
 * (with idat_len their out_len).  Nothing is copied.  The call writes the 41 bytes in front (signature 8,
 * IHDR chunk 25 -- width, height[i], bit_depth, colour_type, 0, 0, 0 and its CRC --, the IDAT's length and
 * type 8) and the 16 bytes behind (the IDAT's CRC over "IDAT" and the stream 4, IEND chunk 12), and sets
 * file_len[i] = idat_len[i] + 57.
 * png_status[i]: 0 ok; 2 -- nothing written, file_len[i] = 0 -- when idat_len[i] is 0 or 0xFFFFFFFF (the
 * image was skipped or overflowed its slot upstream) or above 2^31-1, idat_len[i] + 57 exceeds the slot
 * file_off[i+1] - file_off[i], or height[i] is 0 or above 2^31-1.  width 0 or above 2^31-1, or a depth /
 * colour-type pair that is not one of the specification's fifteen: FDH_ERR_INVALID_ARGUMENT.
 * Bytes outside a slot are never written; those of the slot behind file_len[i] are not specified.
 * fdh_png_file_bound(rows, row_bytes) = fdh_ultrafast_bound(rows * (row_bytes + 1)) + 57: a slot that
 * always suffices for the ultra-fast encoder's file.
 */
#define FDH_PNG_FILE_PREFIX 41u
#define FDH_PNG_FILE_SUFFIX 16u
uint64_t fdh_png_file_bound(uint64_t rows, uint64_t row_bytes);
int fdh_png_frame_batch(uint8_t *file, const uint64_t *file_off, const uint32_t *idat_len,
                        const uint32_t *height, uint32_t *file_len, uint32_t *png_status,
                        uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type,
                        void *hip_stream);

/*
 * fdh_png_scan_files_batch -- walks the chunks of `n` PNG files (one lane per file) and then verifies the
 * CRC of EVERY chunk, ancillary ones included, with the kernel of fdh_crc32_batch (one wavefront per
 * file, sixteen for a batch of fewer than 4096).  File i = file[file_off[i] .. + file_len[i]); file_len
 * nullable (= the whole slot; a length above the slot counts as the slot).  Bytes behind IEND are ignored.
 * info[i].status is the first structural finding in file order, and 6 only if there is none:
 *   0 ok
 *   1 no PNG signature
 *   2 truncated: a chunk runs past the end of the file, or there is no IEND
 *   3 bad IHDR: not the first chunk, length not 13, a zero dimension (or one above 2^31-1), an illegal
 *     depth / colour pair, compression or filter method not 0 (or an interlace method above 1)
 *   4 interlace method 1, unless FDH_PNG_FLAG_ADAM7 is set
 *   5 chunk structure: no IDAT, IDAT chunks not consecutive, a PLTE after IDAT, an unknown critical chunk
 *   6 CRC mismatch in some chunk
 * The walk ends at the first finding; the counts then hold what came before it.  first_idat is the offset
 * of the first IDAT chunk (its length field) in the file, chunks counts IHDR .. IEND.
 * FDH_PNG_FLAG_IGNORE_CRC skips the CRC pass (as FDH_FLAG_IGNORE_ADLER32 skips that check).
 * FDH_PNG_FLAG_ADAM7: an IHDR with interlace method 1 is no finding -- the walk goes on to IEND, every count is
 * filled in, the CRC pass runs, and info.interlace is 1 (fdh_png_unfilter_interlaced_batch below takes such a
 * file's decoded IDAT stream to pixels).  Without the flag such a file is status 4 and the walk ends at IHDR; a
 * method above 1 is status 3 either way.
 *
 * fdh_png_gather_idat_batch -- copies the IDAT bodies of file i, in order, to comp[comp_off[i] ..) as one
 * zlib stream (what fdh_inflate_png_batch takes) and sets comp_len[i] = info[i].idat_bytes; 16 bytes per
 * lane and step wherever the destination's alignment allows.
 * png_status[i]: 0 ok; 3 info[i].status != 0 (skipped, as above); 7 the file's width, depth or colour type
 * is not the call's; 8 the slot comp_off[i+1] - comp_off[i] is too small.  Where it is not 0, comp_len[i] = 0
 * and nothing is written.  Geometry arguments as for fdh_png_frame_batch.
 * Neither the gather nor fdh_png_colour_batch looks at info.interlace: the chunks around the pixels are the same
 * in both layouts, and both calls serve interlaced files as they are.
 */
#define FDH_PNG_FLAG_IGNORE_CRC 0x1u
#define FDH_PNG_FLAG_ADAM7 0x2u
/* info.status of the scan, 1 .. 6 in the order of the list above */
#define FDH_PNG_STATUS_SCAN_NO_SIGNATURE 1u
#define FDH_PNG_STATUS_SCAN_TRUNCATED 2u
#define FDH_PNG_STATUS_SCAN_BAD_IHDR 3u
#define FDH_PNG_STATUS_SCAN_INTERLACED 4u
#define FDH_PNG_STATUS_SCAN_CHUNK_STRUCTURE 5u
#define FDH_PNG_STATUS_SCAN_CRC_MISMATCH 6u
/* png_status of the gather (and 7 of fdh_png_colour_batch) */
#define FDH_PNG_STATUS_OTHER_GEOMETRY 7u
#define FDH_PNG_STATUS_COMP_SLOT_TOO_SMALL 8u
typedef struct fdh_png_info {
  uint32_t status, width, height;
  uint8_t bit_depth, colour_type, interlace, pad;
  uint32_t idat_bytes, idat_chunks, first_idat, chunks;
} fdh_png_info; /* 32 bytes */
int fdh_png_scan_files_batch(const uint8_t *file, const uint64_t *file_off,
                             const uint32_t *file_len, fdh_png_info *info, uint64_t n,
                             uint32_t flags, void *hip_stream);
int fdh_png_gather_idat_batch(const uint8_t *file, const uint64_t *file_off,
                              const fdh_png_info *info, uint8_t *comp, const uint64_t *comp_off,
                              uint32_t *comp_len, uint32_t *png_status, uint64_t n, uint32_t width,
                              uint32_t bit_depth, uint32_t colour_type, void *hip_stream);

/* ---- PNG decode to RGBA8: PLTE and tRNS, sample expansion --------------------------------------
 * image-png's Transformations::EXPAND | STRIP_16 | ALPHA, not the fdeflate crate's ground: the packed
 * scanlines that fdh_inflate_png_batch leaves become [rows, width, 4] uint8 pictures, R, G, B, A.  Samples
 * are unpacked as the PNG specification says (7.2: most significant bits first, 16-bit samples big-endian;
 * padding bits behind a row's last pixel are ignored) and brought to eight bits by to8(s) = s >> 8 at depth
 * 16, s at depth 8, s * 255, s * 85, s * 17 at depths 1, 2, 4.  No gamma.
 *   colour type 0  R = G = B = to8(g); A = 0 if a key is present and the RAW sample equals key & (2^depth - 1),
 *                  else 255
 *   colour type 2  to8 of each sample; A = 0 if a key is present and all three raw samples equal the key's
 *                  three values (each masked to the depth; all 16 bits at depth 16), else 255
 *   colour type 3  PLTE entry idx; A = tRNS byte idx where the chunk has one, else 255
 *   colour type 4  R = G = B = to8(g), A = to8(a)
 *   colour type 6  to8 of each sample
 * A palette index at or above the number of PLTE entries gives (0, 0, 0, 255) and status 9.
 *
 * fdh_png_colour_batch -- reads PLTE and tRNS of file i out of the chunks between IHDR and info[i].first_idat
 * (the scan has verified their CRCs; one wavefront per file).  info as fdh_png_scan_files_batch wrote it; width,
 * bit_depth, colour_type as for fdh_png_gather_idat_batch.
 *   pal[256 n]    per file 256 words R | G << 8 | B << 16 | A << 24: entries behind the PLTE's count are
 *                 0xFF000000, A is 255 where tRNS is shorter.  Nullable unless colour_type is 3 (then not written).
 *   colour[4 n]   word 0 the PLTE entry count (0 for other colour types); word 1 bit 0: a key is present;
 *                 word 2 the key's R or grey | G << 16, word 3 its B (the 16-bit values of the chunk)
 * png_status[i] -- the first finding in file order:
 *   0  ok
 *   3  info[i].status != 0 (or info does not describe the file)
 *   7  the file's width, depth or colour type is not the call's
 *   10 PLTE (colour type 3 only): none in front of IDAT; a length of 0, not a multiple of 3, above 768; a second one
 *   11 tRNS: its length is not 2 (colour type 0) or 6 (colour type 2); for colour type 3 more bytes than PLTE has
 *      entries, or in front of PLTE; a second tRNS (colour types 0, 2, 3)
 * A tRNS in a file of colour type 4 or 6 is ignored (as libpng does), and so is a PLTE in a file of another
 * colour type than 3.  Where png_status[i] != 0, pal and colour of file i are not specified.
 *
 * fdh_png_expand_batch -- image i = pix[pix_off[i] .. pix_off[i+1]), whole packed rows of the geometry's
 * row_bytes at any alignment, to the slot rgba[rgba_off[i] .. rgba_off[i+1]) of exactly rows * width * 4 bytes.
 *   pal       as above; nullable unless colour_type is 3
 *   colour    as above; null: no key anywhere, and every palette index counts as inside the palette
 *   upstream  nullable; where upstream[i] != 0 the image is skipped and png_status[i] = upstream[i] (earlier
 *             failures pass through without a read-back)
 * png_status[i]:
 *   0 ok (an empty pixel slot with an empty output slot as well: nothing is written)
 *   2 the pixel slot is not whole rows, or the output slot is not exactly the image's size: nothing is written
 *   9 a palette index at or above the PLTE's count; the image is written in full
 * An illegal depth / colour pair or width: FDH_ERR_INVALID_ARGUMENT.  No byte outside a slot is written and no
 * byte outside pix[pix_off[0] .. pix_off[n]) is read.  FDH_PNG_EXPAND_WAVES (environment) sets the number of
 * wavefronts per image.
 */
#define FDH_PNG_STATUS_INDEX_OUTSIDE_PALETTE 9u
#define FDH_PNG_STATUS_BAD_PLTE 10u
#define FDH_PNG_STATUS_BAD_TRNS 11u
int fdh_png_colour_batch(const uint8_t *file, const uint64_t *file_off, const fdh_png_info *info,
                         uint32_t *pal, uint32_t *colour, uint32_t *png_status, uint64_t n,
                         uint32_t width, uint32_t bit_depth, uint32_t colour_type, void *hip_stream);
int fdh_png_expand_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *rgba,
                         const uint64_t *rgba_off, const uint32_t *pal, const uint32_t *colour,
                         const uint32_t *upstream, uint32_t *png_status, uint64_t n, uint32_t width,
                         uint32_t bit_depth, uint32_t colour_type, void *hip_stream);

/* ---- PNG decode: Adam7 interlaced images ---------------------------------------------------------
 * image-png's interlace handling, not the fdeflate crate's ground.  PNG specification 8.2: the IDAT stream of a
 * file with interlace method 1 holds seven reduced images ("passes") one behind the other, pass p = 0 .. 6 with
 *   x0 = 0, 4, 0, 2, 0, 1, 0    y0 = 0, 0, 4, 0, 2, 0, 1    dx = 8, 8, 4, 4, 2, 2, 1    dy = 8, 8, 8, 4, 4, 2, 2
 * pw = ceil((width - x0) / dx) pixels wide and ph = ceil((height - y0) / dy) rows high (0 where negative).  A pass
 * with pw = 0 or ph = 0 has no bytes at all; any other is ph rows of 1 + ceil(pw * bits / 8) bytes, filtered as an
 * image of its own: the row above its first row is zeros, and the pixel size of the filters is the full image's,
 * max(1, channels * depth / 8).  Pixel j of row r of pass p is pixel (x0 + j dx, y0 + r dy) of the picture; at
 * depths 1, 2 and 4 pixels are bit fields, most significant first, in both layouts.
 *
 * fdh_png_adam7_size -- the number of bytes the IDAT stream of an interlaced width x height image decodes to
 * (the sum over the passes); 0 for an illegal depth / colour pair or a zero dimension.  Host arithmetic, no device.
 * It can equal the progressive size height * (1 + row_bytes) (1 x 9 grey-8: 18 both ways), so the size never tells
 * the two layouts apart.
 *
 * fdh_png_unfilter_interlaced_batch -- image i = filt[filt_off[i] .. filt_off[i+1]), what the zlib decoder left,
 * goes to packed scanlines in pix[pix_off[i] .. pix_off[i+1]): the layout fdh_png_unfilter_batch produces and
 * fdh_png_expand_batch reads (height_i = slot / row_bytes rows of row_bytes, samples as PNG packs them, padding
 * bits of a row zero: those of an Adam7 image's pass rows are dropped, whatever they hold; a progressive image
 * keeps its own as they come, as with fdh_png_unfilter_batch).  width, bit_depth, colour_type as for
 * fdh_png_expand_batch.
 *   method        a byte per image: 0 progressive, 1 Adam7; null = all Adam7.  A progressive image is the same
 *                 machinery with one pass (x0 = y0 = 0, dx = dy = 1) and gives exactly fdh_png_unfilter_batch's
 *                 bytes, so a batch may mix both kinds (info[i].interlace, byte 14 of a record, is such a byte).
 *   upstream, upstream_len   nullable: the decoder's status and out_len (the gate of fdh_inflate_png_batch)
 * `filt` is NOT const: the images are reconstructed in place, and the contents of the filt slots afterwards are
 * not specified.
 * png_status[i]:
 *   0 ok (two empty slots: nothing is written)
 *   1 a filter type above 4 in some pass row; the contents of the pix slot are not specified
 *   2 the pix slot is not whole rows; or the filt slot is not exactly fdh_png_adam7_size (method 1) or
 *     height * (row_bytes + 1) (method 0); or upstream_len[i] is not the filt slot's size; or a method byte
 *     above 1: nothing is written
 *   3 upstream[i] is not 0: nothing is written
 * No byte outside a pix slot is written, no byte outside filt[filt_off[0] .. filt_off[n]) is read.  No workspace,
 * no host synchronisation, any alignment.  An illegal pair or width: FDH_ERR_INVALID_ARGUMENT.
 * FDH_PNG_ADAM7_WAVES (environment) sets the number of placement wavefronts per image.
 */
uint64_t fdh_png_adam7_size(uint32_t width, uint32_t height, uint32_t bit_depth, uint32_t colour_type);
int fdh_png_unfilter_interlaced_batch(uint8_t *filt, const uint64_t *filt_off, uint8_t *pix,
                                      const uint64_t *pix_off, const uint8_t *method,
                                      const uint32_t *upstream, const uint32_t *upstream_len,
                                      uint32_t *png_status, uint64_t n, uint32_t width,
                                      uint32_t bit_depth, uint32_t colour_type, void *hip_stream);

/* ---- PNG decode: mixed batches ----------------------------------------------------------------------
 * The decode steps above take width, bit_depth and colour_type as arguments of the call: one geometry per batch.
 * The calls of this section take them per image from info[i], so one batch can hold files of any width, height,
 * depth, colour type and interlace method.  The records may be fdh_png_scan_files_batch's or the caller's own, so
 * every call checks them itself.  A record is DECODABLE when status == 0, width and height are 1 .. 2^31-1, the
 * depth / colour pair is one of the fifteen and interlace <= 1; a record that is not gives png_status 3 and
 * nothing is written for that image.  No new status value: 0, 1, 2, 3, 8, 9, 10, 11 mean what they mean above, and
 * 7 (another geometry than the call's) does not occur.
 * All calls enqueue on hip_stream and return: no allocation, no synchronisation, nothing outside a slot written,
 * nothing outside [off[0], off[n]) read, n == 0 is success, more than 2^31-1 images FDH_ERR_INVALID_ARGUMENT.
 *   upstream  (every call but the plan) nullable; where upstream[i] != 0 the image is skipped and png_status[i] =
 *             upstream[i], as with fdh_png_expand_batch.  The exception is fdh_png_unfilter_mixed_batch, whose
 *             upstream is the zlib decoder's status as in fdh_png_unfilter_interlaced_batch: it gives 3.
 *
 * fdh_png_plan_sizes / fdh_png_plan_batch -- what a pipeline has to allocate for an image, on the host for one
 * record (plain arithmetic, no device) and on the device for n (one record per lane).  The four sizes, sizes[0 .. 3]
 * or the four arrays of n (each nullable):
 *   compressed  info.idat_bytes
 *   filtered    what the IDAT stream decodes to: height * (1 + row_bytes), or fdh_png_adam7_size for interlace 1
 *   packed      height * row_bytes                       (row_bytes = ceil(width * channels * depth / 8))
 *   RGBA8       height * width * 4
 * status (the return value, or png_status[i]): 0 ok; 3 the record is not decodable (or rec is null); 2 the filtered
 * size is 2^32 or more -- more than a slot of fdh_inflate_batch can hold --, or max_bytes != 0 and the largest of the
 * four sizes exceeds it.  Where it is not 0 all four sizes are 0: a 40-byte file may declare 2^31-1 by 2^31-1
 * pixels, and a pipeline that sums the sizes allocates nothing for it.  The arithmetic does not wrap.
 *
 * fdh_png_gather_idat_mixed_batch -- fdh_png_gather_idat_batch without the comparison of geometries.
 * png_status[i]: 0 ok; 3 not decodable, or info does not describe the file; 8 the comp slot is too small; or upstream.
 * Where it is not 0, comp_len[i] = 0 and nothing is written.
 *
 * fdh_png_colour_mixed_batch -- fdh_png_colour_batch with the colour type and depth of info[i].  pal[256 n] is
 * required; the 256 words of file i are written only if its colour type is 3, the rows of other files are left as
 * they are.  colour[4 n] is written for every file whose png_status is 0.
 * png_status[i]: 0 ok; 3 not decodable, or info does not describe the file; 10, 11 as there; or upstream.
 *
 * fdh_png_unfilter_mixed_batch -- fdh_png_unfilter_interlaced_batch at image i's own width, depth and colour type,
 * with method = info[i].interlace.  The pix slot and png_status[i] are byte for byte what that call gives for the
 * image alone, the rules about padding bits and upstream_len included; `filt` is reconstructed in place as there.
 * The slots must be exactly the plan's filtered and packed sizes for the record (so the height is info[i].height,
 * not the slot's), else 2.
 * png_status[i]: 0 ok; 1 a filter type above 4; 2 a slot or upstream_len[i] does not fit, or the filtered size is
 * 2^32 or more; 3 not decodable, or upstream[i] != 0.  Where it is 2 or 3 nothing is written.
 *
 * fdh_png_expand_mixed_batch -- fdh_png_expand_batch at image i's own geometry: the RGBA slot and png_status[i]
 * (0, 2, 9) are byte for byte what that call gives for the image alone (the number of rows is the pix slot's, as
 * there).  pal may be null only if no decodable image has colour type 3: such an image gets status 10 then.
 * colour: nullable, with the meaning it has there.  png_status[i] otherwise: 3 not decodable; or upstream.
 *
 * One wavefront per image and step as in the calls these derive from; FDH_PNG_ADAM7_WAVES and
 * FDH_PNG_EXPAND_WAVES apply.
 */
uint32_t fdh_png_plan_sizes(const fdh_png_info *rec, uint64_t max_bytes, uint64_t sizes[4]);
int fdh_png_plan_batch(const fdh_png_info *info, uint64_t max_bytes, uint64_t *comp_size,
                       uint64_t *filt_size, uint64_t *pix_size, uint64_t *rgba_size,
                       uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_gather_idat_mixed_batch(const uint8_t *file, const uint64_t *file_off,
                                    const fdh_png_info *info, const uint32_t *upstream, uint8_t *comp,
                                    const uint64_t *comp_off, uint32_t *comp_len, uint32_t *png_status,
                                    uint64_t n, void *hip_stream);
int fdh_png_colour_mixed_batch(const uint8_t *file, const uint64_t *file_off, const fdh_png_info *info,
                               const uint32_t *upstream, uint32_t *pal, uint32_t *colour,
                               uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_unfilter_mixed_batch(uint8_t *filt, const uint64_t *filt_off, uint8_t *pix,
                                 const uint64_t *pix_off, const fdh_png_info *info,
                                 const uint32_t *upstream, const uint32_t *upstream_len,
                                 uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_expand_mixed_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *rgba,
                               const uint64_t *rgba_off, const fdh_png_info *info, const uint32_t *pal,
                               const uint32_t *colour, const uint32_t *upstream, uint32_t *png_status,
                               uint64_t n, void *hip_stream);

/* ---- PNG encode from RGBA8: analysis, packing, palette files ----------------------------------------
 * The encode side's counterpart of the section "PNG decode to RGBA8": [rows, width, 4] uint8 pictures, R, G, B, A,
 * become packed scanlines of a depth / colour pair (what fdh_png_choose_filters_batch and
 * fdh_png_filter_deflate_ultrafast_batch take), and a palette file gets its PLTE and tRNS.  Nothing is read back.
 *
 * fdh_png_analyse_batch -- what image i = rgba[rgba_off[i] .. rgba_off[i+1]) is: whole rows of width * 4 bytes at
 * any alignment.  max_colours is 1 .. 256.
 *   pal[256 n]    the image's distinct pixels as words R | G << 8 | B << 16 | A << 24 (the layout of
 *                 fdh_png_colour_batch) in ASCENDING order as unsigned 32-bit integers.  A is the most significant
 *                 byte, so every entry with A < 255 sits in front of every opaque one and a tRNS chunk can end behind
 *                 the last of them; and the order makes the result independent of launch shape and scheduling.
 *                 Entries behind the count are 0xFF000000.  Nullable: then only the other outputs are produced.
 *   colour[4 n]   word 0 the number of distinct pixels, words 1 .. 3 zero: what fdh_png_expand_batch takes
 *   trns_len[n]   the number of entries with A < 255
 *   summary[n]    bit 0: every A is 255; bit 1: every pixel has R == G == B; bits 8 .. 15: the smallest d of 1, 2, 4,
 *                 8 such that every R, G and B is a multiple of 255 / (2^d - 1), the grey / RGB sample depth that
 *                 loses nothing.  Always over the whole image, also when the colours overflow.  An image of no rows:
 *                 status 0, no colours, bits 0 and 1 set, depth 1.
 * png_status[i]: 0 ok; 2 the slot is not whole rows: nothing is written for that image; 12 more than max_colours
 * distinct pixels: summary[i] is valid, pal, colour and trns_len of the image are not specified.
 * One workgroup per image with the set in an LDS hash table; FDH_PNG_ANALYSE_WAVES (environment) sets its wavefronts,
 * 1 .. 16, and the result is the same at every setting.  No workspace, no host synchronisation.  width 0 or above
 * 2^31-1, or max_colours outside 1 .. 256: FDH_ERR_INVALID_ARGUMENT.
 *
 * fdh_png_pack_batch -- the exact inverse of fdh_png_expand_batch: image i to the slot pix[pix_off[i] ..
 * pix_off[i+1]) of exactly rows * row_bytes bytes.  Samples are packed as PNG packs them (most significant bits
 * first, 16-bit samples big-endian); the padding bits of a row are zero.
 *   colour type 6  depth 8 copies; depth 16 writes each sample s as the bytes s, s (s * 257: to8 gives s back)
 *   colour type 2  the same without A; needs every A == 255
 *   colour type 4  R and A; needs R == G == B
 *   colour type 0  needs both; below depth 8, R must be a multiple of 255 / (2^depth - 1): the sample is the quotient
 *   colour type 3  the index is the lowest k < count with pal[k] equal to the pixel word, count = colour[4 i]
 *                  (256 where colour is null, and at most 256); it must be below 2^depth.  pal is required; it need
 *                  not be sorted or free of duplicates.
 * Colour keys (tRNS with colour types 0 and 2) are not produced: colour words 1 .. 3 are ignored.
 *   upstream  nullable; where upstream[i] != 0 the image is skipped and png_status[i] = upstream[i]
 * png_status[i]:
 *   0  ok: fdh_png_expand_batch of the pix slot, with the same pal / colour, gives the image back byte for byte
 *   2  the RGBA slot is not whole rows, or the pix slot is not exactly rows * row_bytes: nothing is written
 *   13 some pixel has no lossless representation in the pair; the contents of the pix slot are not specified
 * No byte outside a pix slot is written, no byte outside rgba[rgba_off[0] .. rgba_off[n]) is read.  An illegal pair
 * or width: FDH_ERR_INVALID_ARGUMENT.  FDH_PNG_PACK_WAVES (environment) sets the number of wavefronts per image.
 *
 * fdh_png_palette_file_prefix / fdh_png_frame_palette_batch -- fdh_png_frame_batch for colour type 3, where a file
 * needs a PLTE: again the zlib stream of image i is already in place, now at file_off[i] + prefix with
 *   prefix = 41 + 12 + 3 E + (T ? 12 + T : 0),   E = plte_entries in 1 .. min(256, 2^bit_depth),  T = trns_entries in 0 .. E
 * the same for every file of the call, so that the encoders' single offsets array still serves (the function returns 0
 * for an E outside 1 .. 256 or a T above E).  The prefix holds, in order: signature, IHDR, a PLTE of E entries -- the
 * colour[4 i] entries of pal[256 i ..], then 0, 0, 0 --, where T > 0 a tRNS of T bytes -- the alphas of those entries,
 * then 255 --, and the IDAT's length and type; the 16 bytes behind the stream are fdh_png_frame_batch's.  Every
 * chunk's CRC is computed on the device.  file_len[i] = idat_len[i] + prefix + 16.  Unused palette entries and a tRNS
 * shorter than the PLTE are both legal PNG.
 * png_status[i] -- nothing is written and file_len[i] = 0 unless it is 0; the first that applies:
 *   2  fdh_png_frame_batch's conditions (with this prefix)
 *   10 colour[4 i] is 0 or above E
 *   11 trns_len[i] is above T
 * An illegal width or depth, E or T: FDH_ERR_INVALID_ARGUMENT.
 */
#define FDH_PNG_STATUS_TOO_MANY_COLOURS 12u  /* fdh_png_analyse_batch */
#define FDH_PNG_STATUS_NOT_REPRESENTABLE 13u /* fdh_png_pack_batch */
int fdh_png_analyse_batch(const uint8_t *rgba, const uint64_t *rgba_off, uint32_t *pal,
                          uint32_t *colour, uint32_t *trns_len, uint32_t *summary,
                          uint32_t *png_status, uint64_t n, uint32_t width, uint32_t max_colours,
                          void *hip_stream);
int fdh_png_pack_batch(const uint8_t *rgba, const uint64_t *rgba_off, uint8_t *pix,
                       const uint64_t *pix_off, const uint32_t *pal, const uint32_t *colour,
                       const uint32_t *upstream, uint32_t *png_status, uint64_t n, uint32_t width,
                       uint32_t bit_depth, uint32_t colour_type, void *hip_stream);
uint64_t fdh_png_palette_file_prefix(uint32_t plte_entries, uint32_t trns_entries);
int fdh_png_frame_palette_batch(uint8_t *file, const uint64_t *file_off, const uint32_t *idat_len,
                                const uint32_t *height, const uint32_t *pal, const uint32_t *colour,
                                const uint32_t *trns_len, uint32_t *file_len, uint32_t *png_status,
                                uint64_t n, uint32_t width, uint32_t bit_depth,
                                uint32_t plte_entries, uint32_t trns_entries, void *hip_stream);

/* ---- PNG encode: mixed batches ----------------------------------------------------------------------
 * The encode steps above take width, bit_depth and colour_type as arguments of the call: one geometry per batch.
 * The calls of this section take them per image from info[i], the record of "PNG decode: mixed batches", of which
 * they read status, width, height, bit_depth, colour_type and interlace: one batch can hold pictures of any width,
 * height, depth and colour type, and the calls of that section give the pictures back from what these write.  A record is
 * ENCODABLE when status == 0, width and height are 1 .. 2^31-1, the depth / colour pair is one of the fifteen and
 * interlace == 0 (interlaced files are not written); a DIMENSION record is the same with bit_depth == 0 and
 * colour_type == 0, which means "choose for me": fdh_png_analyse_mixed_batch and the plan take it, the plan turns it
 * into an encodable one.  A record that is neither gives png_status 3 and nothing is written for that image.  No new
 * status value: 0, 1, 2, 3, 10, 11, 12, 13 mean what they mean above.
 * All _batch calls take device pointers, enqueue on hip_stream and return: no allocation, no synchronisation, nothing
 * outside a slot written, nothing outside [off[0], off[n]) read, n == 0 is success, more than 2^31-1 images
 * FDH_ERR_INVALID_ARGUMENT.
 *   upstream  (analyse, pack, choose, fused encoder) nullable; where upstream[i] != 0 the image is skipped and
 *             png_status[i] = upstream[i]
 * The geometry limits of the encode steps are the plan's: row_bytes below 2^25 (fdh_png_choose_filters_batch's) and
 * height * (row_bytes + 1) below 2^31 (the fused encoder's); pack, choose and the fused encoder give 2 for an
 * encodable record beyond them.
 *
 * fdh_png_analyse_mixed_batch -- fdh_png_analyse_batch at info[i].width; the record may be a dimension record or an
 * encodable one.  The slot must be exactly height * width * 4 bytes, else 2.  pal, colour, trns_len, summary and
 * the statuses 0 / 2 / 12 are byte for byte those of the per-width call on the image alone; the palette comes out
 * sorted and FDH_PNG_ANALYSE_WAVES applies.  png_status[i] otherwise: 3 neither kind of record; or upstream.
 *
 * fdh_png_encode_plan_one / fdh_png_encode_plan_batch -- which pair a picture is written with and what a pipeline
 * has to allocate for it, on the host for one record (plain arithmetic, no device) and on the device for n (one
 * record per lane).  colour_count / trns_len point to one word each on the host; colour[4 n] (word 0 the count) /
 * trns_len[n], summary[n] and analyse_status[n] are fdh_png_analyse_mixed_batch's outputs, each nullable: without
 * colour or trns_len there is no palette; a missing summary counts as 0; a missing analyse_status as 12 for a
 * dimension record and 0 for an encodable one.
 * For a dimension record the pair is chosen and written into the record (only where the status is 0).  Candidates:
 *   grey        (0, d)  summary bits 0 and 1 set; d the summary's depth
 *   palette     (3, p)  analyse_status 0, count = colour[4 i] in 1 .. 256 and trns_len[i] <= count; p the smallest of
 *                       1, 2, 4, 8 with 2^p >= count
 *   grey-alpha  (4, 8)  bit 1 set
 *   RGB         (2, 8)  bit 0 set
 *   RGBA        (6, 8)  always
 * A candidate is dropped where bit colour_type of `allowed` is clear; allowed == 0 means all five (other bits:
 * FDH_ERR_INVALID_ARGUMENT from the batch call, ignored by the host call).  The cost of a candidate is height *
 * row_bytes, for the palette plus 12 + 3 count + (trns_len ? 12 + trns_len : 0), its chunks; the smallest cost wins,
 * the lower colour type on equal cost.  For an encodable record the pair is kept.
 * The sizes, sizes[0 .. 3] or the four arrays of n (each nullable, as is png_status):
 *   packed      height * row_bytes
 *   types       height
 *   prefix      41, or for colour type 3  41 + 12 + 3 count + (trns_len ? 12 + trns_len : 0): the EXACT palette, no
 *               padding entries
 *   file        prefix + fdh_ultrafast_bound(height * (row_bytes + 1)) + 16: a slot that always suffices
 * status (the return value, or png_status[i]), the first that applies: 3 neither kind of record (or rec is null);
 * analyse_status where it is neither 0 nor 12; 13 no candidate is left; for an encodable record of colour type 3,
 * 10 without colour / trns_len or with a count outside 1 .. 2^depth, 11 trns_len above the count; 2 row_bytes is 2^25
 * or more, or height * (row_bytes + 1) is 2^31 or more.  Where it is not 0 all four sizes are 0.  Nothing wraps.
 *
 * fdh_png_pack_mixed_batch -- fdh_png_pack_batch at image i's own pair and width.  The slots must be exactly the
 * plan's sizes (height * width * 4 and height * row_bytes), else 2.  pal may be null only if no encodable image has
 * colour type 3: such an image gets status 10 then.  The pix slot and the statuses 0 / 13 are byte for byte what
 * that call gives for the image alone.  png_status[i] otherwise: 3 not encodable; or upstream.
 *
 * fdh_png_choose_filters_mixed_batch -- fdh_png_choose_filters_batch at image i's own row_bytes and bpp: the same
 * types.  The slots must be exactly the plan's packed size and height bytes, else 2.  png_status[i] otherwise: 0;
 * 3 not encodable; or upstream.  FDH_PNG_CHOOSE_LANES and FDH_PNG_CHOOSE_WAVES apply.
 *
 * fdh_png_filter_deflate_ultrafast_mixed_batch -- fdh_png_filter_deflate_ultrafast_batch at image i's own
 * row_bytes and bpp: the same stream and out_len (0xFFFFFFFF where the out slot is too small).  pix and types
 * slots exactly the plan's, else 2.  png_status[i]: 0; 1 a filter type above 4; 2; 3 not encodable; or upstream.
 * Where it is not 0, out_len[i] = 0 and nothing is written.
 *
 * fdh_png_frame_mixed_batch -- fdh_png_frame_batch / fdh_png_frame_palette_batch with the IHDR of info[i] and, for
 * colour type 3, a PLTE of exactly colour[4 i] entries and, where trns_len[i] > 0, a tRNS of exactly trns_len[i]
 * bytes.  The zlib stream of image i is already in place at file_off[i] + prefix_i, the plan's prefix.  Every
 * chunk's CRC is computed on the device.  file_len[i] = idat_len[i] + prefix_i + 16.  pal, colour and trns_len
 * may be null only if no encodable image has colour type 3.
 * png_status[i] -- nothing is written and file_len[i] = 0 unless it is 0; the first that applies: 3 not encodable;
 * 2 fdh_png_frame_batch's conditions with this prefix (a palette that is refused counts with one entry); 10
 * colour[4 i] is 0 or above 2^depth, or the arrays are missing; 11 trns_len[i] is above the count.
 */
uint32_t fdh_png_encode_plan_one(fdh_png_info *rec /* in, out */, const uint32_t *colour_count,
                                 const uint32_t *trns_len, uint32_t summary, uint32_t analyse_status,
                                 uint32_t allowed, uint64_t sizes[4]);
int fdh_png_encode_plan_batch(fdh_png_info *info /* in, out */, const uint32_t *colour,
                              const uint32_t *trns_len, const uint32_t *summary,
                              const uint32_t *analyse_status, uint32_t allowed, uint64_t *pix_size,
                              uint64_t *types_size, uint64_t *prefix, uint64_t *file_size,
                              uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_analyse_mixed_batch(const uint8_t *rgba, const uint64_t *rgba_off, const fdh_png_info *info,
                                const uint32_t *upstream, uint32_t *pal, uint32_t *colour,
                                uint32_t *trns_len, uint32_t *summary, uint32_t *png_status, uint64_t n,
                                uint32_t max_colours, void *hip_stream);
int fdh_png_pack_mixed_batch(const uint8_t *rgba, const uint64_t *rgba_off, uint8_t *pix,
                             const uint64_t *pix_off, const fdh_png_info *info, const uint32_t *pal,
                             const uint32_t *colour, const uint32_t *upstream, uint32_t *png_status,
                             uint64_t n, void *hip_stream);
int fdh_png_choose_filters_mixed_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *types,
                                       const uint64_t *types_off, const fdh_png_info *info,
                                       const uint32_t *upstream, uint32_t *png_status, uint64_t n,
                                       void *hip_stream);
int fdh_png_filter_deflate_ultrafast_mixed_batch(const uint8_t *pix, const uint64_t *pix_off,
                                                 const uint8_t *types, const uint64_t *types_off,
                                                 uint8_t *out, const uint64_t *out_off, uint32_t *out_len,
                                                 const fdh_png_info *info, const uint32_t *upstream,
                                                 uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_frame_mixed_batch(uint8_t *file, const uint64_t *file_off, const uint32_t *idat_len,
                              const fdh_png_info *info, const uint32_t *pal, const uint32_t *colour,
                              const uint32_t *trns_len, uint32_t *file_len, uint32_t *png_status,
                              uint64_t n, void *hip_stream);

/* ---- streaming decoder: `Decompressor` (src/decompress.rs:96-156, 179-342) ----------------
 * A host-side object with exactly `Decompressor::read`'s contract on HOST buffers; every bit of
 * decoding is done by fdh_inflate_batch_resumable on the device (the object keeps a device-resident
 * copy of the stream so far, a device output slot and the resume point of its last attempt: an attempt
 * decodes what is new; see csrc/stream_decompressor.cpp).
 *
 *   fdh_decompressor_new            Decompressor::new()            src/decompress.rs:123
 *   fdh_decompressor_ignore_adler32 Decompressor::ignore_adler32() src/decompress.rs:154
 *   fdh_decompressor_is_done        Decompressor::is_done()        src/decompress.rs:340
 *   fdh_decompressor_read           Decompressor::read(input, output, output_position)
 *                                   -> Result<(consumed, produced), DecompressionError>
 *                                                                  src/decompress.rs:179-337
 * `read` writes only output[output_position .. output_position + *produced); bytes in front of
 * output_position are never read or written.  When it returns FDH_SUCCESS with *stream_status ==
 * FDH_STREAM_OK at least one of the reference's post-conditions holds (src/decompress.rs:167-170):
 * the input is fully consumed (almost always: see 1. below), the output is full but there are
 * more bytes, or the stream is complete (is_done).  Once done, read returns (0, 0)
 * (src/decompress.rs:185-187).  A `DecompressionError` is reported in *stream_status (1 + ordinal)
 * and is sticky.  An EMPTY input asks for whatever can still be produced from the bytes already
 * handed over (how the reference's own test harness, src/decompress/tests/test_utils.rs:70-74, and
 * the png crate finish a stream).  Function return = infrastructure status as everywhere else.
 * `output_position > output_len` (a panic in the reference, :189) is FDH_ERR_INVALID_ARGUMENT.
 *
 * Where the (consumed, produced) pairs differ from the reference's -- the bytes delivered over a whole
 * stream, their order, the final status and is_done never do (tests/test_gpu_streaming.py):
 *   1. Input is buffered on the device, so a call usually consumes all of it where the reference stops once
 *      the output is full (src/decompress.rs:167-170).  *consumed < input_len only when 192 KiB (or the
 *      caller's room, if that is more) are waiting unread on the device already: the rest is to be offered
 *      again, as with the reference.  A caller written against the contract ("consumed bytes must not be
 *      offered again, the others must") behaves identically.
 *   2. With more than 256 KiB of received input a call with NON-EMPTY input may return (consumed, 0)
 *      without a decode attempt (attempts are then made when the stream has grown by 1/8 or by 64 KiB,
 *      and on every EMPTY input).  A caller must therefore conclude "truncated" (the reference's InsufficientInput,
 *      src/decompress.rs:1135-1136) only after a read with empty input has produced nothing and
 *      is_done is still false -- which is what the reference's own harness and the png crate do at
 *      the end of their input anyway.  (tests/test_gpu_streaming.py,
 *      test_reference_bounded_loop_over_the_streaming_object: the loop of the reference's own
 *      decompress_to_vec_bounded, src/decompress.rs:1111-1144, with that one flush added, over streams of more
 *      than 256 KiB whole and in 40 000-byte pieces.)
 *   3. (round 6) The bound of 1. never holds a stream up: an attempt that moved nothing -- no new resume point, no new
 *      byte -- is followed by a call that takes input again, bound or no bound, because more input is the only
 *      thing that can move it.  A sequence of calls with input left therefore never returns (0, 0) for ever.
 * Device memory (round 5): like the reference, which keeps its tables and needs the last 32 KiB of the caller's
 * buffer (src/decompress.rs:96-113, 1067-1070), the object keeps what its resume point needs and no more -- the
 * unread input, a copy of the current block's header, 32 KiB of history and the window with what has been decoded
 * ahead of it: well under 1 MiB for a 16 KiB window, whatever the stream's length (fdh_decompressor_device_bytes). */
typedef struct fdh_decompressor fdh_decompressor;
fdh_decompressor *fdh_decompressor_new(void);
void fdh_decompressor_free(fdh_decompressor *d);
void fdh_decompressor_ignore_adler32(fdh_decompressor *d);
int fdh_decompressor_is_done(const fdh_decompressor *d);
/* Introspection: decode attempts made so far (a stream drained through a small window needs O(log) of
 * them: every attempt decodes ahead of what the caller can take, see fdh_decompressor_read). */
uint64_t fdh_decompressor_attempts(const fdh_decompressor *d);
/* Introspection: output bytes decoded by all attempts together.  An attempt goes on from where the last one
 * stopped (fdh_inflate_batch_resumable), so for a stream of N decoded bytes this stays close to N however the
 * input and the room arrive (rounds 1-3: every attempt started at the first byte). */
uint64_t fdh_decompressor_decoded_bytes(const fdh_decompressor *d);
/* Introspection: the most device memory the object's buffers (input tail + header copy, output slot, one
 * record of metadata) have held together, in bytes. */
uint64_t fdh_decompressor_device_bytes(const fdh_decompressor *d);
int fdh_decompressor_read(fdh_decompressor *d, const uint8_t *input, size_t input_len,
                          uint8_t *output, size_t output_len, size_t output_position,
                          size_t *consumed, size_t *produced, uint32_t *stream_status);

/* ---- single-buffer conveniences on HOST memory (names mirror src/lib.rs:29-36) ---------
 * Each stages through the device (H2D, batch of one, D2H) and synchronises.  Results are
 * malloc'd; release with fdh_free().  `*stream_status` receives the per-stream status. */
int fdh_decompress_to_vec(const uint8_t *input, size_t input_len, uint8_t **output,
                          size_t *output_len, uint32_t *stream_status); /* decompress.rs:1079 */
int fdh_decompress_to_vec_bounded(const uint8_t *input, size_t input_len, size_t maxlen,
                                  uint8_t **output, size_t *output_len,
                                  uint32_t *stream_status); /* decompress.rs:1111 */
int fdh_compress_to_vec_ultra_fast(const uint8_t *input, size_t input_len, uint8_t **output,
                                   size_t *output_len); /* compress/mod.rs:313 */
int fdh_compress_to_vec_stored(const uint8_t *input, size_t input_len, uint8_t **output,
                               size_t *output_len); /* compress_to_vec_with_level(.., 0), compress/mod.rs:299 */
int fdh_compress_to_vec(const uint8_t *input, size_t input_len, uint8_t **output,
                        size_t *output_len); /* compress_to_vec = level 1, compress/mod.rs:294 */
int fdh_compress_to_vec_rle(const uint8_t *input, size_t input_len, uint8_t **output,
                            size_t *output_len); /* compress_to_vec_rle, compress/mod.rs:306 */
/* compress_to_vec_with_level, compress/mod.rs:299: level 0 stored, 1, 2 and 3 the general encoder;
 * level 4 and above returns FDH_ERR_INVALID_ARGUMENT (fdh_last_error() names the levels provided). */
int fdh_compress_to_vec_with_level(const uint8_t *input, size_t input_len, uint32_t level,
                                   uint8_t **output, size_t *output_len);
void fdh_free(void *p);

/* ---- several GPUs of one node, one process --------------------------------
 * Streams are independent: a batch is sharded by contiguous stream ranges, one shard per device,
 * decoded with no data-path exchange; the only collective is an all-gather of the per-stream
 * results {status, out_len, adler} over RCCL / xGMI (librccl is loaded on demand, and only when
 * more than one device takes part).  There is no reference counterpart: the crate is
 * single-threaded; this is how a batch API scales it across the node.
 *   fdh_init(device_mask)   devices with bit d set (0 = every visible device): HIP streams, the
 *                           shared decode tables and the RCCL communicator; call again to change
 *   fdh_shutdown()          releases them
 *   fdh_inflate_batch_multi `n_shards` must equal the number of initialised devices; shard i holds
 *                           device pointers ON device i (the i-th selected one) with the meaning of
 *                           fdh_inflate_batch.  If `meta_all` is given (for every shard), device i
 *                           receives the results of ALL shards there: n_shards x 3 x meta_stride
 *                           words, [shard][status | out_len | adler][stream], zero padded.
 *                           Returns when every device has finished. */
typedef struct fdh_shard {
    const uint8_t *in;
    const uint64_t *in_off;
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t *out_len;
    uint32_t *status;
    uint32_t *adler;    /* nullable */
    uint64_t n;
    uint32_t *meta_all; /* nullable (for every shard or for none) */
} fdh_shard_t;
int fdh_init(uint64_t device_mask);
int fdh_shutdown(void);
int fdh_multi_device_count(void); /* devices selected by the last fdh_init, 0 before */
int fdh_multi_uses_rccl(void);    /* 1 if the gather goes through RCCL: more than one device, or
                                     FDH_MULTI_FORCE_RCCL=1 in the environment of fdh_init (a one-rank
                                     communicator: the way to run that path on a one-GPU box) */
int fdh_inflate_batch_multi(const fdh_shard_t *shards, uint32_t n_shards, uint32_t flags,
                            uint64_t meta_stride);

/* ---- introspection ------------------------------------------------------------------- */
uint32_t fdh_version(void);
const char *fdh_status_name(uint32_t stream_status); /* "Ok", "BadZlibHeader", ... */
const char *fdh_last_error(void);                    /* thread-local message of the last failure */
int fdh_device_count(void);                          /* usable gfx950 devices, 0 if none */

/* Debug / parity hook: run the device Huffman-table builder (the restatement of
 * huffman::build_table + CompressedBlock::build_tables, src/huffman.rs:18-184,
 * src/decompress.rs:561-606) on `code_lengths[320]` and return the decode tables in the
 * library's device layout (documented in DESIGN.md): litlen[4096], dist[512] u32 entries.
 * `build_status` = FDH_STREAM_OK or the error build_tables would return.  Device pointers. */
int fdh_debug_build_tables(const uint8_t *code_lengths320, uint32_t hlit, uint32_t *litlen4096,
                           uint32_t *dist512, uint32_t *build_status, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
