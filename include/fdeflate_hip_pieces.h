/*
 * fdeflate_hip_pieces.h -- extension of fdeflate_hip.h and fdeflate_hip_levels.h: a long input encoded as independent
 * pieces at levels 1 .. 9 and joined into one zlib stream (the pigz construction without the dictionary).
 *
 * fdh_deflate_level_batch encodes one stream per lane of its parser and per wavefront of its block writer: a single
 * long input keeps the device idle.  Here an input of `len` bytes is cut at multiples of a piece size P into
 * max(1, ceil(len / P)) pieces [kP, min((k+1)P, len)) -- the empty input is one empty piece -- every piece is encoded as
 * a raw-deflate stream of its own, and the stitched stream is
 *     78 01 | piece 0 | piece 1 | ... | last piece | Adler-32 of the whole input, big-endian
 * A non-last piece is what the reference writes for that slice from a fresh Compressor::new(w, level, zlib = false)
 * (src/compress/mod.rs:69-72, 99) compressing with Flush::Sync (:284-287; parse/mod.rs:158, 173): the symbols and blocks
 * of a one-shot encode of the slice, every block with BFINAL = 0, then write_bits(0, 3), padding to a byte and
 * 00 00 FF FF.  The last piece is write_data + finish of the same raw compressor: the final block has BFINAL = 1 and is
 * padded to a byte; an empty last piece is the 10-bit fixed block 03 00 (an empty non-last piece, which no cut of an
 * input produces, is the marker alone: 00 00 00 FF FF).  So an input with len <= P is one last piece and its stitched
 * stream is fdh_deflate_level_batch's stream byte for byte, and every stitched stream inflates to the input.  A piece
 * cannot refer to the bytes in front of it: the window is not primed with the previous piece's tail.
 * Conventions, return codes and the meaning of every shared parameter are those of fdeflate_hip.h; no new status value
 * exists.  The symbols live in the same library.  Levels 1 .. 9 only: level 0 and levels above 9 are
 * FDH_ERR_INVALID_ARGUMENT with "level" in the message, before a device is needed (stored blocks need no pieces:
 * fdh_deflate_stored_batch already copies in parallel).
 *
 * fdh_deflate_level_pieces_batch -- fdh_deflate_level_batch in piece mode.  piece_off[n_pieces + 1] are offsets into
 * `raw`, piece k is raw[piece_off[k] .. piece_off[k+1]); piece_last[k] is one byte, not 0 for the last piece of its
 * input.  The parsers run as they do for a stream; the block writer leaves out 78 01, sets BFINAL only where
 * piece_last[k] is set, and ends a non-last piece with the sync marker and a last piece with the padding, in place of
 * the trailer.  out_len[k] is the piece's length, 0xFFFFFFFF for a slot that is too small or a piece above 1 GiB;
 * piece_adler[k] is the Adler-32 of the piece's bytes (B << 16 | A; 0 where out_len[k] is 0xFFFFFFFF because of the
 * piece's size).  Slots of fdh_compress_bound(piece length) bytes always suffice: a slot that takes the piece's zlib
 * stream takes the piece, which has the marker's five bytes at the most (three bits, the padding, four bytes) where
 * the stream has six (78 01 and the Adler-32), and is the same otherwise -- the slack is that of the stream format, no
 * new term of the bound.  Refused before a device is needed: level 0 or above 9, null piece_off / piece_last / out /
 * out_off / out_len / piece_adler, n_pieces above 2^31-1 ("too many"); n_pieces = 0 is success.  Workspace and
 * completion as fdh_deflate_level_batch.
 *
 * fdh_deflate_stitch_batch -- joins pieces into n streams.  Input i owns the pieces first_piece[i] .. first_piece[i+1]
 * (at least one).  Piece k lies at pieces[piece_slot_off[k] ..) with piece_len[k] bytes (the out_len of the call above;
 * piece_slot_off has an entry per piece and one behind the last), covers raw bytes piece_off[k] .. piece_off[k+1], and
 * has the checksum piece_adler[k].  Two kernels.  The plan, one wavefront per input: an exclusive scan of the pieces'
 * lengths gives every piece's place, the total is 2 + sum + 4, and the checksums are combined by a wave reduction with
 *     A = A1 + A2 - 1,   B = B1 + B2 + (len2 mod 65521) * (A1 - 1)      (mod 65521, in 64-bit arithmetic)
 * which is associative; it writes 78 01 and the trailer.  out_len[i] = 0xFFFFFFFF if a piece of the input has
 * piece_len 0xFFFFFFFF, the input has no piece, or the total exceeds the slot out[out_off[i] .. out_off[i+1]) or
 * 2^32 - 2; nothing is written to such a slot.  The copy, one workgroup per piece at a time: the piece's bytes go to
 * their place at ANY byte alignment (a stream behind a PNG prefix starts 41 or more bytes into its file) with 16-byte
 * stores on the destination's alignment and single bytes at both ends; nothing is written outside the piece's place.
 * (A piece is one workgroup's, 256 threads: right at the default size, slow for pieces near 2^30 bytes.)
 * piece_adler is the call's scratch as well: on return piece_adler[k] holds the piece's byte position inside its
 * stream (0xFFFFFFFF for the pieces of a failed input), which is how the copy finds it -- so the call needs no
 * workspace of its own, makes no host synchronisation and reads nothing back; it returns when the kernels are enqueued.
 * `pieces` and `out` must not overlap (the same pointer is refused): the piece slots are a scratch buffer of their own.
 * Refused before a device is needed: a null pointer other than `pieces` of an empty batch, n above 2^31-1 ("too
 * many"); n = 0 is success.
 *
 * Host arithmetic, no device.  piece_bytes below 64 (the per-piece cost dwarfs the data) or above 2^30 (the encoders
 * refuse such a piece) gives 0, as does a level above 9:
 * fdh_deflate_pieces_count -- max(1, ceil(len / piece_bytes)).
 * fdh_deflate_pieces_bound -- the stitched slot: 2 + the sum of fdh_compress_bound over the pieces' lengths + 4.  At
 *   level 0, where there is no piece mode and a caller goes to fdh_deflate_level_batch, fdh_stored_size(len).
 * fdh_png_level_pieces_file_bound -- fdh_png_level_file_bound with that slot: prefix +
 *   fdh_deflate_pieces_bound(rows * (row_bytes + 1), level, piece_bytes) + FDH_PNG_FILE_SUFFIX.
 */
#ifndef FDEFLATE_HIP_PIECES_H
#define FDEFLATE_HIP_PIECES_H

#include "fdeflate_hip.h"
#include "fdeflate_hip_levels.h"

#define FDH_PIECE_BYTES_MIN 64u
#define FDH_PIECE_BYTES_MAX (1u << 30)
#define FDH_PIECE_BYTES_DEFAULT 65536u

#ifdef __cplusplus
extern "C" {
#endif

int fdh_deflate_level_pieces_batch(const uint8_t *raw, const uint64_t *piece_off, const uint8_t *piece_last,
                                   uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint32_t *piece_adler,
                                   uint64_t n_pieces, uint32_t level, void *hip_stream);
int fdh_deflate_stitch_batch(const uint8_t *pieces, const uint64_t *piece_slot_off, const uint32_t *piece_len,
                             uint32_t *piece_adler, const uint64_t *piece_off, const uint64_t *first_piece,
                             uint8_t *out, const uint64_t *out_off, uint32_t *out_len, uint64_t n, void *hip_stream);
uint64_t fdh_deflate_pieces_count(uint64_t len, uint64_t piece_bytes);
uint64_t fdh_deflate_pieces_bound(uint64_t len, uint32_t level, uint64_t piece_bytes);
uint64_t fdh_png_level_pieces_file_bound(uint64_t rows, uint64_t row_bytes, uint32_t level, uint64_t piece_bytes,
                                         uint64_t prefix);

#ifdef __cplusplus
}
#endif
#endif
