/*
 * fdeflate_hip_png_levels.h -- extension of fdeflate_hip.h and fdeflate_hip_levels.h: PNG encode at a compression
 * level, 0 .. 9.
 *
 * The PNG encode calls of fdeflate_hip.h end in the ultra-fast encoder, which is fused with the filters and never has
 * the filtered rows in memory.  fdh_deflate_level_batch (fdeflate_hip_levels.h) encodes buffers in memory at every
 * level.  The call here is the step between them for a mixed batch -- every image's geometry from its own fdh_png_info
 * record, as in "PNG encode: mixed batches" of fdeflate_hip.h -- and two bounds size the slots behind it.  A pipeline
 * is then: packed scanlines (fdh_png_pack_mixed_batch or fdh_png_pack16_mixed_batch), fdh_png_filter_mixed_batch,
 * fdh_deflate_level_batch into the file slots behind each file's prefix, fdh_png_frame_mixed_batch.  Conventions, return
 * codes, statuses and the meaning of every shared parameter are those of fdeflate_hip.h; no new status value exists.
 * The symbols live in the same library.
 *
 * fdh_png_filter_mixed_batch -- image i has the geometry of info[i] (an ENCODABLE record): height rows of row_bytes
 * bytes at pix[pix_off[i] .. pix_off[i+1]).  filt[filt_off[i] .. filt_off[i+1]) receives height rows of 1 + row_bytes
 * bytes: the row's filter type, then the row filtered with it -- what an IDAT stream holds.  The slots must be exact:
 * pix height * row_bytes, types height, filt height * (row_bytes + 1).
 *   flags bit 0 clear (chosen)              each row's type is chosen as fdh_png_choose_filters_mixed_batch chooses it
 *                                           (minimum sum of absolute values, the lowest type number on a tie), written
 *                                           to types[types_off[i] + row] and used at once; types and types_off may both
 *                                           be null: the choice is then recorded in the type bytes of filt only
 *   flags bit 0 set                         types is input: FDH_PNG_FILTER_GIVEN_TYPES
 * The types are those of fdh_png_choose_filters_mixed_batch, the rows those of fdh_png_filter_batch given those types.
 * png_status[i], the first that applies:
 *   upstream[i] where that is not 0
 *   3   the record is not encodable
 *   2   a slot is not exactly its size (or the pair is beyond the encode steps' size limits): nothing is written to the
 *       image's slots
 *   1   flags bit 0 and a type above 4: such a row is written with its type byte and unfiltered, the others as asked
 *   0   otherwise
 * An image that gets upstream[i], 3 or 2 has its filt slot filled with zeros where the slot is exactly the size its
 * record asks for, so that an encoder behind this call reads defined bytes; otherwise nothing of it is touched.  Writes
 * are whole bytes inside the image's own slots.  Refused before a device is needed (FDH_ERR_INVALID_ARGUMENT): null pix,
 * pix_off, filt, filt_off, info or png_status; types without types_off or the reverse; flags bit 0 without types; any
 * other bit of flags; n above 2^31-1 ("too many").  n = 0 is success.  No workspace, no host synchronisation.
 * FDH_PNG_CHOOSE_WAVES and FDH_PNG_CHOOSE_LANES (environment) set the launch shape as for
 * fdh_png_choose_filters_mixed_batch; the result is the same at every setting.
 *
 * fdh_png_level_bound -- the slot fdh_deflate_level_batch needs for `len` bytes at `level`: fdh_stored_size(len) at
 * level 0, fdh_compress_bound(len) at levels 1 .. 9; 0 for a level above 9.
 *
 * fdh_png_level_file_bound -- the file slot of an image of `rows` rows of `row_bytes` bytes whose zlib stream starts
 * `prefix` bytes into the file (FDH_PNG_FILE_PREFIX, or fdh_png_palette_file_prefix): prefix +
 * fdh_png_level_bound(rows * (row_bytes + 1), level) + FDH_PNG_FILE_SUFFIX; 0 for a level above 9.  Host arithmetic.
 */
#ifndef FDEFLATE_HIP_PNG_LEVELS_H
#define FDEFLATE_HIP_PNG_LEVELS_H

#include "fdeflate_hip.h"
#include "fdeflate_hip_levels.h"

#define FDH_PNG_FILTER_GIVEN_TYPES 1u

#ifdef __cplusplus
extern "C" {
#endif

int fdh_png_filter_mixed_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *types, const uint64_t *types_off,
                               uint8_t *filt, const uint64_t *filt_off, const fdh_png_info *info,
                               const uint32_t *upstream, uint32_t flags, uint32_t *png_status, uint64_t n,
                               void *hip_stream);
uint64_t fdh_png_level_bound(uint64_t len, uint32_t level);
uint64_t fdh_png_level_file_bound(uint64_t rows, uint64_t row_bytes, uint32_t level, uint64_t prefix);

#ifdef __cplusplus
}
#endif
#endif
