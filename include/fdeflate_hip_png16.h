/*
 * fdeflate_hip_png16.h -- extension of fdeflate_hip.h: PNG decode and encode at 16 bits per sample.
 *
 * The calls of fdeflate_hip.h stop at eight bits per sample: fdh_png_expand_batch takes the high byte of a 16-bit
 * sample, fdh_png_pack_batch writes 16-bit pairs by doubling eight-bit samples.  The three calls here are their
 * lossless counterparts.  Conventions, return codes, statuses and the meaning of every shared parameter are those of
 * fdeflate_hip.h; no new status value exists.  The symbols live in the same library.
 *
 * RGBA16 -- a picture is [H, W, 4] samples of 16 bits in R, G, B, A order, each in the device's own (little-endian)
 * byte order: a byte buffer viewed as uint16_t is the picture.  Buffers are uint8_t * with byte offsets like every
 * other buffer of the library; the slot of image i is exactly rows * width * 8 bytes and rgba16 + rgba16_off[i] must
 * be 2-byte aligned.
 *
 * fdh_png_expand16_batch -- fdh_png_expand_batch to RGBA16: image i = pix[pix_off[i] .. pix_off[i+1]), whole packed
 * rows at any alignment, to the slot rgba16[rgba16_off[i] .. rgba16_off[i+1]).  pal, colour and upstream as there.
 * The values follow the specification's exact scaling (13.12):
 *   depth 16            the sample itself (big-endian in the file, device order in the picture)
 *   depths 8, 4, 2, 1   s * 257, s * 4369, s * 21845, s * 65535
 *   colour type 3       each channel of the palette entry, and its tRNS alpha, * 257; an index at or above the count
 *                       gives (0, 0, 0, 65535)
 *   tRNS colour key     compared on the raw samples at the file's depth -- all 16 bits at depth 16 --; alpha is 0
 *                       where it matches and 65535 elsewhere
 * png_status[i]:
 *   0 ok (an empty pixel slot with an empty output slot as well: nothing is written)
 *   2 the pixel slot is not whole rows, the output slot is not exactly the image's size, or it starts at an odd
 *     address: nothing is written
 *   9 a palette index at or above the PLTE's count; the image is written in full
 * or upstream[i] where that is not 0.  An illegal depth / colour pair or width: FDH_ERR_INVALID_ARGUMENT.  No byte
 * outside a slot is written and no byte outside pix[pix_off[0] .. pix_off[n]) is read.  FDH_PNG_EXPAND16_WAVES
 * (environment) sets the number of wavefronts per image.
 *
 * fdh_png_expand16_mixed_batch -- fdh_png_expand16_batch at image i's own geometry, read from info[i], as
 * fdh_png_expand_mixed_batch is to fdh_png_expand_batch: the slot's bytes and png_status[i] are what
 * fdh_png_expand16_batch gives for the image alone.  Further statuses: 3 the record is not decodable, 10 colour
 * type 3 and pal is null.
 *
 * fdh_png_pack16_batch -- the exact inverse of fdh_png_expand16_batch for the four pairs of depth 16: image i to the
 * slot pix[pix_off[i] .. pix_off[i+1]) of exactly rows * width * 2 * channels bytes, samples written big-endian.
 *   colour type 6  every sample
 *   colour type 2  R, G, B; needs every A == 65535
 *   colour type 4  R and A; needs R == G == B
 *   colour type 0  R; needs both
 * No colour key is ever written.  upstream as above.
 * png_status[i]:
 *   0  ok: fdh_png_expand16_batch of the pix slot (without a key) gives the image back byte for byte
 *   2  the RGBA16 slot is not whole rows or starts at an odd address, or the pix slot is not exactly the packed size:
 *      nothing is written
 *   13 some pixel has no lossless representation in the pair; the contents of the pix slot are not specified
 * or upstream[i] where that is not 0.  No byte outside a pix slot is written, no byte outside
 * rgba16[rgba16_off[0] .. rgba16_off[n]) is read.  Colour type 3, or any value but 0, 2, 4, 6, or an illegal width:
 * FDH_ERR_INVALID_ARGUMENT.  FDH_PNG_PACK16_WAVES (environment) sets the number of wavefronts per image.
 */
#ifndef FDEFLATE_HIP_PNG16_H
#define FDEFLATE_HIP_PNG16_H

#include "fdeflate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fdh_png_expand16_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *rgba16,
                           const uint64_t *rgba16_off, const uint32_t *pal, const uint32_t *colour,
                           const uint32_t *upstream, uint32_t *png_status, uint64_t n, uint32_t width,
                           uint32_t bit_depth, uint32_t colour_type, void *hip_stream);
int fdh_png_expand16_mixed_batch(const uint8_t *pix, const uint64_t *pix_off, uint8_t *rgba16,
                                 const uint64_t *rgba16_off, const fdh_png_info *info,
                                 const uint32_t *pal, const uint32_t *colour, const uint32_t *upstream,
                                 uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_pack16_batch(const uint8_t *rgba16, const uint64_t *rgba16_off, uint8_t *pix,
                         const uint64_t *pix_off, const uint32_t *upstream, uint32_t *png_status,
                         uint64_t n, uint32_t width, uint32_t colour_type, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
