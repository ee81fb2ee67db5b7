/*
 * fdeflate_hip_png16_encode.h -- extension of fdeflate_hip_png16.h: PNG encode of mixed batches of RGBA16 pictures,
 * the depth / colour pair chosen per picture.
 *
 * fdh_png_pack16_batch writes one width and one colour type of depth 16 per call and knows nothing about the picture.
 * The four calls here are the front of "PNG encode: mixed batches" (fdeflate_hip.h) for RGBA16: what a picture is, the
 * cheapest of the fifteen pairs that holds it without loss, and its packed scanlines in that pair.  Behind the packed
 * scanlines the calls of fdeflate_hip.h take over unchanged: fdh_png_choose_filters_mixed_batch,
 * fdh_png_filter_deflate_ultrafast_mixed_batch and fdh_png_frame_mixed_batch take any encodable record, depth 16
 * included.  Conventions, return codes, statuses and the meaning of every shared parameter are those of fdeflate_hip.h;
 * no new status value exists.  The symbols live in the same library.
 *
 * Records -- info[i] is the fdh_png_info of fdeflate_hip.h; ENCODABLE and DIMENSION records are what "PNG encode:
 * mixed batches" there says.  RGBA16 -- a picture is what fdeflate_hip_png16.h defines: [H, W, 4] samples of 16 bits in
 * the device's byte order, a slot of exactly height * width * 8 bytes that starts at an even address.  A sample is
 * NARROW when its two bytes are equal, s == 257 * (s >> 8): the picture of the high bytes then holds it without loss.
 *
 * fdh_png_analyse16_mixed_batch -- what RGBA16 picture i is, at info[i].width and info[i].height (a dimension record
 * or an encodable one).  summary[i], always over the whole picture:
 *   bit 0        every A is 65535
 *   bit 1        every pixel has R == G == B, on all 16 bits
 *   bit 2        every sample (R, G, B and A) is narrow: eight bits suffice
 *   bits 8..15   the smallest d of 1, 2, 4, 8, 16 such that every R, G, B is a multiple of 65535 / (2^d - 1), that is
 *                of 65535, 21845, 4369, 257, 1
 * (a picture of no rows: bits 0, 1 and 2, depth 1).  Where bit 2 is set, pal, colour and trns_len are what
 * fdh_png_analyse_mixed_batch gives for the picture of the high bytes: the distinct words R | G << 8 | B << 16 | A << 24
 * in ascending order (pal is nullable), their count in colour[4 i], and the number of entries with A < 255.
 * png_status[i], the first that applies:
 *   upstream[i] where that is not 0
 *   3   the record is of neither kind
 *   2   the slot is not exactly height * width * 8 bytes or starts at an odd address: nothing is written for the image
 *   12  bit 2 is clear, or there are more than max_colours distinct pixels: the summary is valid; pal, colour and
 *       trns_len hold the words fdh_png_analyse_mixed_batch writes on overflow
 *   0   otherwise
 * max_colours outside 1 .. 256 or n above 2^31-1: FDH_ERR_INVALID_ARGUMENT before a device is needed.  No workspace, no
 * host synchronisation.  FDH_PNG_ANALYSE_WAVES (environment) sets the wavefronts per image; the result is the same at
 * every setting.
 *
 * fdh_png_encode16_plan_one / fdh_png_encode16_plan_batch -- fdh_png_encode_plan_one / _batch for the outputs of the
 * analysis above: the same parameters, the same four sizes (packed, filter types, prefix, file slot), `allowed` as
 * there.
 *   encodable record                    the pair is kept; sizes and statuses are fdh_png_encode_plan_one's
 *   dimension record, summary bit 2     exactly fdh_png_encode_plan_one with this summary's bits 0, 1 and depth: a narrow
 *                                       picture gets the pair, and later the file, of its high bytes' RGBA8 picture
 *   dimension record, bit 2 clear       candidates grey (0, 16): bits 0 and 1; grey-alpha (4, 16): bit 1; RGB (2, 16):
 *                                       bit 0; RGBA (6, 16) always; each dropped where `allowed` masks its colour type;
 *                                       cost height * row_bytes, the smallest wins, the lower colour type on equal
 *                                       cost; 13 if none is left.  analyse_status 12 is no error (there is no palette),
 *                                       any other value but 0 is passed on
 * Size limits and status 2 as there.  fdh_png_encode16_plan_one is host arithmetic and needs no device.
 *
 * fdh_png_pack16_mixed_batch -- RGBA16 picture i to the packed scanlines of info[i]'s own pair and width, all fifteen
 * pairs:
 *   depth 16 (colour types 0, 2, 4, 6)   the pix slot and the statuses 0 / 13 are byte for byte what
 *                                        fdh_png_pack16_batch gives for the image alone
 *   depth 8 and below (eleven pairs)     every sample of the picture must be narrow, else 13; the slot's bytes are then
 *                                        exactly what fdh_png_pack_batch gives for the picture of the high bytes with
 *                                        the same pal / colour (the lowest index of equal palette words, sub-byte
 *                                        packing in whole bytes, padding bits zero)
 * png_status[i]:
 *   upstream[i] where that is not 0
 *   3   the record is not encodable
 *   2   the RGBA16 slot is not exactly height * width * 8 bytes or starts at an odd address, or the pix slot is not
 *       exactly height * row_bytes bytes (or the pair is beyond the encode steps' size limits): nothing is written
 *   10  colour type 3 and pal is null
 *   13  some pixel has no lossless representation in the pair; the contents of the pix slot are not specified
 *   0   otherwise
 * No byte outside a pix slot is written, no byte outside rgba16[rgba16_off[0] .. rgba16_off[n]) is read.
 * FDH_PNG_PACK16_WAVES (environment) sets the wavefronts per image.
 */
#ifndef FDEFLATE_HIP_PNG16_ENCODE_H
#define FDEFLATE_HIP_PNG16_ENCODE_H

#include "fdeflate_hip_png16.h"

#ifdef __cplusplus
extern "C" {
#endif

int fdh_png_analyse16_mixed_batch(const uint8_t *rgba16, const uint64_t *rgba16_off, const fdh_png_info *info,
                                  const uint32_t *upstream, uint32_t *pal, uint32_t *colour, uint32_t *trns_len,
                                  uint32_t *summary, uint32_t *png_status, uint64_t n, uint32_t max_colours,
                                  void *hip_stream);
uint32_t fdh_png_encode16_plan_one(fdh_png_info *rec, const uint32_t *colour_count, const uint32_t *trns_len,
                                   uint32_t summary, uint32_t analyse_status, uint32_t allowed, uint64_t sizes[4]);
int fdh_png_encode16_plan_batch(fdh_png_info *info, const uint32_t *colour, const uint32_t *trns_len,
                                const uint32_t *summary, const uint32_t *analyse_status, uint32_t allowed,
                                uint64_t *pix_size, uint64_t *types_size, uint64_t *prefix, uint64_t *file_size,
                                uint32_t *png_status, uint64_t n, void *hip_stream);
int fdh_png_pack16_mixed_batch(const uint8_t *rgba16, const uint64_t *rgba16_off, uint8_t *pix, const uint64_t *pix_off,
                               const fdh_png_info *info, const uint32_t *pal, const uint32_t *colour,
                               const uint32_t *upstream, uint32_t *png_status, uint64_t n, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
