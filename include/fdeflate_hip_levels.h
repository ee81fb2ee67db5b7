/*
 * fdeflate_hip_levels.h -- extension of fdeflate_hip.h: `compress_to_vec_with_level(input, level)` at every level the
 * reference names, 0 .. 9 (src/compress/mod.rs:69-101).
 *
 * fdeflate_hip.h provides levels 0-3 and refuses the others: fdh_compress_to_vec_with_level and
 * fdh_deflate_general_batch keep that range and that refusal.  The three calls here take a `level` instead of an
 * FDH_MODE_*.  Levels 0-3 go to the encoders of fdeflate_hip.h and give their bytes (0 fdh_deflate_stored_batch, 1-3
 * fdh_deflate_general_batch in FDH_MODE_LEVEL1 / 2 / 3).  Levels 4-9 are LazyParser (src/compress/parse/lazy.rs) over
 * HybridMatchFinder (src/compress/matchfinder/hybrid.rs), bit-exact with the reference:
 *   level   LazyParser::new(skip_ahead_shift, max_lazy, ..)   HybridMatchFinder::new(min_match, search_depth, nice_length)
 *   4       (9, 12)                                           (5, 16, 32)
 *   5       (9, 16)                                           (5, 64, 64)
 *   6       (9, 16)                                           (4, 128, 128)
 *   7-9     (12, 256)                                         (4, 256, 258)     one parameter set: identical bytes
 * level > 9 is FDH_ERR_INVALID_ARGUMENT with "level" in the message.  This deviates from the reference on purpose: its
 * `7.. =>` arm (mod.rs:87) takes any u8 above 9 as level 7, while its doc comment promises levels 1-9.
 * Conventions, return codes and the meaning of every shared parameter are those of fdeflate_hip.h; no new status value
 * exists.  The symbols live in the same library.  The expected bytes of levels 4-9 come from tests/lazy_model.py, a
 * restatement over the pieces of tests/level_model.py that the oracle pins at level 1 and RLE; the hybrid finder and the
 * lazy loop have no second implementation.
 *
 * fdh_deflate_level_batch -- the contract of fdh_deflate_general_batch: device pointers, slots of at least
 * fdh_compress_bound(len_i) bytes (level 0: fdh_stored_size), out_len[i] = 0xFFFFFFFF for a slot that is too small or a
 * buffer above 1 GiB, nothing written outside a slot, returns after the kernels have finished.  Refused before a device
 * is needed: level > 9, null in_off / out_off / out_len / out, n above 2^31-1 ("too many"); n = 0 is success.  At levels
 * 4-9 the call uses the per-device workspace of the general encoder; a resident stream has two 256 KiB tables and a
 * 128 KiB link ring (640 KiB, at most 16 GiB: 26 214 streams in flight).
 *
 * fdh_compress_to_vec_level -- the host one-shot, as fdh_compress_to_vec_with_level: host pointers, the result from
 * malloc (fdh_free).  The empty input at levels 1-9 gives 78 01 03 00 00 00 00 01.
 *
 * fdh_debug_level_plan -- out = {lanes, wavefronts} of the parser's launch for n streams at a lazy level (4 .. 9) on a
 * device of `cus` CUs; needs no device.  0, or -1 for another level, n = 0 or a null `out`.
 */
#ifndef FDEFLATE_HIP_LEVELS_H
#define FDEFLATE_HIP_LEVELS_H

#include "fdeflate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int fdh_deflate_level_batch(const uint8_t *raw, const uint64_t *in_off, uint8_t *out, const uint64_t *out_off,
                            uint32_t *out_len, uint64_t n, uint32_t level, void *hip_stream);
int fdh_compress_to_vec_level(const uint8_t *input, size_t input_len, uint32_t level, uint8_t **output,
                              size_t *output_len);
int fdh_debug_level_plan(uint64_t n, int cus, uint32_t level, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
