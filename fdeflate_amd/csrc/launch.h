// launch.h -- the boundary between the host side of the ABI (fdeflate_hip.cpp, stream_decompressor.cpp, multi_gpu.cpp)
// and the files that hold the kernels: every launcher is declared here, once, and both its callers and the file that
// defines it include this header, so a definition that disagrees with its declaration does not compile.  Not part of
// the public header.  A launcher returns 0 or a hipError_t (-1: an argument no kernel was built for).  Behind the
// declarations: what the launchers themselves share.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/fdeflate_hip.h"
#include "../../include/fdeflate_hip_png16.h"
#include "../../include/fdeflate_hip_png16_encode.h"
#include "../../include/fdeflate_hip_levels.h"
#include "../../include/fdeflate_hip_png_levels.h"
#include "../../include/fdeflate_hip_pieces.h"

namespace fdh { struct SegArgs; struct EncoderRow; }
int fdh_launch_seg3(const fdh::SegArgs& sa, unsigned blocks, hipStream_t stream);  // inflate_seg3.hip, for inflate.hip

extern "C" {
void fdh_set_last_error(const char* msg);  // fdeflate_hip.cpp: fdh_last_error's text, for the other host files
// inflate.hip
int fdh_launch_inflate(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                       uint32_t* status, uint32_t* adler, uint64_t n, uint32_t flags, void* resume_io, hipStream_t stream);
int fdh_launch_canon_build(hipStream_t stream, uint32_t* host_status);
int fdh_launch_build_tables_debug(const uint8_t* code_lengths, uint32_t hlit, uint32_t* litlen, uint32_t* dist, uint32_t* build_status,
                                  hipStream_t stream);
// deflate_stored.hip
int fdh_launch_deflate_stored(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                              uint64_t n, hipStream_t stream);
int fdh_launch_copy_lines(void* dst, const void* src, size_t bytes, hipStream_t stream);
// deflate_ultrafast.hip
int fdh_launch_deflate_ultrafast(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                                 uint64_t n, hipStream_t stream);
int fdh_launch_png_filter_deflate_ultrafast(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types, const uint64_t* types_off,
                                            uint8_t* out, const uint64_t* out_off, uint32_t* out_len, uint32_t* png_status, uint64_t n,
                                            uint32_t row_bytes, uint32_t bpp, hipStream_t stream);
int fdh_launch_png_filter_deflate_ultrafast_mixed(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types, const uint64_t* types_off,
                                                  uint8_t* out, const uint64_t* out_off, uint32_t* out_len, const fdh_png_info* info,
                                                  const uint32_t* upstream, uint32_t* png_status, uint64_t n, hipStream_t stream);
// deflate_general.hip: the parser of `row` (a row of kEncoders below), then the block writer; `total_in` = in_off[n] -
// in_off[0].  Plans the launch, grows the device's workspace, and returns when both kernels have finished; on failure
// fdh_last_error's text names the step that failed.  With `piece_last` and `piece_adler` (both, or both null for whole
// streams; include/fdeflate_hip_pieces.h) stream k is a piece: raw deflate, closed by the sync marker unless
// piece_last[k], its Adler-32 written to piece_adler[k].
int fdh_launch_deflate_encoder(const uint8_t* in, const uint64_t* in_off, const uint8_t* piece_last, uint8_t* out, const uint64_t* out_off,
                               uint32_t* out_len, uint32_t* piece_adler, uint64_t n, const fdh::EncoderRow* row, uint64_t total_in,
                               hipStream_t stream);
// deflate_stitch.hip (include/fdeflate_hip_pieces.h): the plan kernel and the copy kernel; enqueues only
int fdh_launch_deflate_stitch(const uint8_t* pieces, const uint64_t* piece_slot_off, const uint32_t* piece_len, uint32_t* piece_adler,
                              const uint64_t* piece_off, const uint64_t* first_piece, uint8_t* out, const uint64_t* out_off,
                              uint32_t* out_len, uint64_t n, hipStream_t stream);
// png_filter.hip
int fdh_launch_png_unfilter(const uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off, uint32_t* status,
                            const uint32_t* gate, const uint32_t* gate_len, uint64_t n, uint32_t row_bytes, uint32_t bpp,
                            hipStream_t stream);
int fdh_launch_png_filter(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types, const uint64_t* types_off, uint8_t* filt,
                          const uint64_t* filt_off, uint32_t* status, uint64_t n, uint32_t row_bytes, uint32_t bpp, hipStream_t stream);
// png_choose.hip
int fdh_launch_png_choose(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off, uint32_t* status,
                          uint64_t n, uint32_t row_bytes, uint32_t bpp, hipStream_t stream);
// png_file.hip
int fdh_launch_crc32(const uint8_t* data, const uint64_t* off, const uint32_t* len, const uint32_t* seed, uint32_t* crc, uint32_t* status,
                     uint64_t n, hipStream_t stream);
int fdh_launch_png_frame(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height, uint32_t* file_len,
                         uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
int fdh_launch_png_scan(const uint8_t* file, const uint64_t* file_off, const uint32_t* file_len, fdh_png_info* info, uint64_t n,
                        int verify_crc, int adam7, hipStream_t stream);
int fdh_launch_png_gather(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint8_t* comp, const uint64_t* comp_off,
                          uint32_t* comp_len, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type,
                          hipStream_t stream);
int fdh_launch_png_colour(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint32_t* pal, uint32_t* colour,
                          uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
int fdh_launch_png_frame_palette(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height,
                                 const uint32_t* pal, const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len,
                                 uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t plte_entries,
                                 uint32_t trns_entries, hipStream_t stream);
int fdh_launch_png_frame_mixed(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const fdh_png_info* info, const uint32_t* pal,
                               const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len, uint32_t* png_status, uint64_t n,
                               hipStream_t stream);
// png_expand.hip
int fdh_launch_png_expand(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off, const uint32_t* pal,
                          const uint32_t* colour, const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width,
                          uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
// png_pack.hip
int fdh_launch_png_analyse(const uint8_t* rgba, const uint64_t* rgba_off, uint32_t* pal, uint32_t* colour, uint32_t* trns_len,
                           uint32_t* summary, uint32_t* status, uint64_t n, uint32_t width, uint32_t max_colours, hipStream_t stream);
int fdh_launch_png_pack(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off, const uint32_t* pal,
                        const uint32_t* colour, const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width,
                        uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
// png_adam7.hip
int fdh_launch_png_adam7(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off, const uint8_t* method,
                         const uint32_t* upstream, const uint32_t* upstream_len, uint32_t* status, uint64_t n, uint32_t width,
                         uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
// png_mixed.hip
int fdh_launch_png_plan(const fdh_png_info* info, uint64_t max_bytes, uint64_t* comp_size, uint64_t* filt_size, uint64_t* pix_size,
                        uint64_t* rgba_size, uint32_t* png_status, uint64_t n, hipStream_t stream);
int fdh_launch_png_gather_mixed(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, const uint32_t* upstream,
                                uint8_t* comp, const uint64_t* comp_off, uint32_t* comp_len, uint32_t* png_status, uint64_t n,
                                hipStream_t stream);
int fdh_launch_png_colour_mixed(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, const uint32_t* upstream,
                                uint32_t* pal, uint32_t* colour, uint32_t* png_status, uint64_t n, hipStream_t stream);
int fdh_launch_png_unfilter_mixed(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off, const fdh_png_info* info,
                                  const uint32_t* upstream, const uint32_t* upstream_len, uint32_t* status, uint64_t n, hipStream_t stream);
int fdh_launch_png_expand_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off,
                                const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                uint32_t* status, uint64_t n, hipStream_t stream);
// png_encode_mixed.hip (rgba16: the plan of include/fdeflate_hip_png16_encode.h)
int fdh_launch_png_encode_plan(fdh_png_info* info, const uint32_t* colour, const uint32_t* trns_len, const uint32_t* summary,
                               const uint32_t* analyse_status, uint32_t allowed, uint64_t* pix_size, uint64_t* types_size, uint64_t* prefix,
                               uint64_t* file_size, uint32_t* png_status, uint64_t n, int rgba16, hipStream_t stream);
int fdh_launch_png_analyse_mixed(const uint8_t* rgba, const uint64_t* rgba_off, const fdh_png_info* info, const uint32_t* upstream,
                                 uint32_t* pal, uint32_t* colour, uint32_t* trns_len, uint32_t* summary, uint32_t* status, uint64_t n,
                                 uint32_t max_colours, hipStream_t stream);
int fdh_launch_png_pack_mixed(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off, const fdh_png_info* info,
                              const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* status, uint64_t n,
                              hipStream_t stream);
int fdh_launch_png_choose_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                const fdh_png_info* info, const uint32_t* upstream, uint32_t* status, uint64_t n, hipStream_t stream);
// png_expand16.hip, png_mixed.hip, png_pack16.hip (include/fdeflate_hip_png16.h)
int fdh_launch_png_expand16(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off, const uint32_t* pal,
                            const uint32_t* colour, const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width,
                            uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream);
int fdh_launch_png_expand16_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off,
                                  const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                  uint32_t* status, uint64_t n, hipStream_t stream);
int fdh_launch_png_pack16(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                          const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width, uint32_t colour_type,
                          hipStream_t stream);
// png_encode16_mixed.hip (include/fdeflate_hip_png16_encode.h)
int fdh_launch_png_analyse16_mixed(const uint8_t* rgba16, const uint64_t* rgba16_off, const fdh_png_info* info, const uint32_t* upstream,
                                   uint32_t* pal, uint32_t* colour, uint32_t* trns_len, uint32_t* summary, uint32_t* status, uint64_t n,
                                   uint32_t max_colours, hipStream_t stream);
int fdh_launch_png_pack16_mixed(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                                const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                uint32_t* status, uint64_t n, hipStream_t stream);
// png_filter_mixed.hip (include/fdeflate_hip_png_levels.h); clears `status` first
int fdh_launch_png_filter_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off, uint8_t* filt,
                                const uint64_t* filt_off, const fdh_png_info* info, const uint32_t* upstream, uint32_t flags,
                                uint32_t* status, uint64_t n, hipStream_t stream);
}

namespace fdh {

// an environment variable as an integer (the launchers' overrides for tests and A/B runs); `fallback` where it is not set
inline int env_int(const char* name, int fallback) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : fallback;
}

// The encoders of deflate_general.hip, one row per parser configuration: everything the public calls, the launcher and
// the parser kernel need to know about it.
enum class Parser {
    kRle,        // RleParser: runs only, no match finder and no tables
    kHashTable,  // the greedy parser with the HashTableMatchFinder
    kChain2,     // ... with the HashChainMatchFinder of level 2
    kChain3,     // ... and of level 3
    kLazy,       // deflate_lazy.h: LazyParser with the HybridMatchFinder
};
// The lazy parser's parameters, which its kernel takes as arguments (compress/mod.rs:80-87: LazyParser::new(
// skip_ahead_shift, max_lazy, HybridMatchFinder::new(min_match, search_depth, nice_length)); `7.. =>` is one set).
struct LazyParams {
    uint32_t shift, max_lazy, min_match, depth, nice;
};
struct EncoderRow {
    Parser parser;
    uint64_t table_bytes;   // per resident stream: 64 Ki-entry tables (none, one, one, one, two) and, but for the hash-table
                            // finder, a 32 Ki-entry link ring: 0, 256, 384, 384, 640 KiB
    unsigned waves_per_cu;  // the parser's wavefronts wanted per CU before a wavefront is given more streams
    uint64_t max_resident;  // streams in flight: 16 GiB of tables at the most
    LazyParams lazy;        // Parser::kLazy only
};
constexpr EncoderRow encoder_row(Parser p, LazyParams lazy = {}) {
    const uint64_t entries = p == Parser::kRle ? 0u : (p == Parser::kLazy ? 2 : 1) * 65536u + (p == Parser::kHashTable ? 0u : 32768u);
    return {p, entries * 4, p == Parser::kHashTable ? 8u : 16u, entries ? (16ull << 30) / (entries * 4) : 1ull << 40, lazy};
}
constexpr EncoderRow kEncoders[] = {
    encoder_row(Parser::kRle),                            // FDH_MODE_RLE
    encoder_row(Parser::kHashTable),                      // level 1
    encoder_row(Parser::kChain2),                         // level 2
    encoder_row(Parser::kChain3),                         // level 3
    encoder_row(Parser::kLazy, {9, 12, 5, 16, 32}),       // level 4
    encoder_row(Parser::kLazy, {9, 16, 5, 64, 64}),       // level 5
    encoder_row(Parser::kLazy, {9, 16, 4, 128, 128}),     // level 6
    encoder_row(Parser::kLazy, {12, 256, 4, 256, 258}),   // levels 7, 8 and 9
};
static_assert(kEncoders[7].max_resident == 26214, "16 GiB / 640 KiB");
// the row of a level, 1 .. 9, and of an FDH_MODE_*; nullptr for any other number
inline const EncoderRow* encoder_of_level(uint32_t level) { return level >= 1 && level <= 9 ? &kEncoders[std::min(level, 7u)] : nullptr; }
static_assert(FDH_MODE_LEVEL1 == 1 && FDH_MODE_RLE == 2 && FDH_MODE_LEVEL2 == 3 && FDH_MODE_LEVEL3 == 4, "kModeRows' order");
constexpr unsigned kModeRows[] = {1, 0, 2, 3};
inline const EncoderRow* encoder_of_mode(uint32_t mode) { return mode >= 1 && mode <= 4 ? &kEncoders[kModeRows[mode - 1]] : nullptr; }

// The per-device state (the canonical tables' flags, the general encoder's workspaces) is kept in arrays of this many.
constexpr int kMaxDevices = 64;
inline bool device_ordinal_ok(int dev) { return dev >= 0 && dev < kMaxDevices; }

// Wavefronts per range / threads per file in the kernels of png_file.hip and png_mixed.hip that serve one file per
// workgroup: a batch that fills the device by its count alone gets one wavefront per item.
constexpr uint64_t kFillWaves = 4096;

// Wavefronts per image for the kernels that hand an image's bands b, b + Y, .. to wavefront b of Y: Y is chosen so that
// a small batch of tall images still fills the device; the environment variable `name` (1 .. 65535) sets it.
inline uint32_t png_waves_per_image(uint64_t n, const char* name) {
    const int forced = env_int(name, 0);
    if (forced >= 1 && forced <= 65535) return (uint32_t)forced;
    return (uint32_t)std::min<uint64_t>(4096, (32768 + n - 1) / n);
}

}  // namespace fdh
