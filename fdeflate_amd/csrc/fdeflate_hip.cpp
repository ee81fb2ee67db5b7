// fdeflate_hip.cpp -- host side of the C ABI declared in include/fdeflate_hip.h.
// Thin: argument checks, kernel launches, and H2D/D2H staging for the single-buffer
// conveniences.  There is deliberately no CPU decode/encode path in this library.
#include "launch.h"
#include "png_common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? FDH_ERR_OUT_OF_MEMORY : FDH_ERR_HIP; }

int hip_fail(hipError_t e, const char* what) { return fail(hip_code(e), std::string(what) + ": " + hipGetErrorString(e)); }

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

bool have_device() { return fdh_device_count() > 0; }

int no_device() { return fail(FDH_ERR_NO_DEVICE, "no HIP device: fdeflate_hip has no CPU fallback"); }

// What the batch entry points check once they know there is work, in this order: the pointers the call cannot do
// without (`null_msg` names them), the batch size (`noun`: what the call counts), a device.  A pointer that is required
// only under a condition is listed as `condition ? pointer : one that is required anyway`.
int batch_ok(std::initializer_list<const void*> required, const char* null_msg, uint64_t n, const char* noun) {
    for (const void* p : required)
        if (!p) return fail(FDH_ERR_INVALID_ARGUMENT, null_msg);
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, std::string("too many ") + noun + " in one call (max 2^31-1)");
    if (!have_device()) return no_device();
    return FDH_SUCCESS;
}

// ... and how they end: a launcher's return value as the call's
int launched(const char* what, int rc) { return rc != 0 ? hip_fail(static_cast<hipError_t>(rc), what) : FDH_SUCCESS; }

hipStream_t stream_of(void* hip_stream) { return static_cast<hipStream_t>(hip_stream); }

// The shared decode tables of the ultra-fast prefix are built on the device once per device.
std::mutex g_canon_mutex;
bool g_canon_ready[fdh::kMaxDevices] = {};

// the current device, where the per-device arrays have a slot for it
int device_slot(int& dev) {
    HIP_TRY(hipGetDevice(&dev));
    if (!fdh::device_ordinal_ok(dev)) return fail(FDH_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    return FDH_SUCCESS;
}

int ensure_canon_tables(hipStream_t stream) {
    int dev = 0;
    if (int rc = device_slot(dev)) return rc;
    std::lock_guard<std::mutex> lock(g_canon_mutex);
    if (g_canon_ready[dev]) return FDH_SUCCESS;
    uint32_t st = 0xFFFFFFFFu;
    if (int rc = launched("canonical table build", fdh_launch_canon_build(stream, &st))) return rc;
    if (st != 0) return fail(FDH_ERR_HIP, "canonical table build returned status " + std::to_string(st));
    g_canon_ready[dev] = true;
    return FDH_SUCCESS;
}

const char* kStatusNames[] = {
    "Ok", "BadZlibHeader", "InsufficientInput", "InvalidBlockType", "InvalidUncompressedBlockLength",
    "InvalidHlit", "InvalidHdist", "InvalidCodeLengthRepeat", "BadCodeLengthHuffmanTree",
    "BadLiteralLengthHuffmanTree", "BadDistanceHuffmanTree", "InvalidLiteralLengthCode",
    "InvalidDistanceCode", "InputStartsWithRun", "DistanceTooFarBack", "WrongChecksum", "ExtraInput",
    "OutputTooLarge"};

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    template <class T>
    T* as() { return static_cast<T*>(p); }
};

}  // namespace

extern "C" {

uint32_t fdh_version(void) { return FDH_VERSION; }

const char* fdh_status_name(uint32_t s) { return s < 18 ? kStatusNames[s] : "Unknown"; }

const char* fdh_last_error(void) { return g_last_error.c_str(); }

// used by the other translation units of the library (not part of the public header)
void fdh_set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }

int fdh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

uint64_t fdh_ultrafast_bound(uint64_t len) { return fdh::png_ultrafast_bound(len); }

uint64_t fdh_stored_size(uint64_t len) {
    const uint64_t nb = len / 65535, rem = len - nb * 65535;
    return 2 + nb * (5 + 65535) + (rem ? 5 + rem : 2) + 4;
}

int fdh_deflate_stored_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                             uint32_t* out_len, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({in_off, out_off, out_len}, "null metadata pointer", n, "buffers")) return rc;
    return launched("stored-encoder kernel launch", fdh_launch_deflate_stored(in, in_off, out, out_off, out_len, n, stream_of(hip_stream)));
}

int fdh_inflate_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                      uint32_t* out_len, uint32_t* status, uint32_t* adler, uint64_t n, uint32_t flags,
                      void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({in_off, out_off, out_len, status}, "null metadata pointer", n, "streams")) return rc;
    if (int rc = ensure_canon_tables(stream_of(hip_stream))) return rc;
    return launched("inflate kernel launch", fdh_launch_inflate(in, in_off, out, out_off, out_len, status, adler, n,
                    flags & ~FDH_FLAG_RESUME_IN, nullptr, stream_of(hip_stream)));
}

int fdh_inflate_batch_resumable(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                                uint32_t* out_len, uint32_t* status, uint32_t* adler, uint64_t n, uint32_t flags,
                                fdh_resume_point* resume, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({in_off, out_off, out_len, status, resume}, "null metadata pointer", n, "streams")) return rc;
    if (int rc = ensure_canon_tables(stream_of(hip_stream))) return rc;
    return launched("inflate kernel launch", fdh_launch_inflate(in, in_off, out, out_off, out_len, status, adler, n, flags, resume,
                    stream_of(hip_stream)));
}

int fdh_deflate_ultrafast_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                                uint32_t* out_len, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({in_off, out_off, out_len}, "null metadata pointer", n, "buffers")) return rc;
    return launched("deflate kernel launch", fdh_launch_deflate_ultrafast(in, in_off, out, out_off, out_len, n, stream_of(hip_stream)));
}

int fdh_debug_build_tables(const uint8_t* code_lengths320, uint32_t hlit, uint32_t* litlen4096, uint32_t* dist512,
                           uint32_t* build_status, void* hip_stream) {
    if (!have_device()) return no_device();
    return launched("table-build kernel launch", fdh_launch_build_tables_debug(code_lengths320, hlit, litlen4096, dist512, build_status,
                    stream_of(hip_stream)));
}

// ---- PNG scanline filters (the steps either side of the codec in the PNG pipeline) ----
// (the row calls check their geometry between the pointers and the device, and the first three have no limit on n)
static int png_args_ok(const void* a, const void* b, const void* c, const void* d, const void* st, uint32_t row_bytes,
                       uint32_t bpp) {
    if (!a || !b || !c || !d || !st) return fail(FDH_ERR_INVALID_ARGUMENT, "null pointer");
    if (row_bytes == 0) return fail(FDH_ERR_INVALID_ARGUMENT, "row_bytes must be positive");
    if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8))
        return fail(FDH_ERR_INVALID_ARGUMENT, "bpp must be 1, 2, 3, 4, 6 or 8 (PNG's whole-byte pixel sizes)");
    if (!have_device()) return no_device();
    return FDH_SUCCESS;
}

int fdh_png_unfilter_batch(const uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off,
                           uint32_t* png_status, uint64_t n, uint32_t row_bytes, uint32_t bpp, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = png_args_ok(filt, filt_off, pix, pix_off, png_status, row_bytes, bpp)) return rc;
    return launched("unfilter kernel launch", fdh_launch_png_unfilter(filt, filt_off, pix, pix_off, png_status, nullptr, nullptr, n,
                    row_bytes, bpp, stream_of(hip_stream)));
}

int fdh_png_filter_batch(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types, const uint64_t* types_off,
                         uint8_t* filt, const uint64_t* filt_off, uint32_t* png_status, uint64_t n, uint32_t row_bytes,
                         uint32_t bpp, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = png_args_ok(pix, pix_off, filt, filt_off, png_status, row_bytes, bpp)) return rc;
    if (!types || !types_off) return fail(FDH_ERR_INVALID_ARGUMENT, "null pointer");
    return launched("filter kernel launch", fdh_launch_png_filter(pix, pix_off, types, types_off, filt, filt_off, png_status, n, row_bytes,
                    bpp, stream_of(hip_stream)));
}

int fdh_png_choose_filters_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                 uint32_t* png_status, uint64_t n, uint32_t row_bytes, uint32_t bpp, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (row_bytes >= (1u << 25))
        return fail(FDH_ERR_INVALID_ARGUMENT, "row_bytes must be below 2^25 (a row's filter cost is summed in 32 bits)");
    if (int rc = png_args_ok(pix, pix_off, types, types_off, png_status, row_bytes, bpp)) return rc;
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many images in one call (max 2^31-1)");
    return launched("filter-selection kernel launch", fdh_launch_png_choose(pix, pix_off, types, types_off, png_status, n, row_bytes, bpp,
                    stream_of(hip_stream)));
}

int fdh_png_filter_deflate_ultrafast_batch(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types,
                                           const uint64_t* types_off, uint8_t* out, const uint64_t* out_off,
                                           uint32_t* out_len, uint32_t* png_status, uint64_t n, uint32_t row_bytes,
                                           uint32_t bpp, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = png_args_ok(pix, pix_off, out, out_off, png_status, row_bytes, bpp)) return rc;
    if (!types || !types_off || !out_len) return fail(FDH_ERR_INVALID_ARGUMENT, "null pointer");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many buffers in one call (max 2^31-1)");
    return launched("filter + deflate kernel launch", fdh_launch_png_filter_deflate_ultrafast(pix, pix_off, types, types_off, out, out_off,
                    out_len, png_status, n, row_bytes, bpp, stream_of(hip_stream)));
}

int fdh_inflate_png_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* filt, const uint64_t* filt_off,
                          uint32_t* out_len, uint32_t* status, uint32_t* adler, uint8_t* pix, const uint64_t* pix_off,
                          uint32_t* png_status, uint64_t n, uint32_t flags, uint32_t row_bytes, uint32_t bpp,
                          void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = png_args_ok(filt, filt_off, pix, pix_off, png_status, row_bytes, bpp)) return rc;
    if (int rc = fdh_inflate_batch(in, in_off, filt, filt_off, out_len, status, adler, n, flags, hip_stream)) return rc;
    // same stream: the scanlines are reconstructed as soon as the decode kernels have finished, only
    // for the streams that decoded (status 0) -- the rest gets FDH_PNG_STATUS_SKIPPED -- and that decoded to
    // exactly the bytes of their slot: a stream that ends early would leave stale bytes behind it
    // (FDH_PNG_STATUS_BAD_SIZES; the png crate treats short IDAT data as an error as well)
    return launched("unfilter kernel launch", fdh_launch_png_unfilter(filt, filt_off, pix, pix_off, png_status, status, out_len, n,
                    row_bytes, bpp, stream_of(hip_stream)));
}

// ---- PNG files: CRC-32, framing, container scan, IDAT gather (png_file.hip) ----
int fdh_crc32_batch(const uint8_t* data, const uint64_t* off, const uint32_t* len, const uint32_t* seed, uint32_t* crc,
                    uint32_t* status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({off, crc, status}, "null metadata pointer", n, "ranges")) return rc;
    return launched("CRC-32 kernel launch", fdh_launch_crc32(data, off, len, seed, crc, status, n, stream_of(hip_stream)));
}

uint64_t fdh_png_file_bound(uint64_t rows, uint64_t row_bytes) {
    return fdh_ultrafast_bound(rows * (row_bytes + 1)) + FDH_PNG_FILE_PREFIX + FDH_PNG_FILE_SUFFIX;
}

// (the calls that take a geometry refuse a bad one before anything else, an empty batch included)
static int png_geometry_ok(uint32_t width, uint32_t bit_depth, uint32_t colour_type) {
    if (width == 0 || width > 0x7FFFFFFFu) return fail(FDH_ERR_INVALID_ARGUMENT, "width must be 1 .. 2^31-1");
    if (!fdh::png_pair_ok(bit_depth, colour_type))
        return fail(FDH_ERR_INVALID_ARGUMENT, "bit depth / colour type is not one of the PNG specification's fifteen pairs");
    return FDH_SUCCESS;
}

int fdh_png_frame_batch(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height,
                        uint32_t* file_len, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth,
                        uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, idat_len, height, file_len, png_status}, "null pointer", n, "files")) return rc;
    return launched("PNG framing kernel launch", fdh_launch_png_frame(file, file_off, idat_len, height, file_len, png_status, n, width,
                    bit_depth, colour_type, stream_of(hip_stream)));
}

int fdh_png_scan_files_batch(const uint8_t* file, const uint64_t* file_off, const uint32_t* file_len, fdh_png_info* info,
                             uint64_t n, uint32_t flags, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, info}, "null pointer", n, "files")) return rc;
    return launched("PNG scan kernel launch", fdh_launch_png_scan(file, file_off, file_len, info, n,
                    (flags & FDH_PNG_FLAG_IGNORE_CRC) ? 0 : 1, (flags & FDH_PNG_FLAG_ADAM7) ? 1 : 0, stream_of(hip_stream)));
}

int fdh_png_gather_idat_batch(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint8_t* comp,
                              const uint64_t* comp_off, uint32_t* comp_len, uint32_t* png_status, uint64_t n,
                              uint32_t width, uint32_t bit_depth, uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, info, comp, comp_off, comp_len, png_status}, "null pointer", n, "files")) return rc;
    return launched("IDAT gather kernel launch", fdh_launch_png_gather(file, file_off, info, comp, comp_off, comp_len, png_status, n, width,
                    bit_depth, colour_type, stream_of(hip_stream)));
}

// ---- PNG decode to RGBA8: PLTE / tRNS (png_file.hip), expansion (png_expand.hip) ----
int fdh_png_colour_batch(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint32_t* pal,
                         uint32_t* colour, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth,
                         uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, info, colour, png_status, colour_type == 3 ? pal : png_status}, "null pointer", n, "files")) return rc;
    return launched("PLTE / tRNS kernel launch", fdh_launch_png_colour(file, file_off, info, pal, colour, png_status, n, width, bit_depth,
                    colour_type, stream_of(hip_stream)));
}

int fdh_png_expand_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off,
                         const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* png_status,
                         uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, rgba, rgba_off, png_status, colour_type == 3 ? pal : png_status}, "null pointer", n, "images")) return rc;
    const uint64_t row_bytes = fdh::png_row_bytes(width, fdh::png_pixel_bits(bit_depth, colour_type));
    return launched("RGBA expansion kernel launch", fdh_launch_png_expand(pix, pix_off, rgba, rgba_off, pal, colour, upstream, png_status,
                    n, width, row_bytes, bit_depth, colour_type, stream_of(hip_stream)));
}

// ---- PNG decode: Adam7 interlaced images (png_adam7.hip) ----
uint64_t fdh_png_adam7_size(uint32_t width, uint32_t height, uint32_t bit_depth, uint32_t colour_type) {
    if (width == 0 || height == 0 || !fdh::png_pair_ok(bit_depth, colour_type)) return 0;
    return fdh::png_adam7_size(width, height, fdh::png_pixel_bits(bit_depth, colour_type), 1);
}

int fdh_png_unfilter_interlaced_batch(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off,
                                      const uint8_t* method, const uint32_t* upstream, const uint32_t* upstream_len,
                                      uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth,
                                      uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({filt, filt_off, pix, pix_off, png_status}, "null pointer", n, "images")) return rc;
    return launched("Adam7 reconstruction / placement kernel launch", fdh_launch_png_adam7(filt, filt_off, pix, pix_off, method, upstream,
                    upstream_len, png_status, n, width, bit_depth, colour_type, stream_of(hip_stream)));
}

// ---- PNG decode: mixed batches (png_mixed.hip) ----
uint32_t fdh_png_plan_sizes(const fdh_png_info* rec, uint64_t max_bytes, uint64_t sizes[4]) {
    uint64_t s[4] = {0, 0, 0, 0};
    const uint32_t st = rec ? fdh::png_plan(*rec, max_bytes, s[0], s[1], s[2], s[3]) : FDH_PNG_STATUS_SKIPPED;
    if (sizes) std::copy(s, s + 4, sizes);
    return st;
}

int fdh_png_plan_batch(const fdh_png_info* info, uint64_t max_bytes, uint64_t* comp_size, uint64_t* filt_size, uint64_t* pix_size,
                       uint64_t* rgba_size, uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({info, png_status}, "null pointer", n, "records")) return rc;
    return launched("PNG plan kernel launch", fdh_launch_png_plan(info, max_bytes, comp_size, filt_size, pix_size, rgba_size, png_status, n,
                    stream_of(hip_stream)));
}

int fdh_png_gather_idat_mixed_batch(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, const uint32_t* upstream,
                                    uint8_t* comp, const uint64_t* comp_off, uint32_t* comp_len, uint32_t* png_status, uint64_t n,
                                    void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, info, comp, comp_off, comp_len, png_status}, "null pointer", n, "files")) return rc;
    return launched("IDAT gather kernel launch", fdh_launch_png_gather_mixed(file, file_off, info, upstream, comp, comp_off, comp_len,
                    png_status, n, stream_of(hip_stream)));
}

int fdh_png_colour_mixed_batch(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, const uint32_t* upstream,
                               uint32_t* pal, uint32_t* colour, uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, info, pal, colour, png_status}, "null pointer", n, "files")) return rc;
    return launched("PLTE / tRNS kernel launch", fdh_launch_png_colour_mixed(file, file_off, info, upstream, pal, colour, png_status, n,
                    stream_of(hip_stream)));
}

int fdh_png_unfilter_mixed_batch(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off, const fdh_png_info* info,
                                 const uint32_t* upstream, const uint32_t* upstream_len, uint32_t* png_status, uint64_t n,
                                 void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({filt, filt_off, pix, pix_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed reconstruction / placement kernel launch", fdh_launch_png_unfilter_mixed(filt, filt_off, pix, pix_off, info,
                    upstream, upstream_len, png_status, n, stream_of(hip_stream)));
}

int fdh_png_expand_mixed_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off,
                               const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                               uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, rgba, rgba_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA expansion kernel launch", fdh_launch_png_expand_mixed(pix, pix_off, rgba, rgba_off, info, pal, colour,
                    upstream, png_status, n, stream_of(hip_stream)));
}

// ---- PNG at 16 bits per sample (include/fdeflate_hip_png16.h): png_expand16.hip, png_mixed.hip, png_pack16.hip ----
int fdh_png_expand16_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off,
                           const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* png_status,
                           uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, rgba16, rgba16_off, png_status, colour_type == 3 ? pal : png_status}, "null pointer", n, "images")) return rc;
    const uint64_t row_bytes = fdh::png_row_bytes(width, fdh::png_pixel_bits(bit_depth, colour_type));
    return launched("RGBA16 expansion kernel launch", fdh_launch_png_expand16(pix, pix_off, rgba16, rgba16_off, pal, colour, upstream,
                    png_status, n, width, row_bytes, bit_depth, colour_type, stream_of(hip_stream)));
}

int fdh_png_expand16_mixed_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off,
                                 const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                 uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, rgba16, rgba16_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA16 expansion kernel launch", fdh_launch_png_expand16_mixed(pix, pix_off, rgba16, rgba16_off, info, pal,
                    colour, upstream, png_status, n, stream_of(hip_stream)));
}

int fdh_png_pack16_batch(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                         const uint32_t* upstream, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t colour_type,
                         void* hip_stream) {
    if (colour_type == 3 || !fdh::png_pair_ok(16, colour_type))
        return fail(FDH_ERR_INVALID_ARGUMENT, "colour type must be 0, 2, 4 or 6 (the pairs of depth 16; there is no palette of 16-bit entries)");
    if (int rc = png_geometry_ok(width, 16, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba16, rgba16_off, pix, pix_off, png_status}, "null pointer", n, "images")) return rc;
    return launched("RGBA16 packing kernel launch", fdh_launch_png_pack16(rgba16, rgba16_off, pix, pix_off, upstream, png_status, n, width,
                    colour_type, stream_of(hip_stream)));
}

// ---- PNG encode: mixed batches of RGBA16 pictures (include/fdeflate_hip_png16_encode.h): png_encode16_mixed.hip, and the
// plan kernel of png_encode_mixed.hip ----
// (fdh_png_encode16_plan_one stands beside fdh_png_encode_plan_one below)
int fdh_png_analyse16_mixed_batch(const uint8_t* rgba16, const uint64_t* rgba16_off, const fdh_png_info* info, const uint32_t* upstream,
                                  uint32_t* pal, uint32_t* colour, uint32_t* trns_len, uint32_t* summary, uint32_t* png_status, uint64_t n,
                                  uint32_t max_colours, void* hip_stream) {
    if (max_colours == 0 || max_colours > 256) return fail(FDH_ERR_INVALID_ARGUMENT, "max_colours must be 1 .. 256");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many images in one call (max 2^31-1)");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba16, rgba16_off, info, colour, trns_len, summary, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA16 analysis kernel launch", fdh_launch_png_analyse16_mixed(rgba16, rgba16_off, info, upstream, pal, colour,
                    trns_len, summary, png_status, n, max_colours, stream_of(hip_stream)));
}

int fdh_png_encode16_plan_batch(fdh_png_info* info, const uint32_t* colour, const uint32_t* trns_len, const uint32_t* summary,
                                const uint32_t* analyse_status, uint32_t allowed, uint64_t* pix_size, uint64_t* types_size, uint64_t* prefix,
                                uint64_t* file_size, uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (allowed & ~0x5Du) return fail(FDH_ERR_INVALID_ARGUMENT, "allowed may hold the bits of colour types 0, 2, 3, 4 and 6 only");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many records in one call (max 2^31-1)");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({info}, "null pointer", n, "records")) return rc;
    return launched("RGBA16 encode plan kernel launch", fdh_launch_png_encode_plan(info, colour, trns_len, summary, analyse_status, allowed,
                    pix_size, types_size, prefix, file_size, png_status, n, 1, stream_of(hip_stream)));
}

int fdh_png_pack16_mixed_batch(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                               const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                               uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many images in one call (max 2^31-1)");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba16, rgba16_off, pix, pix_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA16 packing kernel launch", fdh_launch_png_pack16_mixed(rgba16, rgba16_off, pix, pix_off, info, pal, colour,
                    upstream, png_status, n, stream_of(hip_stream)));
}

// ---- PNG encode from RGBA8: analysis and packing (png_pack.hip), palette framing (png_file.hip) ----
int fdh_png_analyse_batch(const uint8_t* rgba, const uint64_t* rgba_off, uint32_t* pal, uint32_t* colour, uint32_t* trns_len,
                          uint32_t* summary, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t max_colours, void* hip_stream) {
    if (width == 0 || width > 0x7FFFFFFFu) return fail(FDH_ERR_INVALID_ARGUMENT, "width must be 1 .. 2^31-1");
    if (max_colours == 0 || max_colours > 256) return fail(FDH_ERR_INVALID_ARGUMENT, "max_colours must be 1 .. 256");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba, rgba_off, colour, trns_len, summary, png_status}, "null pointer", n, "images")) return rc;
    return launched("RGBA analysis kernel launch", fdh_launch_png_analyse(rgba, rgba_off, pal, colour, trns_len, summary, png_status, n,
                    width, max_colours, stream_of(hip_stream)));
}

int fdh_png_pack_batch(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off, const uint32_t* pal,
                       const uint32_t* colour, const uint32_t* upstream, uint32_t* png_status, uint64_t n, uint32_t width,
                       uint32_t bit_depth, uint32_t colour_type, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, colour_type)) return rc;
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba, rgba_off, pix, pix_off, png_status, colour_type == 3 ? pal : png_status}, "null pointer", n, "images")) return rc;
    const uint64_t row_bytes = fdh::png_row_bytes(width, fdh::png_pixel_bits(bit_depth, colour_type));
    return launched("RGBA packing kernel launch", fdh_launch_png_pack(rgba, rgba_off, pix, pix_off, pal, colour, upstream, png_status, n,
                    width, row_bytes, bit_depth, colour_type, stream_of(hip_stream)));
}

uint64_t fdh_png_palette_file_prefix(uint32_t plte_entries, uint32_t trns_entries) {
    if (plte_entries == 0 || plte_entries > 256 || trns_entries > plte_entries) return 0;
    return FDH_PNG_FILE_PREFIX + 12 + 3 * (uint64_t)plte_entries + (trns_entries ? 12 + (uint64_t)trns_entries : 0);
}

int fdh_png_frame_palette_batch(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height,
                                const uint32_t* pal, const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len,
                                uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t plte_entries,
                                uint32_t trns_entries, void* hip_stream) {
    if (int rc = png_geometry_ok(width, bit_depth, 3)) return rc;
    if (plte_entries == 0 || plte_entries > std::min(256u, 1u << bit_depth))
        return fail(FDH_ERR_INVALID_ARGUMENT, "plte_entries must be 1 .. min(256, 2^bit_depth)");
    if (trns_entries > plte_entries) return fail(FDH_ERR_INVALID_ARGUMENT, "trns_entries must be 0 .. plte_entries");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, idat_len, height, pal, colour, trns_len, file_len, png_status}, "null pointer", n, "files")) return rc;
    return launched("PNG palette framing kernel launch", fdh_launch_png_frame_palette(file, file_off, idat_len, height, pal, colour, trns_len,
                    file_len, png_status, n, width, bit_depth, plte_entries, trns_entries, stream_of(hip_stream)));
}

// ---- PNG encode: mixed batches (png_encode_mixed.hip; the fused encoder in deflate_ultrafast.hip, the framing in png_file.hip) ----
// (the plan of one record for RGBA8 pictures and, rgba16, for RGBA16 ones: include/fdeflate_hip_png16_encode.h)
static uint32_t encode_plan_one(bool rgba16, fdh_png_info* rec, const uint32_t* colour_count, const uint32_t* trns_len, uint32_t summary,
                                uint32_t analyse_status, uint32_t allowed, uint64_t sizes[4]) {
    uint64_t s[4] = {0, 0, 0, 0};
    uint32_t st = FDH_PNG_STATUS_SKIPPED;
    if (rec) {
        const bool dimension = fdh::png_dimension_record(rec->status, rec->width, rec->height, rec->bit_depth, rec->colour_type, rec->interlace);
        const bool have_colour = colour_count && trns_len;
        uint32_t depth = rec->bit_depth, colour = rec->colour_type;
        const auto plan = rgba16 ? fdh::png_encode16_plan : fdh::png_encode_plan;
        st = plan(rec->status, rec->width, rec->height, depth, colour, rec->interlace, have_colour, have_colour ? *colour_count : 0u,
                  have_colour ? *trns_len : 0u, summary, analyse_status, allowed, s[0], s[1], s[2], s[3]);
        if (st == FDH_PNG_STATUS_OK && dimension) rec->bit_depth = (uint8_t)depth, rec->colour_type = (uint8_t)colour;
    }
    if (sizes) std::copy(s, s + 4, sizes);
    return st;
}

uint32_t fdh_png_encode_plan_one(fdh_png_info* rec, const uint32_t* colour_count, const uint32_t* trns_len, uint32_t summary,
                                 uint32_t analyse_status, uint32_t allowed, uint64_t sizes[4]) {
    return encode_plan_one(false, rec, colour_count, trns_len, summary, analyse_status, allowed, sizes);
}

uint32_t fdh_png_encode16_plan_one(fdh_png_info* rec, const uint32_t* colour_count, const uint32_t* trns_len, uint32_t summary,
                                   uint32_t analyse_status, uint32_t allowed, uint64_t sizes[4]) {
    return encode_plan_one(true, rec, colour_count, trns_len, summary, analyse_status, allowed, sizes);
}

int fdh_png_encode_plan_batch(fdh_png_info* info, const uint32_t* colour, const uint32_t* trns_len, const uint32_t* summary,
                              const uint32_t* analyse_status, uint32_t allowed, uint64_t* pix_size, uint64_t* types_size, uint64_t* prefix,
                              uint64_t* file_size, uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (allowed & ~0x5Du) return fail(FDH_ERR_INVALID_ARGUMENT, "allowed may hold the bits of colour types 0, 2, 3, 4 and 6 only");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({info}, "null pointer", n, "records")) return rc;
    return launched("PNG encode plan kernel launch", fdh_launch_png_encode_plan(info, colour, trns_len, summary, analyse_status, allowed,
                    pix_size, types_size, prefix, file_size, png_status, n, 0, stream_of(hip_stream)));
}

int fdh_png_analyse_mixed_batch(const uint8_t* rgba, const uint64_t* rgba_off, const fdh_png_info* info, const uint32_t* upstream,
                                uint32_t* pal, uint32_t* colour, uint32_t* trns_len, uint32_t* summary, uint32_t* png_status, uint64_t n,
                                uint32_t max_colours, void* hip_stream) {
    if (max_colours == 0 || max_colours > 256) return fail(FDH_ERR_INVALID_ARGUMENT, "max_colours must be 1 .. 256");
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba, rgba_off, info, colour, trns_len, summary, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA analysis kernel launch", fdh_launch_png_analyse_mixed(rgba, rgba_off, info, upstream, pal, colour, trns_len,
                    summary, png_status, n, max_colours, stream_of(hip_stream)));
}

int fdh_png_pack_mixed_batch(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off, const fdh_png_info* info,
                             const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* png_status, uint64_t n,
                             void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({rgba, rgba_off, pix, pix_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed RGBA packing kernel launch", fdh_launch_png_pack_mixed(rgba, rgba_off, pix, pix_off, info, pal, colour, upstream,
                    png_status, n, stream_of(hip_stream)));
}

int fdh_png_choose_filters_mixed_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                       const fdh_png_info* info, const uint32_t* upstream, uint32_t* png_status, uint64_t n,
                                       void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, types, types_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed filter-selection kernel launch", fdh_launch_png_choose_mixed(pix, pix_off, types, types_off, info, upstream,
                    png_status, n, stream_of(hip_stream)));
}

int fdh_png_filter_deflate_ultrafast_mixed_batch(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types, const uint64_t* types_off,
                                                 uint8_t* out, const uint64_t* out_off, uint32_t* out_len, const fdh_png_info* info,
                                                 const uint32_t* upstream, uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({pix, pix_off, types, types_off, out, out_off, out_len, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed filter + deflate kernel launch", fdh_launch_png_filter_deflate_ultrafast_mixed(pix, pix_off, types, types_off, out,
                    out_off, out_len, info, upstream, png_status, n, stream_of(hip_stream)));
}

int fdh_png_frame_mixed_batch(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const fdh_png_info* info, const uint32_t* pal,
                              const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len, uint32_t* png_status, uint64_t n,
                              void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (int rc = batch_ok({file, file_off, idat_len, info, file_len, png_status}, "null pointer", n, "files")) return rc;
    return launched("mixed PNG framing kernel launch", fdh_launch_png_frame_mixed(file, file_off, idat_len, info, pal, colour, trns_len,
                    file_len, png_status, n, stream_of(hip_stream)));
}

uint64_t fdh_compress_bound(uint64_t len) { return len + len / 2 + 1024; }

// fdh_deflate_general_batch, fdh_deflate_level_batch at levels 1 .. 9 and fdh_deflate_level_pieces_batch: one contract,
// one body.  Each resolves its mode or level to a row of launch.h's kEncoders (`row` null: a number that is none);
// with `pieces` (include/fdeflate_hip_pieces.h) the streams are pieces.
struct PieceMode {
    const uint8_t* last;
    uint32_t* adler;
};
static int general_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off, uint32_t* out_len, uint64_t n,
                         const fdh::EncoderRow* row, void* hip_stream, PieceMode pieces = {nullptr, nullptr}) {
    if (n == 0) return FDH_SUCCESS;
    if (!in_off || !out_off || !out_len) return fail(FDH_ERR_INVALID_ARGUMENT, "null metadata pointer");
    if (!out) return fail(FDH_ERR_INVALID_ARGUMENT, "null data pointer");  // (`in` may be null for a batch of empty inputs: below)
    if (!row) return fail(FDH_ERR_INVALID_ARGUMENT, "unknown encoder mode");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many streams in one call");
    if (!have_device()) return no_device();
    hipStream_t stream = stream_of(hip_stream);
    int dev = 0;
    if (int rc = device_slot(dev)) return rc;
    // the launcher sizes its record arrays by the bytes the batch spans
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], in_off, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&ends[1], in_off + n, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (ends[1] < ends[0]) return fail(FDH_ERR_INVALID_ARGUMENT, "in_off is not ascending");
    const uint64_t total_in = ends[1] - ends[0];
    // an empty input has a defined encoding (78 01 03 00 00 00 00 01), and a zero-element buffer has no address
    if (!in && total_in != 0) return fail(FDH_ERR_INVALID_ARGUMENT, "null data pointer");
    // the launcher (deflate_general.hip) plans the launch, keeps the workspace and has left the text of a failure
    const int rc = fdh_launch_deflate_encoder(in, in_off, pieces.last, out, out_off, out_len, pieces.adler, n, row, total_in, stream);
    return rc == 0 ? FDH_SUCCESS : hip_code(static_cast<hipError_t>(rc));
}

int fdh_deflate_general_batch(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                              uint32_t* out_len, uint64_t n, uint32_t mode, void* hip_stream) {
    return general_batch(in, in_off, out, out_off, out_len, n, fdh::encoder_of_mode(mode), hip_stream);
}

// include/fdeflate_hip_levels.h: level 0 is the stored encoder, 1 .. 9 are rows
static int bad_level() { return fail(FDH_ERR_INVALID_ARGUMENT, "compression level above 9: levels 0 .. 9 exist"); }

int fdh_deflate_level_batch(const uint8_t* raw, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                            uint64_t n, uint32_t level, void* hip_stream) {
    if (level > 9) return bad_level();
    if (n == 0) return FDH_SUCCESS;
    // This door's own order and, at level 0, its own texts: the count is refused before a null `out` is (general_batch has
    // them the other way round) and in general_batch's words, not in the stored call's (tests/test_abi_levels.py).
    if (!in_off || !out_off || !out_len) return fail(FDH_ERR_INVALID_ARGUMENT, "null metadata pointer");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many streams in one call");
    if (level == 0) return fdh_deflate_stored_batch(raw, in_off, out, out_off, out_len, n, hip_stream);
    return general_batch(raw, in_off, out, out_off, out_len, n, fdh::encoder_of_level(level), hip_stream);
}

// ---- PNG encode at a compression level (include/fdeflate_hip_png_levels.h): png_filter_mixed.hip ----
int fdh_png_filter_mixed_batch(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off, uint8_t* filt,
                               const uint64_t* filt_off, const fdh_png_info* info, const uint32_t* upstream, uint32_t flags,
                               uint32_t* png_status, uint64_t n, void* hip_stream) {
    if (flags & ~FDH_PNG_FILTER_GIVEN_TYPES) return fail(FDH_ERR_INVALID_ARGUMENT, "unknown flags (bit 0, FDH_PNG_FILTER_GIVEN_TYPES, is the only one)");
    if (n > 0x7FFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "too many images in one call (max 2^31-1)");
    if (n == 0) return FDH_SUCCESS;
    if (!types != !types_off) return fail(FDH_ERR_INVALID_ARGUMENT, "null pointer: types and types_off go together");
    if ((flags & FDH_PNG_FILTER_GIVEN_TYPES) && !types) return fail(FDH_ERR_INVALID_ARGUMENT, "null pointer: the given types");
    if (int rc = batch_ok({pix, pix_off, filt, filt_off, info, png_status}, "null pointer", n, "images")) return rc;
    return launched("mixed filter kernel launch", fdh_launch_png_filter_mixed(pix, pix_off, types, types_off, filt, filt_off, info, upstream,
                    flags, png_status, n, stream_of(hip_stream)));
}

uint64_t fdh_png_level_bound(uint64_t len, uint32_t level) {
    return level > 9 ? 0 : level == 0 ? fdh_stored_size(len) : fdh_compress_bound(len);
}

uint64_t fdh_png_level_file_bound(uint64_t rows, uint64_t row_bytes, uint32_t level, uint64_t prefix) {
    return level > 9 ? 0 : prefix + fdh_png_level_bound(rows * (row_bytes + 1), level) + FDH_PNG_FILE_SUFFIX;
}

// ---- long inputs in pieces (include/fdeflate_hip_pieces.h): deflate_general.hip in piece mode, deflate_stitch.hip ----
static bool piece_bytes_ok(uint64_t piece_bytes) { return piece_bytes >= FDH_PIECE_BYTES_MIN && piece_bytes <= FDH_PIECE_BYTES_MAX; }

// the one implementation behind the three host functions: the number of pieces and the stitched slot of `len` bytes
static void pieces_of(uint64_t len, uint64_t piece_bytes, uint64_t* count, uint64_t* bound) {
    const uint64_t full = len / piece_bytes, rest = len - full * piece_bytes;
    *count = full + (rest || !full ? 1 : 0);
    *bound = 2 + full * fdh_compress_bound(piece_bytes) + (rest || !full ? fdh_compress_bound(rest) : 0) + 4;
}

uint64_t fdh_deflate_pieces_count(uint64_t len, uint64_t piece_bytes) {
    uint64_t count = 0, bound = 0;
    if (piece_bytes_ok(piece_bytes)) pieces_of(len, piece_bytes, &count, &bound);
    return count;
}

uint64_t fdh_deflate_pieces_bound(uint64_t len, uint32_t level, uint64_t piece_bytes) {
    uint64_t count = 0, bound = 0;
    if (level > 9 || !piece_bytes_ok(piece_bytes)) return 0;
    if (level == 0) return fdh_stored_size(len);
    pieces_of(len, piece_bytes, &count, &bound);
    return bound;
}

uint64_t fdh_png_level_pieces_file_bound(uint64_t rows, uint64_t row_bytes, uint32_t level, uint64_t piece_bytes, uint64_t prefix) {
    const uint64_t stream = fdh_deflate_pieces_bound(rows * (row_bytes + 1), level, piece_bytes);
    return stream ? prefix + stream + FDH_PNG_FILE_SUFFIX : 0;
}

int fdh_deflate_level_pieces_batch(const uint8_t* raw, const uint64_t* piece_off, const uint8_t* piece_last, uint8_t* out,
                                   const uint64_t* out_off, uint32_t* out_len, uint32_t* piece_adler, uint64_t n_pieces, uint32_t level,
                                   void* hip_stream) {
    if (level == 0 || level > 9) return fail(FDH_ERR_INVALID_ARGUMENT, "compression level outside 1 .. 9: piece mode exists at levels 1 .. 9");
    if (n_pieces == 0) return FDH_SUCCESS;
    if (!piece_last || !piece_adler) return fail(FDH_ERR_INVALID_ARGUMENT, "null metadata pointer");
    return general_batch(raw, piece_off, out, out_off, out_len, n_pieces, fdh::encoder_of_level(level), hip_stream, {piece_last, piece_adler});
}

int fdh_deflate_stitch_batch(const uint8_t* pieces, const uint64_t* piece_slot_off, const uint32_t* piece_len, uint32_t* piece_adler,
                             const uint64_t* piece_off, const uint64_t* first_piece, uint8_t* out, const uint64_t* out_off,
                             uint32_t* out_len, uint64_t n, void* hip_stream) {
    if (n == 0) return FDH_SUCCESS;
    if (pieces && pieces == out)
        return fail(FDH_ERR_INVALID_ARGUMENT, "pieces and out are the same buffer: the piece slots are a scratch buffer of their own");
    if (int rc = batch_ok({pieces, piece_slot_off, piece_len, piece_adler, piece_off, first_piece, out, out_off, out_len}, "null pointer", n,
                          "streams"))
        return rc;
    return launched("stitch kernel launch", fdh_launch_deflate_stitch(pieces, piece_slot_off, piece_len, piece_adler, piece_off, first_piece,
                    out, out_off, out_len, n, stream_of(hip_stream)));
}

// ---- single-buffer conveniences (host memory) --------------------------------------------

// One decode of a host buffer into a device slot of `cap` bytes; the decoded (or partial) bytes
// are returned in a malloc'd buffer.  The device copy of the input is kept by the caller so that
// a retry with a larger slot does not upload it again.
static int inflate_one(DevBuf& d_in, size_t input_len, size_t cap, uint8_t** output, size_t* output_len,
                       uint32_t* stream_status) {
    DevBuf d_out, d_meta;
    HIP_TRY(d_out.alloc(cap));
    HIP_TRY(d_meta.alloc(64));
    uint64_t meta[8] = {0, (uint64_t)input_len, 0, (uint64_t)cap, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(d_meta.p, meta, sizeof(meta), hipMemcpyHostToDevice));
    uint64_t* m = d_meta.as<uint64_t>();
    uint32_t* res = reinterpret_cast<uint32_t*>(m + 4);
    int rc = fdh_inflate_batch(d_in.as<uint8_t>(), m, d_out.as<uint8_t>(), m + 2, res, res + 1, res + 2, 1, 0, nullptr);
    if (rc != FDH_SUCCESS) return rc;
    uint32_t host_res[4];
    HIP_TRY(hipMemcpy(host_res, res, sizeof(host_res), hipMemcpyDeviceToHost));  // synchronises the null stream
    *stream_status = host_res[1];
    size_t n = host_res[0];
    if (n > cap) n = cap;
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    if (!buf) return fail(FDH_ERR_OUT_OF_MEMORY, "malloc");
    if (n) {
        hipError_t e = hipMemcpy(buf, d_out.p, n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            std::free(buf);
            return hip_fail(e, "hipMemcpy(decoded bytes)");
        }
    }
    *output = buf;
    *output_len = n;
    return FDH_SUCCESS;
}

// decompress_to_vec_bounded (src/decompress.rs:1111-1144).  The reference grows its Vec from 1 KiB
// by 32 KiB steps up to `maxlen` (:1117, :1133); the device needs a slot size up front, so the slot
// starts at min(maxlen, 4 x input + 64 KiB) and is quadrupled (up to maxlen) while the stream
// reports OutputTooLarge below maxlen -- a huge `maxlen` never allocates more than the stream
// needs (x4), and the result is the one a slot of `maxlen` bytes would have given.
static int inflate_growing(const uint8_t* input, size_t input_len, size_t maxlen, uint8_t** output,
                           size_t* output_len, uint32_t* stream_status) {
    if (!output || !output_len || !stream_status) return fail(FDH_ERR_INVALID_ARGUMENT, "null result pointer");
    *output = nullptr;
    *output_len = 0;
    if (!have_device()) return no_device();
    if (input_len >= (1ull << 31)) return fail(FDH_ERR_INVALID_ARGUMENT, "stream too large (>= 2 GiB)");
    if (maxlen > 0xFFFFFFF0ull) maxlen = 0xFFFFFFF0ull;
    DevBuf d_in;
    HIP_TRY(d_in.alloc(input_len));
    if (input_len) HIP_TRY(hipMemcpy(d_in.p, input, input_len, hipMemcpyHostToDevice));
    size_t cap = std::min<size_t>(maxlen, input_len * 4 + 65536);
    for (;;) {
        int rc = inflate_one(d_in, input_len, cap, output, output_len, stream_status);
        if (rc != FDH_SUCCESS) return rc;
        if (*stream_status != FDH_OUTPUT_TOO_LARGE || cap >= maxlen) return FDH_SUCCESS;
        std::free(*output);
        *output = nullptr;
        *output_len = 0;
        cap = cap > maxlen / 4 ? maxlen : cap * 4;
    }
}

int fdh_decompress_to_vec_bounded(const uint8_t* input, size_t input_len, size_t maxlen, uint8_t** output,
                                  size_t* output_len, uint32_t* stream_status) {
    return inflate_growing(input, input_len, maxlen, output, output_len, stream_status);
}

// decompress_to_vec grows its Vec without bound (src/decompress.rs:1079-1087): the same loop with
// the ABI's largest slot as the bound.
int fdh_decompress_to_vec(const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len,
                          uint32_t* stream_status) {
    return inflate_growing(input, input_len, 0xFFFFFFF0ull, output, output_len, stream_status);
}

// which encoder a host call runs: the ultra-fast one, the stored one, or the general one in a row of launch.h's kEncoders
struct Encoder {
    enum Type { kUltraFast, kStored, kGeneral } type;
    const fdh::EncoderRow* row = nullptr;  // kGeneral
};
static Encoder encoder_of_level(uint32_t level) { return level ? Encoder{Encoder::kGeneral, fdh::encoder_of_level(level)} : Encoder{Encoder::kStored}; }

static int compress_one(Encoder enc, const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len) {
    if (!output || !output_len) return fail(FDH_ERR_INVALID_ARGUMENT, "null result pointer");
    if (input_len >= 0xFFFFFFFFull) return fail(FDH_ERR_INVALID_ARGUMENT, "buffer too large (>= 4 GiB)");
    if (!have_device()) return no_device();
    const size_t cap = (size_t)(enc.type == Encoder::kStored      ? fdh_stored_size(input_len)
                                : enc.type == Encoder::kUltraFast ? fdh_ultrafast_bound(input_len)
                                                                  : fdh_compress_bound(input_len));
    DevBuf d_in, d_out, d_meta;
    HIP_TRY(d_in.alloc(input_len));
    HIP_TRY(d_out.alloc(cap));
    HIP_TRY(d_meta.alloc(64));
    uint64_t meta[8] = {0, (uint64_t)input_len, 0, (uint64_t)cap, 0, 0, 0, 0};
    if (input_len) HIP_TRY(hipMemcpy(d_in.p, input, input_len, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_meta.p, meta, sizeof(meta), hipMemcpyHostToDevice));
    uint64_t* m = d_meta.as<uint64_t>();
    uint32_t* res = reinterpret_cast<uint32_t*>(m + 4);
    int rc = enc.type == Encoder::kStored      ? fdh_deflate_stored_batch(d_in.as<uint8_t>(), m, d_out.as<uint8_t>(), m + 2, res, 1, nullptr)
             : enc.type == Encoder::kUltraFast ? fdh_deflate_ultrafast_batch(d_in.as<uint8_t>(), m, d_out.as<uint8_t>(), m + 2, res, 1, nullptr)
                                               : general_batch(d_in.as<uint8_t>(), m, d_out.as<uint8_t>(), m + 2, res, 1, enc.row, nullptr);
    if (rc != FDH_SUCCESS) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t n32 = 0;
    HIP_TRY(hipMemcpy(&n32, res, 4, hipMemcpyDeviceToHost));
    if (n32 == 0xFFFFFFFFu) return fail(FDH_ERR_HIP, "internal: encoder bound exceeded");
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(n32 ? n32 : 1));
    if (!buf) return fail(FDH_ERR_OUT_OF_MEMORY, "malloc");
    if (n32) {
        hipError_t e = hipMemcpy(buf, d_out.p, n32, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            std::free(buf);
            return hip_fail(e, "hipMemcpy(compressed bytes)");
        }
    }
    *output = buf;
    *output_len = n32;
    return FDH_SUCCESS;
}

int fdh_compress_to_vec_ultra_fast(const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len) {
    return compress_one({Encoder::kUltraFast}, input, input_len, output, output_len);
}

int fdh_compress_to_vec_stored(const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len) {
    return compress_one({Encoder::kStored}, input, input_len, output, output_len);
}

int fdh_compress_to_vec(const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len) {
    return compress_one({Encoder::kGeneral, fdh::encoder_of_mode(FDH_MODE_LEVEL1)}, input, input_len, output, output_len);
}

int fdh_compress_to_vec_rle(const uint8_t* input, size_t input_len, uint8_t** output, size_t* output_len) {
    return compress_one({Encoder::kGeneral, fdh::encoder_of_mode(FDH_MODE_RLE)}, input, input_len, output, output_len);
}

int fdh_compress_to_vec_with_level(const uint8_t* input, size_t input_len, uint32_t level, uint8_t** output,
                                   size_t* output_len) {
    if (level > 3)
        return fail(FDH_ERR_INVALID_ARGUMENT, "compression level not provided by this call: levels 0, 1, 2 and 3 are (4-9, the lazy parser: "
                                              "fdh_compress_to_vec_level of fdeflate_hip_levels.h)");
    return compress_one(encoder_of_level(level), input, input_len, output, output_len);
}

int fdh_compress_to_vec_level(const uint8_t* input, size_t input_len, uint32_t level, uint8_t** output, size_t* output_len) {
    if (level > 9) return bad_level();
    return compress_one(encoder_of_level(level), input, input_len, output, output_len);
}

void fdh_free(void* p) { std::free(p); }

}  // extern "C"
