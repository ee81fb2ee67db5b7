// png_expand.hip -- packed PNG scanlines to RGBA8 (include/fdeflate_hip.h, "PNG decode to RGBA8"): sample unpacking
// (PNG specification 7.2: most significant bits first, 16-bit samples big-endian), scaling to eight bits, palette
// look-up, the tRNS colour key.  tests/png_expand_model.py is the authority on every value.
//
// One kernel per (bit depth, colour type) pair: everything the pair decides -- bytes per pixel, the scale factor, whether
// there is a palette or a key -- is a compile-time constant.  grid(n, Y), one wavefront per workgroup: workgroup (i, b)
// takes the bands b, b + Y, .. of kExpandBand rows of image i, as png_choose_kernel does.  A lane produces four pixels per
// step: ONE 16-byte store, 1 KiB per wavefront and step, from 0.5 (1-bit grey) to 32 (16-bit RGBA) bytes of input, read
// with one load of exactly those bytes, so nothing outside the image is ever read.
//
// Rows whose bits fill whole bytes (every pair of 8 bits or more per pixel, and narrower ones at a fitting width) have no
// padding: a band is then ONE run of pixels, and where the output slot is 4-byte aligned the lanes start at its first
// 16-byte boundary, so every wide store is aligned whatever the width.  Rows with padding bits are taken row by row; rows
// of fewer than 64 quads share a step (64 / quads rows to a step).
//
// Palette: 256 words R | G << 8 | B << 16 | A << 24 per image (fdh_png_colour_batch writes them, 0xFF000000 behind the
// PLTE's count), copied to the LDS once per workgroup.  An index at or above the count is what kPngIndexOutsidePalette
// reports: one atomicOr per wavefront that saw one.
#include "png_expand_body.h"

namespace fdh {

template <int DEPTH, int COLOUR>
__global__ __launch_bounds__(kWave) void png_expand_kernel(PngExpandArgs a) {
    __shared__ uint32_t pal[256];
    png_expand_image<DEPTH, COLOUR>(a, blockIdx.x, threadIdx.x, pal);
}

}  // namespace fdh

// A wavefront takes the bands b, b + Y, .. of its image; Y is chosen so that a small batch of tall images still fills the
// GPU (png_waves_per_image), FDH_PNG_EXPAND_WAVES sets it.  The statuses start at kPngOk: kPngIndexOutsidePalette is OR-ed in.
extern "C" int fdh_launch_png_expand(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off,
                                     const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* status,
                                     uint64_t n, uint32_t width, uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type,
                                     hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_EXPAND_WAVES");
    fdh::PngExpandArgs a{pix, pix_off, rgba, rgba_off, pal, colour, upstream, status, n, row_bytes, width};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
#define FDH_EXPAND_CASE(D, C)                                                                  \
    case (D) * 8 + (C):                                                                        \
        hipLaunchKernelGGL((fdh::png_expand_kernel<D, C>), grid, block, 0, stream, a);         \
        break;
    switch (bit_depth * 8 + colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_EXPAND_CASE)
        default: return -1;
    }
#undef FDH_EXPAND_CASE
    return (int)hipGetLastError();
}
