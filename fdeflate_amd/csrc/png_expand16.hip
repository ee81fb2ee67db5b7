// png_expand16.hip -- packed PNG scanlines to RGBA16 (include/fdeflate_hip_png16.h): the kernels of png_expand.hip with
// eight bytes per output pixel -- four samples of 16 bits in the device's byte order -- and the specification's exact
// scaling (13.12): the sample itself at depth 16, s * 257, 4369, 21845, 65535 below, palette entries and their alphas
// * 257, the tRNS key compared on the raw samples.  tests/png16_model.py is the authority on every value.
//
// The code is png_expand_body.h's at OPX = 8: the same bands, flat runs and shared steps, one kernel per (bit depth,
// colour type) pair, grid(n, Y), one wavefront per workgroup.  A lane produces kExpand16Group pixels per step from one
// load of exactly their bytes, and every store of a whole group is a 16-byte store.  Where the slot is 8-byte aligned
// the lanes start at its first 16-byte boundary (at most one pixel alone in front), so those stores are aligned whatever
// the width; a slot at 2, 4 or 6 mod 8 is written correctly with unaligned stores -- no whole number of 8-byte pixels
// reaches a boundary from there.  A slot at an odd address is kPngBadSizes.
//
// Depth 16 is a byte swap per sample: v_perm_b32 swaps both samples of a loaded word (ExpandBytes::swap16), and what is
// left for colour types 0, 2 and 4 is moving 16-bit halves into place.
#include "png_expand_body.h"

namespace fdh {

template <int DEPTH, int COLOUR>
__global__ __launch_bounds__(kWave) void png_expand16_kernel(PngExpandArgs a) {
    __shared__ uint32_t pal[256];
    png_expand_image<DEPTH, COLOUR, 8>(a, blockIdx.x, threadIdx.x, pal);
}

}  // namespace fdh

// As fdh_launch_png_expand; FDH_PNG_EXPAND16_WAVES sets the wavefronts per image.
extern "C" int fdh_launch_png_expand16(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off,
                                       const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream, uint32_t* status,
                                       uint64_t n, uint32_t width, uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type,
                                       hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_EXPAND16_WAVES");
    fdh::PngExpandArgs a{pix, pix_off, rgba16, rgba16_off, pal, colour, upstream, status, n, row_bytes, width};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
#define FDH_EXPAND16_CASE(D, C)                                                                  \
    case (D) * 8 + (C):                                                                          \
        hipLaunchKernelGGL((fdh::png_expand16_kernel<D, C>), grid, block, 0, stream, a);         \
        break;
    switch (bit_depth * 8 + colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_EXPAND16_CASE)
        default: return -1;
    }
#undef FDH_EXPAND16_CASE
    return (int)hipGetLastError();
}
