// png_adam7.hip -- Adam7 interlaced PNG images (include/fdeflate_hip.h, "PNG decode: Adam7 interlaced images"):
// what the zlib decoder left of an IDAT stream -- seven reduced images ("passes") one behind the other, each
// filtered as an image of its own -- becomes the packed scanlines that fdh_png_unfilter_batch produces.  PNG
// specification 8.2 (pass extraction) and 9.2 / 9.4 (filters); tests/png_adam7_model.py is the authority on every
// byte.  A progressive image is the same machinery with one pass, so one batch can hold both kinds.
//
// Two kernels on the stream, no workspace:
//
// png_adam7_recon_kernel<BPP> -- reconstruction IN PLACE, one image per wavefront.  The passes do not depend on each
// other, so the rows of ALL passes form one list (120 rows for 341 x 64: 8 + 8 + 8 + 16 + 16 + 32 + 32) that is cut
// into bands of 64 consecutive rows, one row per lane, skewed by one 16-byte chunk per row as in png_wave_kernel:
// at step t lane j works on chunk t - j of its row, and the chunk above it is what lane j - 1 produced one step
// earlier, handed up by a DPP lane shift.  A lane whose row is the first of its pass has zeros above it instead
// (never the last row of the pass before); lane 0 of a later band reads the row above from memory, where the band
// before has left it.  The lanes' rows have different lengths: a band runs max(chunks + lane) steps.  Passes one
// after the other would keep 8 of 64 lanes busy in passes 1 to 3 of the 64-row shape.  In place is safe in this
// schedule: a lane loads chunk c + 1 of its row before it stores chunk c, and a row is read by no lane but its own
// (and, across a band boundary, by lane 0 of the next band, behind a fence).  Every load is of the bytes of the
// lane's own row and no others, whole chunks and partial ones alike.
//
// png_adam7_place_kernel<BITS> -- placement BY OUTPUT: a lane produces 16 consecutive bytes of a picture row and
// stores them once.  Odd rows are pass 7 alone (and every row of a progressive image is its one pass): a straight
// copy.  An even row y interleaves at most four pass rows -- pass 6 at odd x; at even x pass 5 (y % 4 == 2), passes
// 4 and 3 (y % 8 == 4) or passes 4, 2 and 1 (y % 8 == 0) --, whose addresses are worked out once per 16 bytes; the
// bytes are then gathered in the largest unit that divides both the pixel and the 16 bytes (1, 2, 4 or 8 bytes: one
// byte for RGB8), pixels narrower than a byte bit field by bit field.  One instance per pixel size in bits.
#include "png_adam7_body.h"

namespace fdh {

template <int BPP>
__global__ __launch_bounds__(kWave) void png_adam7_recon_kernel(Adam7Args a) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const Adam7Image g = adam7_image(a, i);
    adam7_recon_image<BPP>(a, g, i, lane);
}

template <int BITS>
__global__ __launch_bounds__(kWave) void png_adam7_place_kernel(Adam7Args a) {
    __shared__ uint64_t s_base[7], s_stride[7];
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (uni(a.status[i]) > kPngBadFilterType) return;  // (kPngBadSizes, kPngSkipped: refused by the reconstruction kernel, nothing is written)
    const Adam7Image g = adam7_image(a, i);
    adam7_place_image<BITS>(a, g, lane, s_base, s_stride);
}

}  // namespace fdh

// Reconstruction: one wavefront per image.  Placement: a wavefront takes the bands b, b + Y, .. of 64 picture rows of its
// image; Y is chosen so that a small batch of tall images still fills the GPU (as fdh_launch_png_expand does),
// FDH_PNG_ADAM7_WAVES sets it.
extern "C" int fdh_launch_png_adam7(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off,
                                    const uint8_t* method, const uint32_t* upstream, const uint32_t* upstream_len,
                                    uint32_t* status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t colour_type,
                                    hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t bits = fdh::png_pixel_bits(bit_depth, colour_type);
    const uint64_t row_bytes = fdh::png_row_bytes(width, bits);
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_ADAM7_WAVES");
    fdh::Adam7Args a{filt, filt_off, pix, pix_off, method, upstream, upstream_len, status, n, row_bytes, width, bits};
    const dim3 block(fdh::kWave), grid((unsigned)n), grid2((unsigned)n, waves);
#define FDH_ADAM7_CASE(BITS)                                                                    \
    case BITS:                                                                                  \
        hipLaunchKernelGGL((fdh::png_adam7_recon_kernel<(int)fdh::png_bpp(BITS)>), grid, block, 0, stream, a); \
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;                   \
        hipLaunchKernelGGL((fdh::png_adam7_place_kernel<BITS>), grid2, block, 0, stream, a);    \
        break;
    switch (bits) {
        FDH_ADAM7_CASE(1)
        FDH_ADAM7_CASE(2)
        FDH_ADAM7_CASE(4)
        FDH_ADAM7_CASE(8)
        FDH_ADAM7_CASE(16)
        FDH_ADAM7_CASE(24)
        FDH_ADAM7_CASE(32)
        FDH_ADAM7_CASE(48)
        FDH_ADAM7_CASE(64)
        default: return -1;
    }
#undef FDH_ADAM7_CASE
    return (int)hipGetLastError();
}
