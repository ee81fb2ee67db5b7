// png_choose.hip -- filter selection (fdh_png_choose_filters_batch): which of the five types each row is filtered with.
//
// The heuristic of the PNG specification (12.8, libpng's default): filter the row with every type,
// read each filtered byte as signed, sum the absolute values (128 counts 128), take the type with the
// smallest sum, the LOWEST type number on equal sums.  With p the predictor as an integer 0..255 the
// cost of a byte x is min(|x - p|, 256 - |x - p|) whichever way the difference wraps.
//
// Filtering uses the raw neighbours, so a row's choice depends on pixel rows r and r - 1 only: no
// skew, no serial walk.  The lanes lie ALONG the row, 16 bytes each.  A row has a group of G lanes
// (a power of two, 1..64), a wavefront works on 64 / G consecutive rows per step and walks down a
// band of kChooseBand rows of one image; the band's bytes are read front to back in runs of whole
// rows.  The row above a group's row is the chunk the group before it holds in the same step (the
// first group: what the last group held one step earlier), fetched with one cross-lane read per
// dword, so a pixel byte is loaded once and serves as "current" and as "above".  The byte `bpp` to
// the left comes from the lane below (DPP shift), not from a second, overlapping load.  Rows wider
// than 16 G bytes (J > 1 pieces per lane) loop along the row and accumulate; they read the row
// above from memory again (the registers cannot hold a row of any length; it is the row the same
// wavefront has just read).
//
// None, Sub, Up and Average are computed four bytes to a word (byte-wise subtraction in a 32-bit
// word, fold of the negative bytes, v_sad_u8 against zero plus the count of sign bits); Paeth byte by
// byte with png_paeth.  A lane's five sums over 16 bytes are at most 2048 each, sixteen lanes' at
// most 32768: two sums share a word for the four reduction steps inside a row of sixteen lanes.
#include "device_common.h"
#include "launch.h"
#include "png_choose_body.h"
#include "png_common.h"
#include "png_rows.h"

namespace fdh {

// (the body: png_choose_body.h, which png_encode_mixed.hip runs at every image's own row size)
template <int BPP, bool LOOP>
__global__ __launch_bounds__(kWave) void png_choose_kernel(PngChooseArgs a) {
    png_choose_image<BPP, LOOP>(a, blockIdx.x, threadIdx.x);
}

}  // namespace fdh

// G = the row's chunks rounded up to a power of two, 64 at most; FDH_PNG_CHOOSE_LANES (1, 2, 4 .. 64) sets it (tests: every
// shape at every width -- narrow groups, one step per row, looped rows, and their combinations).  A wavefront takes the bands
// b, b + Y, .. of its image; Y is chosen so that a small batch of tall images still fills the GPU, FDH_PNG_CHOOSE_WAVES sets it.
extern "C" int fdh_launch_png_choose(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                     uint32_t* status, uint64_t n, uint32_t row_bytes, uint32_t bpp, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t chunks = (row_bytes + 15) / 16;
    uint32_t group = 1;
    while (group < fdh::kWave && group < chunks) group <<= 1;
    const int v = fdh::env_int("FDH_PNG_CHOOSE_LANES", 0);
    if (v >= 1 && v <= fdh::kWave && (v & (v - 1)) == 0) group = (uint32_t)v;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_CHOOSE_WAVES");
    const uint32_t pieces = (chunks + group - 1) / group;
    fdh::PngChooseArgs a{pix, pix_off, types, types_off, status, n, row_bytes, group, pieces};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
#define FDH_PNG_CASE(B)                                                                           \
    case B:                                                                                       \
        if (pieces > 1) hipLaunchKernelGGL((fdh::png_choose_kernel<B, true>), grid, block, 0, stream, a); \
        else hipLaunchKernelGGL((fdh::png_choose_kernel<B, false>), grid, block, 0, stream, a);   \
        break;
    switch (bpp) {
        FDH_PNG_CASE(1)
        FDH_PNG_CASE(2)
        FDH_PNG_CASE(3)
        FDH_PNG_CASE(4)
        FDH_PNG_CASE(6)
        FDH_PNG_CASE(8)
        default: return -1;
    }
#undef FDH_PNG_CASE
    return (int)hipGetLastError();
}
