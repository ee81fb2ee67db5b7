// png_pack.hip -- PNG encode from RGBA8 (include/fdeflate_hip.h, "PNG encode from RGBA8"): what an RGBA8 image is and
// its sorted palette (fdh_png_analyse_batch), and RGBA8 to the packed scanlines of a depth / colour pair
// (fdh_png_pack_batch), the exact inverse of png_expand.hip.  tests/png_pack_model.py is the authority on every value.
//
// The bodies are png_pack_body.h's (png_encode_mixed.hip runs them with every image's own geometry).
//
// Analysis: one workgroup per image, 1 .. 16 wavefronts.  The distinct pixel words live in an LDS open-addressed table
// (linear probing, insertion by compare-and-swap); a lane reads four pixels with one 16-byte load and probes only for a
// pixel that differs from the one in front of it.  The summary (opaque, grey, sample depth) is three OR-ed difference
// masks and an AND over the words.  Once more than max_colours keys are in, insertion stops and the summary goes on.
// At the end the at most 256 keys are ranked against each other in the LDS and written in ascending order: the result
// does not depend on which lane saw which pixel first.
//
// Packing: one kernel per (bit depth, colour type) pair, grid(n, Y), one wavefront per workgroup that takes the bands
// b, b + Y, .. of kPackBand rows of image i, as png_expand_kernel does.  A lane takes four pixels per step: ONE 16-byte
// load, and a store of the 0.5 .. 32 bytes they pack to.  Rows whose bits fill whole bytes have no padding: a band is
// then ONE run of pixels.  Below eight bits per pixel a lane's four pixels are 4, 8 or 16 bits: two bytes or one are
// stored by the lane itself, and the two halves of a byte of 1-bit pixels meet in the even lane through a DPP move --
// memory is only ever written in whole bytes, each by one lane.  Colour type 3: the workgroup hashes the caller's 256
// palette words into the LDS once (the lowest index of equal words wins) and a lane tries the previous pixel's answer
// before it probes.  A pixel without a lossless representation: one atomicOr per wavefront that saw one.
#include "device_common.h"
#include "launch.h"
#include "png_common.h"
#include "png_pack_body.h"

namespace fdh {

// ---- fdh_png_analyse_batch ----
__global__ __launch_bounds__(kAnalyseMaxThreads) void png_analyse_kernel(PngAnalyseArgs a) {
    __shared__ uint32_t table[kAnalyseSlots];
    __shared__ uint32_t keys[256];
    __shared__ uint32_t sh[kAwWords];
    png_analyse_image(a, blockIdx.x, table, keys, sh);
}

// ---- fdh_png_pack_batch ----
template <int DEPTH, int COLOUR>
__global__ __launch_bounds__(kWave) void png_pack_kernel(PngPackArgs a) {
    __shared__ uint32_t pal[256];
    __shared__ uint32_t slot[COLOUR == 3 ? kPackSlots : 1];
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (a.upstream) {
        const uint32_t up = uni(a.upstream[i]);
        if (up != 0) {
            if (blockIdx.y == 0 && lane == 0) a.status[i] = up;
            return;
        }
    }
    png_pack_image<DEPTH, COLOUR>(a, i, lane, pal, slot);
}

}  // namespace fdh

// One workgroup per image and the set in one LDS: the wavefronts per image are those of the workgroup, 1 .. 16
// (png_waves_per_image: one for a batch that fills the device by its count, more for a small batch of large images);
// FDH_PNG_ANALYSE_WAVES sets it.
extern "C" int fdh_launch_png_analyse(const uint8_t* rgba, const uint64_t* rgba_off, uint32_t* pal, uint32_t* colour, uint32_t* trns_len,
                                      uint32_t* summary, uint32_t* status, uint64_t n, uint32_t width, uint32_t max_colours,
                                      hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t waves = std::min<uint32_t>(fdh::kAnalyseMaxThreads / fdh::kWave, fdh::png_waves_per_image(n, "FDH_PNG_ANALYSE_WAVES"));
    fdh::PngAnalyseArgs a{rgba, rgba_off, pal, colour, trns_len, summary, status, n, width, max_colours};
    hipLaunchKernelGGL(fdh::png_analyse_kernel, dim3((unsigned)n), dim3(waves * fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

// As fdh_launch_png_expand: FDH_PNG_PACK_WAVES sets the wavefronts per image; the statuses start at kPngOk and
// kPngNotRepresentable is OR-ed in.
extern "C" int fdh_launch_png_pack(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off, const uint32_t* pal,
                                   const uint32_t* colour, const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width,
                                   uint64_t row_bytes, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_PACK_WAVES");
    fdh::PngPackArgs a{rgba, rgba_off, pix, pix_off, pal, colour, upstream, status, n, row_bytes, width};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
#define FDH_PACK_CASE(D, C)                                                                \
    case (D) * 8 + (C):                                                                    \
        hipLaunchKernelGGL((fdh::png_pack_kernel<D, C>), grid, block, 0, stream, a);       \
        break;
    switch (bit_depth * 8 + colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_PACK_CASE)
        default: return -1;
    }
#undef FDH_PACK_CASE
    return (int)hipGetLastError();
}
