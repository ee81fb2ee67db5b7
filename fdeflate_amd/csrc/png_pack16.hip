// png_pack16.hip -- RGBA16 to the packed scanlines of the four pairs of depth 16 (include/fdeflate_hip_png16.h,
// fdh_png_pack16_batch): the exact inverse of png_expand16.hip for colour types 0, 2, 4 and 6, samples written
// big-endian.  tests/png16_model.py is the authority on every value.
//
// One kernel per colour type, grid(n, Y), one wavefront per workgroup that takes the bands b, b + Y, .. of kPack16Band
// rows of image i, as png_pack_kernel does.  Every pair has whole bytes per pixel, so a band is ONE run of pixels.  A
// lane takes kPack16Group pixels per step: 16-byte loads, aligned wherever the slot is 8-byte aligned (at most one
// pixel alone in front), the samples that the colour type keeps moved together in registers, both samples of a word
// swapped by one v_perm_b32, and one store of the 2 .. 8 bytes per pixel they pack to -- memory is only ever written in
// whole bytes, each by one lane.  A pixel without a lossless representation (R, G, B not all equal for colour types 0
// and 4, A != 65535 for 0 and 2): one atomicOr per wavefront that saw one.
//
// The body is png_pack16_body.h's (png_encode16_mixed.hip runs it with every image's own geometry).
#include "device_common.h"
#include "launch.h"
#include "png_common.h"
#include "png_pack16_body.h"

namespace fdh {

template <int COLOUR>
__global__ __launch_bounds__(kWave) void png_pack16_kernel(PngPack16Args a) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (a.upstream) {
        const uint32_t up = uni(a.upstream[i]);
        if (up != 0) {
            if (blockIdx.y == 0 && lane == 0) a.status[i] = up;
            return;
        }
    }
    png_pack16_image<COLOUR>(a, i, lane);
}

}  // namespace fdh

// As fdh_launch_png_pack: FDH_PNG_PACK16_WAVES sets the wavefronts per image; the statuses start at kPngOk and
// kPngNotRepresentable is OR-ed in.
extern "C" int fdh_launch_png_pack16(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                                     const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width, uint32_t colour_type,
                                     hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_PACK16_WAVES");
    fdh::PngPack16Args a{rgba16, rgba16_off, pix, pix_off, upstream, status, n, width};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
    switch (colour_type) {
        case 0: hipLaunchKernelGGL((fdh::png_pack16_kernel<0>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((fdh::png_pack16_kernel<2>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((fdh::png_pack16_kernel<4>), grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL((fdh::png_pack16_kernel<6>), grid, block, 0, stream, a); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}
