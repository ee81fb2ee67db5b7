// png_filter_mixed.hip -- fdh_png_filter_mixed_batch (include/fdeflate_hip_png_levels.h): the filtered rows of every
// image of a mixed batch in memory, type byte and all, with the types chosen on the way or given by the caller.  It is
// the step between the packed scanlines and an encoder that is not fused with the filters: the level encoders.  The
// body is png_filter_mixed_body.h (png_choose_body.h's walk, which keeps what it computed); the gate in front of it is
// png_mixed_choose_kernel's: the record once per workgroup through readfirstlane, png_encodable asked here, the lanes
// per row and pieces per row in scalar registers, one instance of the body per filter pixel size and row length.
//
// Statuses.  The launcher clears png_status and the kernel stores only what is not kPngOk: the gate's finding by one
// lane of the image's first workgroup, kPngBadFilterType by whichever band meets such a type (every store of it stores
// the same word).  An image that fails the gate has its filt slot zero-filled where the slot is the size its record
// asks for -- the encoder behind this call reads every slot -- and is left alone where it is not.
#include "device_common.h"
#include "launch.h"
#include "png_common.h"
#include "png_filter_mixed_body.h"
#include "png_record.h"

namespace fdh {

struct MixedFilterArgs {
    const uint8_t* pix;
    const uint64_t* pix_off;    // n + 1
    uint8_t* types;             // given: read; chosen: written, nullable
    const uint64_t* types_off;  // n + 1 (null with types)
    uint8_t* filt;
    const uint64_t* filt_off;   // n + 1
    const PngInfo* info;
    const uint32_t* upstream;   // nullable
    uint32_t* status;           // cleared by the launcher
    uint32_t forced_group;      // FDH_PNG_CHOOSE_LANES, or 0
};

template <bool GIVEN>
__global__ __launch_bounds__(kWave) void png_mixed_filter_kernel(MixedFilterArgs m) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const PngInfo r = mixed_record(m.info, i);
    uint64_t rb, pix_size;
    uint32_t st = mixed_encode_image(r, m.upstream, i, rb, pix_size);
    const uint64_t f0 = uni64(m.filt_off[i]), have_filt = uni64(m.filt_off[i + 1]) - f0;
    uint64_t filt_size = (uint64_t)r.height * (rb + 1);
    if (st != kPngOk) {
        // the slot of an image an earlier step refused: known where the record itself is sound
        uint64_t rb2 = 0, p2 = 0;
        const bool sound = mixed_encodable(r) && png_encode_sizes(r.width, r.height, r.bit_depth, r.colour_type, rb2, p2) == kPngOk;
        filt_size = sound ? (uint64_t)r.height * (rb2 + 1) : ~0ull;
    } else {
        const uint64_t have_pix = uni64(m.pix_off[i + 1] - m.pix_off[i]);
        const uint64_t have_types = m.types ? uni64(m.types_off[i + 1] - m.types_off[i]) : r.height;
        if (have_pix != pix_size || have_types != r.height || have_filt != filt_size) {
            st = kPngBadSizes;
            filt_size = ~0ull;  // (a slot of another size is not touched)
        }
    }
    if (st != kPngOk) {
        if (blockIdx.y == 0 && lane == 0) m.status[i] = st;
        if (have_filt != filt_size) return;
        const uint4 zero = make_uint4(0, 0, 0, 0);
        for (uint64_t o = ((uint64_t)blockIdx.y * kWave + lane) * 16; o < have_filt; o += (uint64_t)gridDim.y * kWave * 16)
            png_store_part(m.filt + f0 + o, zero, (uint32_t)min((uint64_t)16, have_filt - o));
        return;
    }
    // lanes per row and pieces per row exactly as fdh_launch_png_choose has them, in scalar registers
    PngFilterMixedImage a;
    a.pix = m.pix + uni64(m.pix_off[i]);
    a.types = m.types ? m.types + uni64(m.types_off[i]) : nullptr;
    a.filt = m.filt + f0;
    a.status = m.status + i;
    a.rows = r.height;
    a.row_bytes = (uint32_t)rb;  // (below 2^25)
    const uint32_t chunks = (a.row_bytes + 15) / 16;
    uint32_t group = 1;
    while (group < (uint32_t)kWave && group < chunks) group <<= 1;
    if (m.forced_group) group = m.forced_group;
    a.group = group;
    a.pieces = (chunks + group - 1) / group;
#define FDH_MIXED_FILTER_CASE(B)                                                  \
    case B:                                                                       \
        if (a.pieces > 1) png_filter_mixed_image<B, true, GIVEN>(a, lane);        \
        else png_filter_mixed_image<B, false, GIVEN>(a, lane);                    \
        break;
    switch (png_bpp(png_pixel_bits(r.bit_depth, r.colour_type))) {
        FDH_MIXED_FILTER_CASE(1)
        FDH_MIXED_FILTER_CASE(2)
        FDH_MIXED_FILTER_CASE(3)
        FDH_MIXED_FILTER_CASE(4)
        FDH_MIXED_FILTER_CASE(6)
        default: FDH_MIXED_FILTER_CASE(8)
    }
#undef FDH_MIXED_FILTER_CASE
}

}  // namespace fdh

// (the launch shape is fdh_launch_png_choose_mixed's, under the same environment variables)
extern "C" int fdh_launch_png_filter_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                           uint8_t* filt, const uint64_t* filt_off, const fdh_png_info* info, const uint32_t* upstream,
                                           uint32_t flags, uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);  // (the kernel stores only what is not kPngOk)
    if (e != hipSuccess) return (int)e;
    const int v = fdh::env_int("FDH_PNG_CHOOSE_LANES", 0);
    const uint32_t forced = (v >= 1 && v <= fdh::kWave && (v & (v - 1)) == 0) ? (uint32_t)v : 0u;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_CHOOSE_WAVES");
    fdh::MixedFilterArgs a{pix, pix_off, types, types_off, filt, filt_off, info, upstream, status, forced};
    const dim3 grid((unsigned)n, waves), block(fdh::kWave);
    if (flags & FDH_PNG_FILTER_GIVEN_TYPES) hipLaunchKernelGGL(fdh::png_mixed_filter_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(fdh::png_mixed_filter_kernel<false>, grid, block, 0, stream, a);
    return (int)hipGetLastError();
}
