// png_encode16_mixed.hip -- the front of the PNG encode of mixed batches for RGBA16 pictures
// (include/fdeflate_hip_png16_encode.h): what a picture is and which pixels it has (fdh_png_analyse16_mixed_batch), and
// its packed scanlines in any of the fifteen depth / colour pairs (fdh_png_pack16_mixed_batch).  The shape is
// png_encode_mixed.hip's: a workgroup serves one image, loads its record once through readfirstlane (png_record.h) and
// switches to the instance of the body that was compiled for the image's pair.  The bodies are the ones the other calls
// run: png_analyse_image and png_pack_image of png_pack_body.h with the pixel source of eight bytes (PixelSource<8>: two
// 16-byte loads for a lane's four pixels, the narrow test on every word of two samples, the four high bytes moved
// together by one v_perm_b32), and png_pack16_image of png_pack16_body.h for depth 16.  The plan of these batches is
// png_encode_mixed.hip's plan kernel with png_common.h's png_encode16_plan.  tests/png16_encode_model.py is the
// authority on every value.
#include "device_common.h"
#include "launch.h"
#include "png_common.h"
#include "png_pack16_body.h"
#include "png_pack_body.h"
#include "png_record.h"

namespace fdh {

// ---- fdh_png_analyse16_mixed_batch ----
struct MixedAnalyse16Args {
    PngAnalyseArgs a;  // (rgba: the RGBA16 pictures; its width is filled in per image)
    const PngInfo* info;
    const uint32_t* upstream;  // nullable
};

__global__ __launch_bounds__(kAnalyseMaxThreads) void png_mixed_analyse16_kernel(MixedAnalyse16Args m) {
    __shared__ uint32_t table[kAnalyseSlots];
    __shared__ uint32_t keys[256];
    __shared__ uint32_t sh[kAwWords16];
    const uint64_t i = blockIdx.x;
    const PngInfo r = mixed_record(m.info, i);
    const uint32_t up = m.upstream ? uni(m.upstream[i]) : 0u;
    const bool known = mixed_encodable(r) || png_dimension_record(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace);
    const uint64_t o0 = uni64(m.a.rgba_off[i]), o1 = uni64(m.a.rgba_off[i + 1]);
    // (height * width * 8 is below 2^64: both factors are below 2^31)
    const bool fits = o1 - o0 == (uint64_t)r.height * r.width * 8 && (reinterpret_cast<uintptr_t>(m.a.rgba + o0) & 1) == 0;
    const uint32_t st = up != 0 ? up : !known ? kPngSkipped : !fits ? kPngBadSizes : kPngOk;
    if (st != kPngOk) {
        if (threadIdx.x == 0) m.a.status[i] = st;
        return;
    }
    PngAnalyseArgs a = m.a;
    a.width = r.width;
    png_analyse_image<8>(a, i, table, keys, sh);
}

// ---- fdh_png_pack16_mixed_batch ----
struct MixedPack16Args {
    PngPackArgs p;  // (rgba: the RGBA16 pictures; its row_bytes and width are filled in per image)
    const PngInfo* info;
};

template <int DEPTH, int COLOUR>
__device__ __forceinline__ void png_pack16_any(const PngPackArgs& a, uint64_t i, uint32_t lane, uint32_t* pal, uint32_t* slot) {
    if constexpr (DEPTH == 16) {
        const PngPack16Args w{a.rgba, a.rgba_off, a.pix, a.pix_off, nullptr, a.status, a.n, a.width};
        png_pack16_image<COLOUR>(w, i, lane);
    } else {
        png_pack_image<DEPTH, COLOUR, 8>(a, i, lane, pal, slot);
    }
}

__global__ __launch_bounds__(kWave) void png_mixed_pack16_kernel(MixedPack16Args m) {
    __shared__ uint32_t pal[256];
    __shared__ uint32_t slot[kPackSlots];  // (touched, and the table built, only by a workgroup whose image is colour type 3)
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const bool first = blockIdx.y == 0 && lane == 0;
    const PngInfo r = mixed_record(m.info, i);
    uint64_t rb, pix_size;
    uint32_t st = mixed_encode_image(r, m.p.upstream, i, rb, pix_size);
    if (st == kPngOk) {
        const uint64_t o0 = uni64(m.p.rgba_off[i]), have_rgba = uni64(m.p.rgba_off[i + 1]) - o0;
        const uint64_t have_pix = uni64(m.p.pix_off[i + 1] - m.p.pix_off[i]);
        if (have_rgba != (uint64_t)r.height * r.width * 8 || have_pix != pix_size || (reinterpret_cast<uintptr_t>(m.p.rgba + o0) & 1) != 0)
            st = kPngBadSizes;
        else if (r.colour_type == 3 && !m.p.pal) st = kPngBadPlte;
    }
    if (st != kPngOk) {
        if (first) m.p.status[i] = st;
        return;
    }
    PngPackArgs a = m.p;
    a.width = r.width;
    a.row_bytes = rb;
#define FDH_MIXED_PACK16_CASE(D, C) \
    case (D) * 8 + (C): png_pack16_any<D, C>(a, i, lane, pal, slot); break;
    switch ((uint32_t)r.bit_depth * 8 + r.colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_MIXED_PACK16_CASE)
        default: break;  // (png_encodable has let none but the fifteen through)
    }
#undef FDH_MIXED_PACK16_CASE
}

}  // namespace fdh

// ---- launchers ----
// (the launch shapes are those of fdh_launch_png_analyse_mixed and fdh_launch_png_pack16, under the same environment
// variables)
extern "C" int fdh_launch_png_analyse16_mixed(const uint8_t* rgba16, const uint64_t* rgba16_off, const fdh_png_info* info,
                                              const uint32_t* upstream, uint32_t* pal, uint32_t* colour, uint32_t* trns_len,
                                              uint32_t* summary, uint32_t* status, uint64_t n, uint32_t max_colours, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t waves = std::min<uint32_t>(fdh::kAnalyseMaxThreads / fdh::kWave, fdh::png_waves_per_image(n, "FDH_PNG_ANALYSE_WAVES"));
    fdh::MixedAnalyse16Args a{{rgba16, rgba16_off, pal, colour, trns_len, summary, status, n, 0, max_colours}, info, upstream};
    hipLaunchKernelGGL(fdh::png_mixed_analyse16_kernel, dim3((unsigned)n), dim3(waves * fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_pack16_mixed(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                                           const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                           uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);  // (kPngNotRepresentable is OR-ed in)
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_PACK16_WAVES");
    fdh::MixedPack16Args a{{rgba16, rgba16_off, pix, pix_off, pal, colour, upstream, status, n, 0, 0}, info};
    hipLaunchKernelGGL(fdh::png_mixed_pack16_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}
