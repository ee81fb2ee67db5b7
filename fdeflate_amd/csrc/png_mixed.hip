// png_mixed.hip -- PNG decode of batches whose files differ in width, depth, colour type and interlace method
// (include/fdeflate_hip.h, "PNG decode: mixed batches").  The steps are those of png_file.hip, png_adam7.hip and
// png_expand.hip, and so is their code (png_chunks.h, png_adam7_body.h, png_expand_body.h): what differs is where the
// geometry comes from.  There it is an argument of the call and a template parameter of the kernel; here it is
// info[i], a 32-byte record per image that the container scan wrote or the caller made.
//
// Dispatch: a workgroup serves one image.  It loads the record once, through readfirstlane, so that every value in
// it is in scalar registers and every branch on it is a scalar branch, and switches to the instance of the body that
// was compiled for the image's pixel size (reconstruction: 6, placement: 9) or depth / colour pair (expansion: 15).
// Such a kernel holds all instances and is allocated the registers of the widest one; profiles/png_mixed_kres.txt
// has the numbers.  Records are not trusted: every kernel asks png_decodable itself before it uses a width.
//
// The plan (one record per lane) is the arithmetic of png_common.h and nothing else.
#include "device_common.h"
#include "launch.h"
#include "png_adam7_body.h"
#include "png_chunks.h"
#include "png_common.h"
#include "png_expand_body.h"

namespace fdh {

// (mixed_record and mixed_decodable: png_record.h, shared with the encode side's mixed batches)

// ---- fdh_png_plan_batch ----
struct PlanArgs {
    const PngInfo* info;
    uint64_t max_bytes;
    uint64_t* size[4];  // each nullable: compressed, filtered, packed, RGBA8
    uint32_t* png_status;
    uint64_t n;
};

__global__ __launch_bounds__(256) void png_plan_kernel(PlanArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const PngInfo r = a.info[i];
    uint64_t s[4];
    const uint32_t st = png_plan(r, a.max_bytes, s[0], s[1], s[2], s[3]);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (a.size[k]) a.size[k][i] = s[k];
    a.png_status[i] = st;
}

// ---- fdh_png_gather_idat_mixed_batch, fdh_png_colour_mixed_batch ----
struct MixedGatherArgs {
    GatherArgs g;              // (its width, bit_depth and colour_type are not used)
    const uint32_t* upstream;  // nullable
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void png_mixed_gather_kernel(MixedGatherArgs a) {
    const uint64_t i = blockIdx.x;
    const PngInfo r = mixed_record(a.g.info, i);
    const uint64_t room = a.g.comp_off[i + 1] - a.g.comp_off[i];
    const uint32_t up = a.upstream ? uni(a.upstream[i]) : 0u;
    uint32_t st = kPngOk;
    if (up != 0) st = up;
    else if (!mixed_decodable(r)) st = kPngSkipped;
    else if (r.idat_bytes > room) st = kPngCompSlotTooSmall;
    png_gather_file<THREADS>(a.g, i, r, st);
}

struct MixedColourArgs {
    ColourArgs c;              // (pal is required; width, bit_depth and colour_type are not used)
    const uint32_t* upstream;  // nullable
};

__global__ __launch_bounds__(kWave) void png_mixed_colour_kernel(MixedColourArgs a) {
    const uint64_t i = blockIdx.x;
    const PngInfo r = mixed_record(a.c.info, i);
    const uint32_t up = a.upstream ? uni(a.upstream[i]) : 0u;
    const uint32_t st = up != 0 ? up : mixed_decodable(r) ? kPngOk : kPngSkipped;
    png_colour_file(a.c, i, threadIdx.x, r, r.colour_type, st);
}

// ---- fdh_png_unfilter_mixed_batch ----
struct MixedRowsArgs {
    uint8_t* filt;
    const uint64_t* filt_off;  // n + 1
    uint8_t* pix;
    const uint64_t* pix_off;   // n + 1
    const PngInfo* info;
    const uint32_t* upstream;      // nullable: the decoder's status
    const uint32_t* upstream_len;  // nullable: the decoder's out_len
    uint32_t* status;
    uint64_t n;
};

// Image i as png_adam7_body.h wants it: the call's arguments with the image's own geometry, and what adam7_image
// finds out -- here from the record, whose sizes (png_plan) the two slots must have exactly.
__device__ __forceinline__ void mixed_rows_image(const MixedRowsArgs& m, uint64_t i, Adam7Args& a, Adam7Image& g) {
    const PngInfo r = mixed_record(m.info, i);
    const uint64_t f1 = m.filt_off[i + 1], d1 = m.pix_off[i + 1];
    g.f0 = m.filt_off[i];
    g.d0 = m.pix_off[i];
    g.method = r.interlace;
    g.height = r.height;
    g.status = kPngOk;
    uint32_t bits = 8;
    if (m.upstream && m.upstream[i] != 0) g.status = kPngSkipped;
    else if (!mixed_decodable(r)) g.status = kPngSkipped;
    else {
        bits = png_pixel_bits(r.bit_depth, r.colour_type);
        uint64_t comp, filt, pix, rgba;
        const uint32_t planned = png_plan(r, 0, comp, filt, pix, rgba);
        if (m.upstream_len && (uint64_t)m.upstream_len[i] != f1 - g.f0) g.status = kPngBadSizes;
        else if (planned != kPngOk || filt != f1 - g.f0 || pix != d1 - g.d0) g.status = kPngBadSizes;
    }
    a = Adam7Args{m.filt, m.filt_off, m.pix, m.pix_off, nullptr, m.upstream, m.upstream_len, m.status, m.n,
                  png_row_bytes(r.width, bits), r.width, bits};
}

__global__ __launch_bounds__(kWave) void png_mixed_recon_kernel(MixedRowsArgs m) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    Adam7Args a;
    Adam7Image g;
    mixed_rows_image(m, i, a, g);
    switch (g.status == kPngOk ? png_bpp(a.bits) : 1u) {  // (an image that is refused: any instance writes its status)
        case 1: adam7_recon_image<1>(a, g, i, lane); break;
        case 2: adam7_recon_image<2>(a, g, i, lane); break;
        case 3: adam7_recon_image<3>(a, g, i, lane); break;
        case 4: adam7_recon_image<4>(a, g, i, lane); break;
        case 6: adam7_recon_image<6>(a, g, i, lane); break;
        default: adam7_recon_image<8>(a, g, i, lane); break;
    }
}

__global__ __launch_bounds__(kWave) void png_mixed_place_kernel(MixedRowsArgs m) {
    __shared__ uint64_t s_base[7], s_stride[7];
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (uni(m.status[i]) > kPngBadFilterType) return;  // (refused by the reconstruction kernel: nothing is written)
    Adam7Args a;
    Adam7Image g;
    mixed_rows_image(m, i, a, g);
    if (g.status != kPngOk) return;
    switch (a.bits) {
        case 1: adam7_place_image<1>(a, g, lane, s_base, s_stride); break;
        case 2: adam7_place_image<2>(a, g, lane, s_base, s_stride); break;
        case 4: adam7_place_image<4>(a, g, lane, s_base, s_stride); break;
        case 8: adam7_place_image<8>(a, g, lane, s_base, s_stride); break;
        case 16: adam7_place_image<16>(a, g, lane, s_base, s_stride); break;
        case 24: adam7_place_image<24>(a, g, lane, s_base, s_stride); break;
        case 32: adam7_place_image<32>(a, g, lane, s_base, s_stride); break;
        case 48: adam7_place_image<48>(a, g, lane, s_base, s_stride); break;
        default: adam7_place_image<64>(a, g, lane, s_base, s_stride); break;
    }
}

// ---- fdh_png_expand_mixed_batch ----
struct MixedExpandArgs {
    PngExpandArgs e;  // (its row_bytes and width are filled in per image)
    const PngInfo* info;
};

// Image blockIdx.x at OPX bytes per output pixel: 4 RGBA8, 8 RGBA16 (png_expand_body.h)
template <int OPX>
__device__ __forceinline__ void mixed_expand_image(const MixedExpandArgs& m, uint32_t* pal) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const bool first = blockIdx.y == 0 && lane == 0;
    const uint32_t up = m.e.upstream ? uni(m.e.upstream[i]) : 0u;
    const PngInfo r = mixed_record(m.info, i);
    // (an image that is skipped may have a record that is not decodable: its upstream value wins)
    const uint32_t st = up != 0 ? up : !mixed_decodable(r) ? kPngSkipped : (r.colour_type == 3 && !m.e.pal) ? kPngBadPlte : kPngOk;
    if (st != kPngOk) {
        if (first) m.e.status[i] = st;
        return;
    }
    PngExpandArgs a = m.e;
    a.width = r.width;
    a.row_bytes = png_row_bytes(r.width, png_pixel_bits(r.bit_depth, r.colour_type));
#define FDH_MIXED_EXPAND_CASE(D, C) \
    case (D) * 8 + (C): png_expand_image<D, C, OPX>(a, i, lane, pal); break;
    switch ((uint32_t)r.bit_depth * 8 + r.colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_MIXED_EXPAND_CASE)
        default: break;  // (png_decodable has let none but the fifteen through)
    }
#undef FDH_MIXED_EXPAND_CASE
}

__global__ __launch_bounds__(kWave) void png_mixed_expand_kernel(MixedExpandArgs m) {
    __shared__ uint32_t pal[256];
    mixed_expand_image<4>(m, pal);
}

// ---- fdh_png_expand16_mixed_batch (include/fdeflate_hip_png16.h) ----
__global__ __launch_bounds__(kWave) void png_mixed_expand16_kernel(MixedExpandArgs m) {
    __shared__ uint32_t pal[256];
    mixed_expand_image<8>(m, pal);
}

}  // namespace fdh

// ---- launchers ----
extern "C" int fdh_launch_png_plan(const fdh_png_info* info, uint64_t max_bytes, uint64_t* comp_size, uint64_t* filt_size,
                                   uint64_t* pix_size, uint64_t* rgba_size, uint32_t* png_status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    fdh::PlanArgs a{info, max_bytes, {comp_size, filt_size, pix_size, rgba_size}, png_status, n};
    hipLaunchKernelGGL(fdh::png_plan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}

// (the launch shapes are those of fdh_launch_png_gather and fdh_launch_png_colour)
extern "C" int fdh_launch_png_gather_mixed(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info,
                                           const uint32_t* upstream, uint8_t* comp, const uint64_t* comp_off, uint32_t* comp_len,
                                           uint32_t* png_status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    fdh::MixedGatherArgs a{{file, file_off, info, comp, comp_off, comp_len, png_status, n, 0, 0, 0}, upstream};
    if (n >= fdh::kFillWaves) hipLaunchKernelGGL((fdh::png_mixed_gather_kernel<64>), dim3((unsigned)n), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((fdh::png_mixed_gather_kernel<256>), dim3((unsigned)n), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_colour_mixed(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info,
                                           const uint32_t* upstream, uint32_t* pal, uint32_t* colour, uint32_t* png_status, uint64_t n,
                                           hipStream_t stream) {
    if (n == 0) return 0;
    fdh::MixedColourArgs a{{file, file_off, info, pal, colour, png_status, n, 0, 0, 0}, upstream};
    hipLaunchKernelGGL(fdh::png_mixed_colour_kernel, dim3((unsigned)n), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

// Reconstruction: one wavefront per image.  Placement and expansion: Y wavefronts per image as in fdh_launch_png_adam7 and
// fdh_launch_png_expand, under the same environment variables.
extern "C" int fdh_launch_png_unfilter_mixed(uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off,
                                             const fdh_png_info* info, const uint32_t* upstream, const uint32_t* upstream_len,
                                             uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_ADAM7_WAVES");
    fdh::MixedRowsArgs a{filt, filt_off, pix, pix_off, info, upstream, upstream_len, status, n};
    hipLaunchKernelGGL(fdh::png_mixed_recon_kernel, dim3((unsigned)n), dim3(fdh::kWave), 0, stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fdh::png_mixed_place_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_expand_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba, const uint64_t* rgba_off,
                                           const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour,
                                           const uint32_t* upstream, uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);  // (kPngIndexOutsidePalette is OR-ed in)
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_EXPAND_WAVES");
    fdh::MixedExpandArgs a{{pix, pix_off, rgba, rgba_off, pal, colour, upstream, status, n, 0, 0}, info};
    hipLaunchKernelGGL(fdh::png_mixed_expand_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

// (FDH_PNG_EXPAND16_WAVES, as fdh_launch_png_expand16)
extern "C" int fdh_launch_png_expand16_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* rgba16, const uint64_t* rgba16_off,
                                             const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour,
                                             const uint32_t* upstream, uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_EXPAND16_WAVES");
    fdh::MixedExpandArgs a{{pix, pix_off, rgba16, rgba16_off, pal, colour, upstream, status, n, 0, 0}, info};
    hipLaunchKernelGGL(fdh::png_mixed_expand16_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}
