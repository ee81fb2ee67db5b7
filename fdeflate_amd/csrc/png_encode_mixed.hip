// png_encode_mixed.hip -- PNG encode of batches whose pictures differ in width, height, depth and colour type
// (include/fdeflate_hip.h, "PNG encode: mixed batches"): the mirror of png_mixed.hip.  The steps are those of
// png_pack.hip and png_choose.hip, and so is their code (png_pack_body.h, png_choose_body.h): what differs is where the
// geometry comes from.  There it is an argument of the call and a template parameter of the kernel; here it is info[i],
// the 32-byte record of the decode side, of which the encode steps read status, width, height, bit_depth, colour_type
// and interlace.
//
// Dispatch: a workgroup serves one image.  It loads the record once, through readfirstlane (png_record.h), so that every
// value in it -- and the row bytes, lanes per row and pieces per row that follow from it -- is in scalar registers and
// every branch on it is a scalar branch, and switches to the instance of the body that was compiled for the image's
// depth / colour pair (packing: 15) or pixel size and row length (filter selection: 6 x 2).  Such a kernel holds all
// instances and is allocated the registers of the widest one.  Records are not trusted: every kernel asks png_encodable
// itself before it uses a width.  The other two steps that take the record live with the code they share: the fused
// filter + deflate in deflate_ultrafast.hip, the framing with the CRC tables in png_file.hip.
//
// The plan (one record per lane) is the arithmetic of png_common.h and nothing else.
#include "device_common.h"
#include "launch.h"
#include "png_choose_body.h"
#include "png_common.h"
#include "png_pack_body.h"
#include "png_record.h"

namespace fdh {

// ---- fdh_png_encode_plan_batch, fdh_png_encode16_plan_batch ----
struct EncodePlanArgs {
    PngInfo* info;                  // in, out: a dimension record gets its pair
    const uint32_t* colour;         // nullable: word 0 of 4 is the palette's count
    const uint32_t* trns_len;       // nullable
    const uint32_t* summary;        // nullable: counts as 0 (nothing known: RGBA)
    const uint32_t* analyse_status; // nullable: counts as kPngTooManyColours for a dimension record (no palette), kPngOk else
    uint64_t* size[4];              // each nullable: packed, filter types, prefix, file slot
    uint32_t* png_status;           // nullable
    uint64_t n;
    uint32_t allowed;
};

// RGBA16: the pictures are RGBA16 and summary / analyse_status fdh_png_analyse16_mixed_batch's (png_encode16_plan)
template <bool RGBA16>
__global__ __launch_bounds__(256) void png_encode_plan_kernel(EncodePlanArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const PngInfo r = a.info[i];
    const bool have_colour = a.colour && a.trns_len;
    const bool dimension = png_dimension_record(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace);
    uint32_t depth = r.bit_depth, colour = r.colour_type;
    uint64_t s[4];
    const uint32_t count = have_colour ? a.colour[4 * i] : 0u, trns_len = have_colour ? a.trns_len[i] : 0u;
    const uint32_t summary = a.summary ? a.summary[i] : 0u;
    const uint32_t analysed = a.analyse_status ? a.analyse_status[i] : dimension ? kPngTooManyColours : kPngOk;
    const uint32_t st = RGBA16 ? png_encode16_plan(r.status, r.width, r.height, depth, colour, r.interlace, have_colour, count, trns_len, summary,
                                                   analysed, a.allowed, s[0], s[1], s[2], s[3])
                               : png_encode_plan(r.status, r.width, r.height, depth, colour, r.interlace, have_colour, count, trns_len, summary,
                                                 analysed, a.allowed, s[0], s[1], s[2], s[3]);
    if (st == kPngOk && dimension) {
        a.info[i].bit_depth = (uint8_t)depth;
        a.info[i].colour_type = (uint8_t)colour;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (a.size[k]) a.size[k][i] = s[k];
    if (a.png_status) a.png_status[i] = st;
}

// ---- fdh_png_analyse_mixed_batch ----
struct MixedAnalyseArgs {
    PngAnalyseArgs a;  // (its width is filled in per image)
    const PngInfo* info;
    const uint32_t* upstream;  // nullable
};

__global__ __launch_bounds__(kAnalyseMaxThreads) void png_mixed_analyse_kernel(MixedAnalyseArgs m) {
    __shared__ uint32_t table[kAnalyseSlots];
    __shared__ uint32_t keys[256];
    __shared__ uint32_t sh[kAwWords];
    const uint64_t i = blockIdx.x;
    const PngInfo r = mixed_record(m.info, i);
    const uint32_t up = m.upstream ? uni(m.upstream[i]) : 0u;
    const bool known = mixed_encodable(r) || png_dimension_record(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace);
    // (height * width * 4 is below 2^64: both factors are below 2^31)
    const uint32_t st = up != 0 ? up : !known ? kPngSkipped
                        : uni64(m.a.rgba_off[i + 1] - m.a.rgba_off[i]) != (uint64_t)r.height * r.width * 4 ? kPngBadSizes : kPngOk;
    if (st != kPngOk) {
        if (threadIdx.x == 0) m.a.status[i] = st;
        return;
    }
    PngAnalyseArgs a = m.a;
    a.width = r.width;
    png_analyse_image(a, i, table, keys, sh);
}

// ---- fdh_png_pack_mixed_batch ----
struct MixedPackArgs {
    PngPackArgs p;  // (its row_bytes and width are filled in per image)
    const PngInfo* info;
};

__global__ __launch_bounds__(kWave) void png_mixed_pack_kernel(MixedPackArgs m) {
    __shared__ uint32_t pal[256];
    __shared__ uint32_t slot[kPackSlots];  // (touched, and the table built, only by a workgroup whose image is colour type 3)
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const bool first = blockIdx.y == 0 && lane == 0;
    const PngInfo r = mixed_record(m.info, i);
    uint64_t rb, pix_size;
    uint32_t st = mixed_encode_image(r, m.p.upstream, i, rb, pix_size);
    if (st == kPngOk) {
        const uint64_t have_rgba = uni64(m.p.rgba_off[i + 1] - m.p.rgba_off[i]), have_pix = uni64(m.p.pix_off[i + 1] - m.p.pix_off[i]);
        if (have_rgba != (uint64_t)r.height * r.width * 4 || have_pix != pix_size) st = kPngBadSizes;
        else if (r.colour_type == 3 && !m.p.pal) st = kPngBadPlte;
    }
    if (st != kPngOk) {
        if (first) m.p.status[i] = st;
        return;
    }
    PngPackArgs a = m.p;
    a.width = r.width;
    a.row_bytes = rb;
#define FDH_MIXED_PACK_CASE(D, C) \
    case (D) * 8 + (C): png_pack_image<D, C>(a, i, lane, pal, slot); break;
    switch ((uint32_t)r.bit_depth * 8 + r.colour_type) {
        FDH_PNG_FOR_EACH_PAIR(FDH_MIXED_PACK_CASE)
        default: break;  // (png_encodable has let none but the fifteen through)
    }
#undef FDH_MIXED_PACK_CASE
}

// ---- fdh_png_choose_filters_mixed_batch ----
struct MixedChooseArgs {
    PngChooseArgs c;  // (its row_bytes, group and pieces are filled in per image)
    const PngInfo* info;
    const uint32_t* upstream;  // nullable
    uint32_t forced_group;     // FDH_PNG_CHOOSE_LANES, or 0
};

__global__ __launch_bounds__(kWave) void png_mixed_choose_kernel(MixedChooseArgs m) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const PngInfo r = mixed_record(m.info, i);
    uint64_t rb, pix_size;
    uint32_t st = mixed_encode_image(r, m.upstream, i, rb, pix_size);
    if (st == kPngOk) {
        const uint64_t have_pix = uni64(m.c.pix_off[i + 1] - m.c.pix_off[i]), have_types = uni64(m.c.types_off[i + 1] - m.c.types_off[i]);
        if (have_pix != pix_size || have_types != r.height) st = kPngBadSizes;
    }
    if (st != kPngOk) {
        if (blockIdx.y == 0 && lane == 0) m.c.status[i] = st;
        return;
    }
    // lanes per row and pieces per row exactly as fdh_launch_png_choose has them, in scalar registers
    PngChooseArgs a = m.c;
    a.row_bytes = (uint32_t)rb;  // (below 2^25)
    const uint32_t chunks = (a.row_bytes + 15) / 16;
    uint32_t group = 1;
    while (group < (uint32_t)kWave && group < chunks) group <<= 1;
    if (m.forced_group) group = m.forced_group;
    a.group = group;
    a.pieces = (chunks + group - 1) / group;
#define FDH_MIXED_CHOOSE_CASE(B)                                     \
    case B:                                                          \
        if (a.pieces > 1) png_choose_image<B, true>(a, i, lane);     \
        else png_choose_image<B, false>(a, i, lane);                 \
        break;
    switch (png_bpp(png_pixel_bits(r.bit_depth, r.colour_type))) {
        FDH_MIXED_CHOOSE_CASE(1)
        FDH_MIXED_CHOOSE_CASE(2)
        FDH_MIXED_CHOOSE_CASE(3)
        FDH_MIXED_CHOOSE_CASE(4)
        FDH_MIXED_CHOOSE_CASE(6)
        default: FDH_MIXED_CHOOSE_CASE(8)
    }
#undef FDH_MIXED_CHOOSE_CASE
}

}  // namespace fdh

// ---- launchers ----
extern "C" int fdh_launch_png_encode_plan(fdh_png_info* info, const uint32_t* colour, const uint32_t* trns_len, const uint32_t* summary,
                                          const uint32_t* analyse_status, uint32_t allowed, uint64_t* pix_size, uint64_t* types_size,
                                          uint64_t* prefix, uint64_t* file_size, uint32_t* png_status, uint64_t n, int rgba16,
                                          hipStream_t stream) {
    if (n == 0) return 0;
    fdh::EncodePlanArgs a{info, colour, trns_len, summary, analyse_status, {pix_size, types_size, prefix, file_size}, png_status, n, allowed};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (rgba16) hipLaunchKernelGGL(fdh::png_encode_plan_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(fdh::png_encode_plan_kernel<false>, grid, block, 0, stream, a);
    return (int)hipGetLastError();
}

// (the launch shapes are those of fdh_launch_png_analyse, fdh_launch_png_pack and fdh_launch_png_choose, under the same
// environment variables)
extern "C" int fdh_launch_png_analyse_mixed(const uint8_t* rgba, const uint64_t* rgba_off, const fdh_png_info* info, const uint32_t* upstream,
                                            uint32_t* pal, uint32_t* colour, uint32_t* trns_len, uint32_t* summary, uint32_t* status,
                                            uint64_t n, uint32_t max_colours, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t waves = std::min<uint32_t>(fdh::kAnalyseMaxThreads / fdh::kWave, fdh::png_waves_per_image(n, "FDH_PNG_ANALYSE_WAVES"));
    fdh::MixedAnalyseArgs a{{rgba, rgba_off, pal, colour, trns_len, summary, status, n, 0, max_colours}, info, upstream};
    hipLaunchKernelGGL(fdh::png_mixed_analyse_kernel, dim3((unsigned)n), dim3(waves * fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_pack_mixed(const uint8_t* rgba, const uint64_t* rgba_off, uint8_t* pix, const uint64_t* pix_off,
                                         const fdh_png_info* info, const uint32_t* pal, const uint32_t* colour, const uint32_t* upstream,
                                         uint32_t* status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);  // (kPngNotRepresentable is OR-ed in)
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_PACK_WAVES");
    fdh::MixedPackArgs a{{rgba, rgba_off, pix, pix_off, pal, colour, upstream, status, n, 0, 0}, info};
    hipLaunchKernelGGL(fdh::png_mixed_pack_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_choose_mixed(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                           const fdh_png_info* info, const uint32_t* upstream, uint32_t* status, uint64_t n,
                                           hipStream_t stream) {
    if (n == 0) return 0;
    const int v = fdh::env_int("FDH_PNG_CHOOSE_LANES", 0);
    const uint32_t forced = (v >= 1 && v <= fdh::kWave && (v & (v - 1)) == 0) ? (uint32_t)v : 0u;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_CHOOSE_WAVES");
    fdh::MixedChooseArgs a{{pix, pix_off, types, types_off, status, n, 0, 0, 0}, info, upstream, forced};
    hipLaunchKernelGGL(fdh::png_mixed_choose_kernel, dim3((unsigned)n, waves), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}
