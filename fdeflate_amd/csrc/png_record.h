// png_record.h -- how the kernels of the mixed batches (png_mixed.hip, png_encode_mixed.hip, the fused encoder's mixed
// instance) read an image's fdh_png_info record: once, through readfirstlane, so that every field is in scalar
// registers and every branch on it is a scalar branch.  Records are not trusted: a kernel asks png_decodable or
// png_encodable itself before it uses a width.
#pragma once
#include "device_common.h"
#include "png_common.h"

namespace fdh {

using PngInfo = fdh_png_info;
static_assert(sizeof(PngInfo) == 32, "fdh_png_info is 32 bytes");

// Record i with every field the same in all lanes as far as the compiler is concerned.
__device__ __forceinline__ PngInfo mixed_record(const PngInfo* info, uint64_t i) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(info + i);
    const uint32_t geom = uni(w[3]);
    PngInfo r;
    r.status = uni(w[0]), r.width = uni(w[1]), r.height = uni(w[2]);
    r.bit_depth = (uint8_t)geom, r.colour_type = (uint8_t)(geom >> 8), r.interlace = (uint8_t)(geom >> 16), r.pad = 0;
    r.idat_bytes = uni(w[4]), r.idat_chunks = uni(w[5]), r.first_idat = uni(w[6]), r.chunks = uni(w[7]);
    return r;
}

__device__ __forceinline__ bool mixed_decodable(const PngInfo& r) {
    return png_decodable(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace);
}

__device__ __forceinline__ bool mixed_encodable(const PngInfo& r) {
    return png_encodable(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace);
}

// What every encode step of a mixed batch starts with: upstream's value where that is not 0, kPngSkipped for a record
// that is not encodable, kPngBadSizes for a geometry the encode steps cannot take (png_encode_sizes), else kPngOk with
// the image's row bytes and packed size.
__device__ __forceinline__ uint32_t mixed_encode_image(const PngInfo& r, const uint32_t* upstream, uint64_t i, uint64_t& row_bytes, uint64_t& pix) {
    row_bytes = pix = 0;
    const uint32_t up = upstream ? uni(upstream[i]) : 0u;
    if (up != 0) return up;
    if (!mixed_encodable(r)) return kPngSkipped;
    return png_encode_sizes(r.width, r.height, r.bit_depth, r.colour_type, row_bytes, pix);
}

}  // namespace fdh
