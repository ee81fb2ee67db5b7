// png_common.h -- what every part of the PNG layer agrees on, once, for host and device code: the legal depth / colour
// pairs, the sizes that follow from a geometry, the Adam7 pass tables with the size of an interlaced stream, and the
// per-image status values.  Nothing here touches the device: the header compiles in a plain C++ program as well.
#pragma once
#include <stdint.h>

#include "../../include/fdeflate_hip.h"  // FDH_PNG_STATUS_*: the public names of the status values

#if defined(__HIPCC__)
#define FDH_PNG_FN __host__ __device__ __forceinline__ constexpr
#else
#define FDH_PNG_FN inline constexpr
#endif

namespace fdh {

// ---- per-image status values (include/fdeflate_hip.h describes them call by call) ----
// the row calls: a filter type above 4; slots that do not fit the geometry (or each other); refused by an earlier step
constexpr uint32_t kPngOk = 0, kPngBadFilterType = 1, kPngBadSizes = 2, kPngSkipped = 3;
// info.status of the container scan: the first finding in file order
constexpr uint32_t kPngScanNoSignature = 1, kPngScanTruncated = 2, kPngScanBadIhdr = 3, kPngScanInterlaced = 4;
constexpr uint32_t kPngScanChunkStructure = 5, kPngScanCrcMismatch = 6;
// the decode steps behind the scan: the file's geometry is not the call's; the gather's destination; OR-ed into kPngOk by the expansion
constexpr uint32_t kPngOtherGeometry = 7, kPngCompSlotTooSmall = 8, kPngIndexOutsidePalette = 9, kPngBadPlte = 10, kPngBadTrns = 11;
// the encode steps in front of the filters: more distinct colours than the call allows; a pixel the pair cannot hold (OR-ed into kPngOk)
constexpr uint32_t kPngTooManyColours = 12, kPngNotRepresentable = 13;

static_assert(kPngOk == FDH_PNG_STATUS_OK && kPngBadFilterType == FDH_PNG_STATUS_BAD_FILTER_TYPE && kPngBadSizes == FDH_PNG_STATUS_BAD_SIZES &&
              kPngSkipped == FDH_PNG_STATUS_SKIPPED && kPngScanNoSignature == FDH_PNG_STATUS_SCAN_NO_SIGNATURE &&
              kPngScanTruncated == FDH_PNG_STATUS_SCAN_TRUNCATED && kPngScanBadIhdr == FDH_PNG_STATUS_SCAN_BAD_IHDR &&
              kPngScanInterlaced == FDH_PNG_STATUS_SCAN_INTERLACED && kPngScanChunkStructure == FDH_PNG_STATUS_SCAN_CHUNK_STRUCTURE &&
              kPngScanCrcMismatch == FDH_PNG_STATUS_SCAN_CRC_MISMATCH && kPngOtherGeometry == FDH_PNG_STATUS_OTHER_GEOMETRY &&
              kPngCompSlotTooSmall == FDH_PNG_STATUS_COMP_SLOT_TOO_SMALL && kPngIndexOutsidePalette == FDH_PNG_STATUS_INDEX_OUTSIDE_PALETTE &&
              kPngBadPlte == FDH_PNG_STATUS_BAD_PLTE && kPngBadTrns == FDH_PNG_STATUS_BAD_TRNS &&
              kPngTooManyColours == FDH_PNG_STATUS_TOO_MANY_COLOURS && kPngNotRepresentable == FDH_PNG_STATUS_NOT_REPRESENTABLE, "the public header names the same values");

// ---- geometry ----
// the fifteen depth / colour-type pairs of the PNG specification (11.2.2, table 11.1): X(depth, colour) for each, in the order of
// every switch over them
#define FDH_PNG_FOR_EACH_PAIR(X) X(1, 0) X(2, 0) X(4, 0) X(8, 0) X(16, 0) X(8, 2) X(16, 2) \
                                 X(1, 3) X(2, 3) X(4, 3) X(8, 3) X(8, 4) X(16, 4) X(8, 6) X(16, 6)
FDH_PNG_FN bool png_pair_ok(uint32_t depth, uint32_t colour) {
    switch (colour) {
        case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
        case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
        case 2:
        case 4:
        case 6: return depth == 8 || depth == 16;
        default: return false;
    }
}
FDH_PNG_FN uint32_t png_channels(uint32_t colour) { return colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 1; }
FDH_PNG_FN uint32_t png_pixel_bits(uint32_t depth, uint32_t colour) { return png_channels(colour) * depth; }
// bytes of a packed row of `width` pixels of `bits` bits (the last byte padded)
FDH_PNG_FN uint64_t png_row_bytes(uint64_t width, uint64_t bits) { return (width * bits + 7) / 8; }
// the pixel size of the filters: whole bytes, 1 for the narrower pixels (PNG specification 9.2)
FDH_PNG_FN uint32_t png_bpp(uint32_t bits) { return bits >= 8 ? bits / 8 : 1; }

// ---- Adam7 (PNG specification 8.2) ----
// The pass tables, pass p in nibble p: first column and row, log2 of the column and row steps.
constexpr uint32_t kAdam7X0 = 0x0102040u, kAdam7Y0 = 0x1020400u, kAdam7LogDx = 0x0112233u, kAdam7LogDy = 0x1122333u;
FDH_PNG_FN uint32_t adam7_nib(uint32_t table, uint32_t p) { return (table >> (4 * p)) & 15u; }

// Width and height of pass p of a width x height image (method 0: one pass, the image itself); 0 x 0 if it is empty.
FDH_PNG_FN void adam7_pass_dims(uint32_t method, uint32_t p, uint64_t width, uint64_t height, uint64_t& pw, uint64_t& ph) {
    if (method == 0) {
        pw = p == 0 ? width : 0;
        ph = p == 0 ? height : 0;
    } else {
        const uint32_t x0 = adam7_nib(kAdam7X0, p), y0 = adam7_nib(kAdam7Y0, p), lx = adam7_nib(kAdam7LogDx, p), ly = adam7_nib(kAdam7LogDy, p);
        pw = width > x0 ? (width - x0 + (1u << lx) - 1) >> lx : 0;
        ph = height > y0 ? (height - y0 + (1u << ly) - 1) >> ly : 0;
    }
    if (pw == 0 || ph == 0) pw = ph = 0;
}

// The bytes the IDAT stream of a width x height image of `bits` bits per pixel decodes to: every row of every pass
// with its type byte (method 1), or height * (1 + row bytes) (method 0).  An empty pass has no bytes.  adam7_image
// (png_adam7_body.h) checks every slot against this sum, written out there from the same adam7_pass_dims and png_row_bytes.
FDH_PNG_FN uint64_t png_adam7_size(uint32_t width, uint64_t height, uint32_t bits, uint32_t method) {
    uint64_t total = 0;
    for (uint32_t p = 0; p < 7; p++) {
        uint64_t pw = 0, ph = 0;
        adam7_pass_dims(method, p, width, height, pw, ph);
        total += ph * (1 + png_row_bytes(pw, bits));
    }
    return total;
}

// ---- mixed batches: the geometry is each image's own, read from its fdh_png_info record ----
// A record the decode steps can work with: the scan found nothing (or the caller says so), and the IHDR values are
// ones the specification allows.  Records need not come from the scan, so every kernel asks this itself.
FDH_PNG_FN bool png_decodable(uint32_t status, uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, uint32_t interlace) {
    return status == kPngOk && width >= 1 && width <= 0x7FFFFFFFu && height >= 1 && height <= 0x7FFFFFFFu && png_pair_ok(depth, colour) &&
           interlace <= 1;
}

// The four buffer sizes of an image -- compressed (idat_bytes), filtered (what the IDAT stream decodes to), packed
// scanlines, RGBA8 -- and whether a pipeline can take it: kPngSkipped for a record that is not decodable,
// kPngBadSizes for a filtered size of 2^32 or more (a decoder slot cannot hold it) or, with max_bytes != 0, a
// largest size above max_bytes; all four sizes are 0 then.  Nothing wraps: with row_bytes below 2^32 every product
// stays below 2^63 and the seven passes have fewer than 2^32 rows together; with row_bytes of 2^32 or more the
// filtered size is out of range whatever the height (it exceeds the packed size in both layouts: every picture row
// has at least one pass row, with a type byte, that starts in it).
FDH_PNG_FN uint32_t png_plan(uint32_t status, uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, uint32_t interlace,
                             uint32_t idat_bytes, uint64_t max_bytes, uint64_t& comp, uint64_t& filt, uint64_t& pix, uint64_t& rgba) {
    comp = filt = pix = rgba = 0;
    if (!png_decodable(status, width, height, depth, colour, interlace)) return kPngSkipped;
    const uint32_t bits = png_pixel_bits(depth, colour);
    const uint64_t rb = png_row_bytes(width, bits);
    if (rb >> 32) return kPngBadSizes;
    const uint64_t f = png_adam7_size(width, height, bits, interlace);
    if (f >> 32) return kPngBadSizes;
    const uint64_t p = (uint64_t)height * rb, r = (uint64_t)height * width * 4;
    uint64_t largest = idat_bytes;
    if (f > largest) largest = f;
    if (p > largest) largest = p;
    if (r > largest) largest = r;
    if (max_bytes != 0 && largest > max_bytes) return kPngBadSizes;
    comp = idat_bytes, filt = f, pix = p, rgba = r;
    return kPngOk;
}
FDH_PNG_FN uint32_t png_plan(const fdh_png_info& r, uint64_t max_bytes, uint64_t& comp, uint64_t& filt, uint64_t& pix, uint64_t& rgba) {
    return png_plan(r.status, r.width, r.height, r.bit_depth, r.colour_type, r.interlace, r.idat_bytes, max_bytes, comp, filt, pix, rgba);
}

// ---- encode: mixed batches (include/fdeflate_hip.h, "PNG encode: mixed batches") ----
// A record the encode steps can work with: as png_decodable, without interlacing (interlaced writing does not exist).
FDH_PNG_FN bool png_encodable(uint32_t status, uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, uint32_t interlace) {
    return interlace == 0 && png_decodable(status, width, height, depth, colour, interlace);
}
// A record that says only how large the picture is: depth 0 and colour type 0 mean "choose for me" (png_encode_plan does).
FDH_PNG_FN bool png_dimension_record(uint32_t status, uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, uint32_t interlace) {
    return status == kPngOk && width >= 1 && width <= 0x7FFFFFFFu && height >= 1 && height <= 0x7FFFFFFFu && depth == 0 && colour == 0 &&
           interlace == 0;
}

// fdh_ultrafast_bound: the largest stream the ultra-fast encoder makes of `len` bytes
FDH_PNG_FN uint64_t png_ultrafast_bound(uint64_t len) { return 53 + (5 + 12 * len + 12 + 7) / 8 + 4; }

// The bytes of a file in front of its zlib stream: signature, IHDR and the IDAT's head (41), and for colour type 3 a PLTE
// of exactly `count` entries and, where there are alphas, a tRNS of exactly `trns_len` bytes.  The plan, the framing, the
// IDAT's CRC pass and the finishing kernel all ask here.
constexpr uint32_t kPngFilePrefix = FDH_PNG_FILE_PREFIX, kPngFileSuffix = FDH_PNG_FILE_SUFFIX;
FDH_PNG_FN uint32_t png_encode_prefix(uint32_t colour, uint32_t count, uint32_t trns_len) {
    return colour == 3 ? kPngFilePrefix + 12 + 3 * count + (trns_len ? 12 + trns_len : 0) : kPngFilePrefix;
}

// Row bytes and packed size of an encodable geometry, and whether the encode steps can take it: kPngBadSizes for
// row_bytes of 2^25 or more (a row's filter cost is summed in 32 bits) or a filtered size height * (row_bytes + 1) of
// 2^31 or more (the fused encoder's limit); both sizes are 0 then.  Nothing wraps: row_bytes is below 2^34, and it is
// below 2^25 before it is multiplied.
FDH_PNG_FN uint32_t png_encode_sizes(uint32_t width, uint32_t height, uint32_t depth, uint32_t colour, uint64_t& row_bytes, uint64_t& pix) {
    row_bytes = pix = 0;
    const uint64_t rb = png_row_bytes(width, png_pixel_bits(depth, colour));
    if (rb >= (1ull << 25) || (uint64_t)height * (rb + 1) >= (1ull << 31)) return kPngBadSizes;
    row_bytes = rb, pix = (uint64_t)height * rb;
    return kPngOk;
}

// The encode plan of one image: the pair for a dimension record (written to depth / colour where the status is kPngOk),
// and the four sizes -- packed scanlines, filter types, prefix, file slot -- of the pair.  have_colour: count and
// trns_len are known (the palette's entries, and how many of them have A < 255); summary and analyse_status are
// fdh_png_analyse_batch's; allowed: bit c set = colour type c may be chosen, 0 = all five.
//   candidates   grey (0, d): summary bits 0 and 1, d the summary's depth; palette (3, p): analyse_status 0, count in
//                1 .. 256, trns_len <= count, p the smallest of 1, 2, 4, 8 with 2^p >= count; grey-alpha (4, 8): bit 1;
//                RGB (2, 8): bit 0; RGBA (6, 8) always
//   cost         height * row_bytes, for the palette + 12 + 3 count + (trns_len ? 12 + trns_len : 0): the smallest wins,
//                the lower colour type on equal cost (below 2^64: 32 bits per pixel at the most)
// status: kPngSkipped the record is of neither kind; analyse_status where it is neither 0 nor kPngTooManyColours;
// kPngNotRepresentable no candidate is left; kPngBadPlte / kPngBadTrns an encodable record of colour type 3 without
// count (or with one outside 1 .. 2^depth) / with trns_len above count; kPngBadSizes png_encode_sizes refuses the pair.
// All four sizes are 0 unless the status is kPngOk.
FDH_PNG_FN uint32_t png_encode_plan(uint32_t status, uint32_t width, uint32_t height, uint32_t& depth, uint32_t& colour, uint32_t interlace,
                                    bool have_colour, uint32_t count, uint32_t trns_len, uint32_t summary, uint32_t analyse_status,
                                    uint32_t allowed, uint64_t& pix, uint64_t& types, uint64_t& prefix, uint64_t& file) {
    pix = types = prefix = file = 0;
    const bool dimension = png_dimension_record(status, width, height, depth, colour, interlace);
    if (!dimension && !png_encodable(status, width, height, depth, colour, interlace)) return kPngSkipped;
    if (analyse_status != kPngOk && analyse_status != kPngTooManyColours) return analyse_status;
    uint32_t d = depth, c = colour;
    if (dimension) {
        if (allowed == 0) allowed = 0x5Du;  // colour types 0, 2, 3, 4, 6
        const bool opaque = (summary & 1u) != 0, grey = (summary & 2u) != 0;
        const uint32_t sd = (summary >> 8) & 0xFFu;
        const bool palette = analyse_status == kPngOk && have_colour && count >= 1 && count <= 256 && trns_len <= count;
        const uint32_t pd = count <= 2 ? 1u : count <= 4 ? 2u : count <= 16 ? 4u : 8u;
        const uint32_t cand_colour[5] = {0, 2, 3, 4, 6}, cand_depth[5] = {sd, 8, pd, 8, 8};
        const bool cand_ok[5] = {opaque && grey && (sd == 1 || sd == 2 || sd == 4 || sd == 8), opaque, palette, grey, true};
        bool found = false;
        uint64_t least = 0;
        for (int k = 0; k < 5; k++) {
            if (!cand_ok[k] || !((allowed >> cand_colour[k]) & 1u)) continue;
            uint64_t cost = (uint64_t)height * png_row_bytes(width, png_pixel_bits(cand_depth[k], cand_colour[k]));
            if (cand_colour[k] == 3) cost += png_encode_prefix(3, count, trns_len) - kPngFilePrefix;
            if (!found || cost < least) found = true, least = cost, d = cand_depth[k], c = cand_colour[k];  // (ascending colour types)
        }
        if (!found) return kPngNotRepresentable;
    } else if (c == 3) {
        if (!have_colour || count < 1 || count > (1u << d)) return kPngBadPlte;
        if (trns_len > count) return kPngBadTrns;
    }
    uint64_t rb = 0, p = 0;
    if (png_encode_sizes(width, height, d, c, rb, p) != kPngOk) return kPngBadSizes;
    depth = d, colour = c;
    pix = p, types = height;
    prefix = png_encode_prefix(c, count, trns_len);
    file = prefix + png_ultrafast_bound((uint64_t)height * (rb + 1)) + kPngFileSuffix;
    return kPngOk;
}

// The encode plan of one RGBA16 image (include/fdeflate_hip_png16_encode.h): png_encode_plan with the summary and
// analyse_status of fdh_png_analyse16_mixed_batch.  An encodable record keeps its pair, and a dimension record whose
// summary has bit 2 (every sample is narrow: the picture of the high bytes holds it) is planned as that RGBA8 picture:
// both are png_encode_plan itself.  A dimension record with bit 2 clear has no palette and no depth below 16:
//   candidates   grey (0, 16): summary bits 0 and 1; RGB (2, 16): bit 0; grey-alpha (4, 16): bit 1; RGBA (6, 16) always
//   cost         height * row_bytes: the smallest wins, the lower colour type on equal cost.  The height is every
//                candidate's, so the row bytes are compared (the product may pass 2^64 at 64 bits per pixel)
// and analyse_status kPngTooManyColours is what the analysis says of every such picture, not an error.  The sizes, and
// kPngBadSizes, are png_encode_plan's for the pair that won.
FDH_PNG_FN uint32_t png_encode16_plan(uint32_t status, uint32_t width, uint32_t height, uint32_t& depth, uint32_t& colour, uint32_t interlace,
                                      bool have_colour, uint32_t count, uint32_t trns_len, uint32_t summary, uint32_t analyse_status,
                                      uint32_t allowed, uint64_t& pix, uint64_t& types, uint64_t& prefix, uint64_t& file) {
    if ((summary & 4u) != 0 || !png_dimension_record(status, width, height, depth, colour, interlace))
        return png_encode_plan(status, width, height, depth, colour, interlace, have_colour, count, trns_len, summary & 0xFF03u, analyse_status,
                               allowed, pix, types, prefix, file);
    pix = types = prefix = file = 0;
    if (analyse_status != kPngOk && analyse_status != kPngTooManyColours) return analyse_status;
    if (allowed == 0) allowed = 0x5Du;
    const bool opaque = (summary & 1u) != 0, grey = (summary & 2u) != 0;
    const uint32_t cand_colour[4] = {0, 2, 4, 6};
    const bool cand_ok[4] = {opaque && grey, opaque, grey, true};
    uint32_t c = 0;
    uint64_t least = 0;
    for (int k = 0; k < 4; k++) {
        if (!cand_ok[k] || !((allowed >> cand_colour[k]) & 1u)) continue;
        const uint64_t rb = png_row_bytes(width, png_pixel_bits(16, cand_colour[k]));
        if (least == 0 || rb < least) least = rb, c = cand_colour[k];  // (ascending colour types; a row has bytes)
    }
    if (least == 0) return kPngNotRepresentable;
    uint32_t d = 16;
    const uint32_t st = png_encode_plan(status, width, height, d, c, interlace, false, 0, 0, 0, kPngOk, 0, pix, types, prefix, file);
    if (st == kPngOk) depth = d, colour = c;
    return st;
}

// ---- values that follow from the specification ----
static_assert(png_encode_prefix(0, 7, 7) == 41 && png_encode_prefix(3, 1, 0) == 56 && png_encode_prefix(3, 256, 256) == 41 + 12 + 768 + 12 + 256,
              "the exact-palette prefix");
static_assert(png_ultrafast_bound(0) == 60 && png_ultrafast_bound(65536) == 98364, "fdh_ultrafast_bound");
#define FDH_PNG_PAIR_OK(D, C) && png_pair_ok(D, C)
static_assert(true FDH_PNG_FOR_EACH_PAIR(FDH_PNG_PAIR_OK), "the fifteen pairs");
#undef FDH_PNG_PAIR_OK
static_assert(!png_pair_ok(16, 3) && !png_pair_ok(8, 1) && !png_pair_ok(4, 2) && !png_pair_ok(0, 0) && !png_pair_ok(8, 7), "and no others");
static_assert(png_bpp(1) == 1 && png_bpp(24) == 3 && png_bpp(64) == 8, "filter pixel sizes");
static_assert(png_row_bytes(1, 1) == 1 && png_row_bytes(9, 1) == 2 && png_row_bytes(341, 24) == 1023 &&
              png_row_bytes(0x7FFFFFFFull, 64) == 0x3FFFFFFF8ull, "row bytes, in 64 bits");
static_assert(png_adam7_size(8, 8, 8, 1) == 2 + 2 + 3 + 6 + 10 + 20 + 36, "8 x 8 grey-8, interlaced: 79 bytes");
static_assert(png_adam7_size(8, 8, 8, 0) == 8 * 9 && png_adam7_size(1, 9, 8, 1) == 18 && png_adam7_size(1, 1, 1, 1) == 2, "one pass; empty passes");

}  // namespace fdh
