// png_choose_body.h -- filter selection: which of the five types each row is filtered with, as a device function of one
// image (png_choose_image): png_choose.hip (one row size per call) and png_encode_mixed.hip (the row size of each image
// from its fdh_png_info record) run the same code behind their own checks.
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
#pragma once
#include "device_common.h"
#include "png_common.h"
#include "png_rows.h"

namespace fdh {

constexpr uint32_t kChooseBand = 64;  // rows per band: one band = one image of the bench shape

struct PngChooseArgs {
    const uint8_t* pix;
    const uint64_t* pix_off;    // n + 1
    uint8_t* types;             // one byte per row
    const uint64_t* types_off;  // n + 1
    uint32_t* status;           // kPngOk or kPngBadSizes
    uint64_t n;
    uint32_t row_bytes;
    uint32_t group;             // G: lanes per row
    uint32_t pieces;            // J: 16 G-byte pieces per row
};

constexpr uint32_t kHi = 0x80808080u;

// x - p byte by byte, modulo 256
__device__ __forceinline__ uint32_t png_sub4(uint32_t x, uint32_t p) { return ((x | kHi) - (p & ~kHi)) ^ ((x ^ ~p) & kHi); }
// floor((a + b) / 2) byte by byte (the sum is not taken modulo 256)
__device__ __forceinline__ uint32_t png_avg4(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
// acc + the costs of the four filtered bytes of f: a byte v >= 128 costs 256 - v = (v ^ 0xFF) + 1
__device__ __forceinline__ uint32_t png_cost4(uint32_t f, uint32_t acc) {
    const uint32_t s = f & kHi;
    const uint32_t fold = f ^ (s | (s - (s >> 7)));
    return __builtin_amdgcn_sad_u8(fold, 0u, acc) + (uint32_t)__builtin_popcount(s);
}
// the 16 bytes that lie BPP in front of the chunk v: (tz, tw) are the last 8 bytes in front of it
template <int BPP>
__device__ __forceinline__ uint4 png_left16(const uint4& v, uint32_t tz, uint32_t tw) {
    const uint32_t s[6] = {tz, tw, v.x, v.y, v.z, v.w};
    constexpr int wi = (8 - BPP) / 4, sh = (8 - BPP) % 4;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = sh ? (uint32_t)(((((uint64_t)s[wi + k + 1]) << 32) | s[wi + k]) >> (8 * sh)) : s[wi + k];
    return make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ uint4 png_and16(const uint4& v, const uint4& m) { return make_uint4(v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w); }
// all ones in the first `valid` (0..16) bytes
__device__ __forceinline__ uint4 png_valid_mask(uint32_t valid) {
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = valid >= 4u * k + 4 ? 0xFFFFFFFFu : (valid <= 4u * k ? 0u : (1u << (8 * (valid - 4u * k))) - 1u);
    return make_uint4(m[0], m[1], m[2], m[3]);
}
// the costs of one chunk under the five types, added to sum[]: x the pixels, b the row above, a / c the bytes BPP to their left
__device__ __forceinline__ void png_costs16(const uint4& x, const uint4& a, const uint4& b, const uint4& c, uint32_t (&sum)[5]) {
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        sum[0] = png_cost4(xs[k], sum[0]);
        sum[1] = png_cost4(png_sub4(xs[k], as[k]), sum[1]);
        sum[2] = png_cost4(png_sub4(xs[k], bs[k]), sum[2]);
        sum[3] = png_cost4(png_sub4(xs[k], png_avg4(as[k], bs[k])), sum[3]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t d = __builtin_amdgcn_sad_u8(png_byte(x, k), png_paeth(png_byte(a, k), png_byte(b, k), png_byte(c, k)), 0u);
        sum[4] += min(d, 256u - d);
    }
}
template <int CTRL>
__device__ __forceinline__ uint32_t png_dpp_add(uint32_t v) { return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
// v summed over the aligned group of `group` lanes (a power of two) this lane is in; every lane gets the sum
__device__ __forceinline__ uint32_t png_group_sum16(uint32_t v, uint32_t group) {  // the steps inside 16 lanes
    if (group >= 2) v = png_dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    if (group >= 4) v = png_dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    if (group >= 8) v = png_dpp_add<0x141>(v);  // row_half_mirror: the other quad of eight lanes
    if (group >= 16) v = png_dpp_add<0x140>(v); // row_mirror: the other eight of sixteen
    return v;
}
__device__ __forceinline__ uint32_t png_group_sum64(uint32_t v, uint32_t group) {  // ... and across them
    if (group >= 32) v += (uint32_t)__shfl_xor((int)v, 16, 64);
    if (group >= 64) v += (uint32_t)__shfl_xor((int)v, 32, 64);
    return v;
}
__device__ __forceinline__ uint4 png_shfl16(const uint4& v, int src) {
    return make_uint4((uint32_t)__shfl((int)v.x, src, 64), (uint32_t)__shfl((int)v.y, src, 64), (uint32_t)__shfl((int)v.z, src, 64), (uint32_t)__shfl((int)v.w, src, 64));
}

// Image i of the call at a.row_bytes, a.group and a.pieces: the slots' check, the status, the bands blockIdx.y,
// blockIdx.y + gridDim.y, ..  LOOP: rows of more than one piece per lane (J > 1).
template <int BPP, bool LOOP>
__device__ __forceinline__ void png_choose_image(const PngChooseArgs& a, uint64_t i, uint32_t lane) {
    const uint64_t s0 = a.pix_off[i], s1 = a.pix_off[i + 1], t0 = a.types_off[i], t1 = a.types_off[i + 1];
    const uint64_t rb = a.row_bytes;
    const uint64_t rows = (s1 - s0) / rb;
    const bool fits = rows * rb == s1 - s0 && t1 - t0 == rows;
    if (blockIdx.y == 0 && lane == 0) a.status[i] = fits ? kPngOk : kPngBadSizes;
    if (!fits) return;
    const uint32_t G = a.group, R = kWave / G;  // lanes per row, rows per step
    const uint32_t g = lane / G, q = lane & (G - 1);
    const uint8_t* const img = a.pix + s0;
    const uint8_t* const end = a.pix + s1;
    // 16 bytes of row r at x, zero behind the row's end; never reads behind the image
    auto load = [&](uint64_t r, uint64_t x) -> uint4 {
        if (x >= rb) return make_uint4(0, 0, 0, 0);
        const uint8_t* const p = img + r * rb + x;
        const uint32_t valid = (uint32_t)min((uint64_t)16, rb - x);
        const uint4 v = p + 16 <= end ? png_load16(p) : png_load_part(p, valid);
        return png_and16(v, png_valid_mask(valid));
    };
    uint8_t* const types = a.types + t0;
    const uint64_t bands = (rows + kChooseBand - 1) / kChooseBand;
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kChooseBand;
        const uint64_t r1 = min(rows, r0 + kChooseBand);
        // what the last group "held one step earlier" at the band's first step: the row above the band
        uint4 held = make_uint4(0, 0, 0, 0);
        if (!LOOP && g == R - 1 && r0 > 0) held = load(r0 - 1, (uint64_t)q * 16);
        for (uint64_t rs = r0; rs < r1; rs += R) {
            const uint64_t r = rs + g;
            const bool have = r < r1;
            uint32_t sum[5] = {0, 0, 0, 0, 0};
            if (!LOOP) {
                const uint64_t x = (uint64_t)q * 16;
                const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                uint4 cur = make_uint4(0, 0, 0, 0);
                if (have) cur = load(r, x);
                // the row above: the group before this one holds it (group 0: the last group's chunk of the step before)
                uint4 up = cur;
                if (G < kWave) up = png_shfl16(g == R - 1 ? held : cur, (int)((lane - G) & (kWave - 1)));
                else up = held;
                held = cur;
                if (r == 0) up = make_uint4(0, 0, 0, 0);
                const bool first = q == 0;  // nothing to the left of the row's first pixel
                uint32_t cz = png_from_lane_below(cur.z), cw = png_from_lane_below(cur.w);
                uint32_t uz = png_from_lane_below(up.z), uw = png_from_lane_below(up.w);
                if (first) cz = cw = uz = uw = 0;
                const uint4 left = png_and16(png_left16<BPP>(cur, cz, cw), mask);
                const uint4 upleft = png_and16(png_left16<BPP>(up, uz, uw), mask);
                png_costs16(cur, left, up, upleft, sum);
                // two sums to a word inside sixteen lanes (at most 32768 each)
                uint32_t w0 = png_group_sum16(sum[0] | (sum[1] << 16), G), w1 = png_group_sum16(sum[2] | (sum[3] << 16), G);
                sum[4] = png_group_sum16(sum[4], G);
                sum[0] = w0 & 0xFFFF, sum[1] = w0 >> 16, sum[2] = w1 & 0xFFFF, sum[3] = w1 >> 16;
            } else {
                uint32_t cz = 0, cw = 0, uz = 0, uw = 0;  // lane q == 0: the bytes in front of its piece (the group's last lane had them)
                const int last = (int)(lane | (G - 1));
                for (uint32_t j = 0; j < a.pieces; j++) {
                    const uint64_t x = ((uint64_t)j * G + q) * 16;
                    const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                    uint4 cur = make_uint4(0, 0, 0, 0), up = cur;
                    if (have) cur = load(r, x);
                    if (have && r > 0) up = load(r - 1, x);
                    uint32_t lz = png_from_lane_below(cur.z), lw = png_from_lane_below(cur.w);
                    uint32_t vz = png_from_lane_below(up.z), vw = png_from_lane_below(up.w);
                    if (q == 0) lz = cz, lw = cw, vz = uz, vw = uw;
                    cz = (uint32_t)__shfl((int)cur.z, last, 64), cw = (uint32_t)__shfl((int)cur.w, last, 64);
                    uz = (uint32_t)__shfl((int)up.z, last, 64), uw = (uint32_t)__shfl((int)up.w, last, 64);
                    const uint4 left = png_and16(png_left16<BPP>(cur, lz, lw), mask);
                    const uint4 upleft = png_and16(png_left16<BPP>(up, vz, vw), mask);
                    png_costs16(cur, left, up, upleft, sum);
                }
#pragma unroll
                for (int t = 0; t < 5; t++) sum[t] = png_group_sum16(sum[t], G);
            }
            uint32_t best = 0, least = 0;
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const uint32_t s = png_group_sum64(sum[t], G);
                if (t == 0 || s < least) best = t, least = s;  // strictly smaller: the lowest type number wins a tie
            }
            if (have && q == 0) types[r] = (uint8_t)best;
        }
    }
}

}  // namespace fdh
