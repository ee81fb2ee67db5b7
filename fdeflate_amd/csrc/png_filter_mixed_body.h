// png_filter_mixed_body.h -- filter selection and filtering of one image in one pass, as a device function
// (png_filter_mixed_image): what png_choose_body.h computes to choose a row's type is all it takes to WRITE the row
// filtered with that type, so the step between packed scanlines and an encoder that wants the filtered rows in memory
// (the level encoders, include/fdeflate_hip_png_levels.h) reads a pixel byte once.
//
// The walk is png_choose_image's, unchanged: lanes along the row, 16 bytes each, a group of G lanes per row, 64 / G
// rows per step down a band of kChooseBand rows, the row above through a cross-lane read, the bytes to the left from
// the lane below.  What differs is what is kept: the chunk filtered under each of the five types stays in registers
// (twenty words) while its costs are summed -- Paeth's filtered bytes are packed into words and costed with png_cost4
// like the others, the same number as min(d, 256 - d) of the byte distance d -- and when the group's sums have met, the
// chunk of the winning type is selected and stored.  GIVEN: the caller's types; the same loads and neighbours, no costs,
// only the row's own type computed.  LOOP (rows of more than one piece per lane): the costs are summed along the row
// as there, and the row is walked a second time once the type is known; the second walk's loads hit the lines the first
// brought in.
//
// Stores.  Output rows lie row_bytes + 1 apart -- a type byte in front of every row -- so whatever the alignment of the
// slot, the 16-byte chunks of consecutive rows sit at every offset modulo 16 in turn and no choice of chunk origin
// aligns more than one row in sixteen.  The chunks are stored where they fall, as unaligned 16-byte stores, one
// instruction each (PngChunkAnywhere; the hardware splits one that straddles a 64-byte boundary); a wavefront's stores of one step still cover one contiguous
// run of 64 / G rows, type bytes included, so every line it touches is written in full by that step or the next.  A
// row's last, partial chunk leaves as an 8-, a 4-, a 2- and a 1-byte store (png_store_part); no store reads back or
// rounds up, so nothing outside the image's own slot is written.
#pragma once
#include "device_common.h"
#include "png_choose_body.h"
#include "png_common.h"
#include "png_rows.h"

namespace fdh {

// One image's slots, checked by the caller: pix rows * row_bytes bytes, filt rows * (row_bytes + 1), types rows
// (null: chosen mode without a record of the choice).
struct PngFilterMixedImage {
    const uint8_t* pix;
    uint8_t* types;
    uint8_t* filt;
    uint32_t* status;  // this image's word: kPngBadFilterType is stored here (GIVEN), nothing else
    uint64_t rows;
    uint32_t row_bytes;
    uint32_t group;   // G: lanes per row
    uint32_t pieces;  // J: 16 G-byte pieces per row
};

// sixteen bytes at any address, as one vector: a whole chunk leaves in one store instruction (written as a 16-byte
// memcpy beside png_store_part's pieces, the compiler merges the two and stores two halves)
struct __attribute__((packed, aligned(1))) PngChunkAnywhere {
    uint32_t v __attribute__((ext_vector_type(4)));
};

// the chunk x filtered under the five types: a / c the bytes BPP to the left of x and of b, the row above
__device__ __forceinline__ void png_filter16_all(const uint4& x, const uint4& a, const uint4& b, const uint4& c, uint4 (&f)[5]) {
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        o[0][k] = png_sub4(xs[k], as[k]);
        o[1][k] = png_sub4(xs[k], bs[k]);
        o[2][k] = png_sub4(xs[k], png_avg4(as[k], bs[k]));
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int at = 4 * k + j;
            w |= ((png_byte(x, at) - png_paeth(png_byte(a, at), png_byte(b, at), png_byte(c, at))) & 0xFFu) << (8 * j);
        }
        o[3][k] = w;
    }
    f[0] = x;
#pragma unroll
    for (int t = 0; t < 4; t++) f[t + 1] = make_uint4(o[t][0], o[t][1], o[t][2], o[t][3]);
}
// ... and under type t alone (0 .. 4; lanes of one row agree on t, rows of one wavefront need not)
__device__ __forceinline__ uint4 png_filter16(uint32_t t, const uint4& x, const uint4& a, const uint4& b, const uint4& c) {
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4];
    if (t == 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int at = 4 * k + j;
                w |= ((png_byte(x, at) - png_paeth(png_byte(a, at), png_byte(b, at), png_byte(c, at))) & 0xFFu) << (8 * j);
            }
            o[k] = w;
        }
    } else {
        const uint32_t ma = t == 1 || t == 3 ? 0xFFFFFFFFu : 0u, mb = t == 2 || t == 3 ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t pa = as[k] & ma, pb = bs[k] & mb;
            o[k] = png_sub4(xs[k], t == 3 ? png_avg4(pa, pb) : pa | pb);
        }
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ uint32_t png_cost16(const uint4& f, uint32_t acc) {
    return png_cost4(f.w, png_cost4(f.z, png_cost4(f.y, png_cost4(f.x, acc))));
}

// The bands blockIdx.y, blockIdx.y + gridDim.y, .. of one image.  GIVEN: m.types is read (a value above 4: the image's
// status becomes kPngBadFilterType, the row is written with its type byte and unfiltered); else the type of every row is
// chosen by png_choose_image's rule, written to m.types where that is not null, and used.
template <int BPP, bool LOOP, bool GIVEN>
__device__ __forceinline__ void png_filter_mixed_image(const PngFilterMixedImage& m, uint32_t lane) {
    const uint64_t rb = m.row_bytes, rows = m.rows;
    const uint32_t G = m.group, R = kWave / G;  // lanes per row, rows per step
    const uint32_t g = lane / G, q = lane & (G - 1);
    const uint8_t* const img = m.pix;
    const uint8_t* const end = m.pix + rows * rb;
    // 16 bytes of row r at x, zero behind the row's end; never reads behind the image
    auto load = [&](uint64_t r, uint64_t x) -> uint4 {
        if (x >= rb) return make_uint4(0, 0, 0, 0);
        const uint8_t* const p = img + r * rb + x;
        const uint32_t valid = (uint32_t)min((uint64_t)16, rb - x);
        const uint4 v = p + 16 <= end ? png_load16(p) : png_load_part(p, valid);
        return png_and16(v, png_valid_mask(valid));
    };
    // the filtered chunk of row r at x: behind the row's type byte, the bytes of the row only
    auto store = [&](uint64_t r, uint64_t x, const uint4& f) {
        if (x >= rb) return;
        uint8_t* const p = m.filt + r * (rb + 1) + 1 + x;
        if (x + 16 <= rb) *reinterpret_cast<PngChunkAnywhere*>(p) = PngChunkAnywhere{{f.x, f.y, f.z, f.w}};  // ONE 16-byte store
        else png_store_part(p, f, (uint32_t)(rb - x));
    };
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
            uint32_t given = 0;
            if (GIVEN && have) {
                given = m.types[r];
                if (given > 4 && q == 0) *m.status = kPngBadFilterType;
            }
            uint32_t sum[5] = {0, 0, 0, 0, 0};
            uint4 cur = make_uint4(0, 0, 0, 0), up = cur, left = cur, upleft = cur;  // (!LOOP: the row's one piece)
            uint4 f[5];
            if (!LOOP) {
                const uint64_t x = (uint64_t)q * 16;
                const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                if (have) cur = load(r, x);
                // the row above: the group before this one holds it (group 0: the last group's chunk of the step before)
                if (G < kWave) up = png_shfl16(g == R - 1 ? held : cur, (int)((lane - G) & (kWave - 1)));
                else up = held;
                held = cur;
                if (r == 0) up = make_uint4(0, 0, 0, 0);
                uint32_t cz = png_from_lane_below(cur.z), cw = png_from_lane_below(cur.w);
                uint32_t uz = png_from_lane_below(up.z), uw = png_from_lane_below(up.w);
                if (q == 0) cz = cw = uz = uw = 0;  // nothing to the left of the row's first pixel
                left = png_and16(png_left16<BPP>(cur, cz, cw), mask);
                upleft = png_and16(png_left16<BPP>(up, uz, uw), mask);
                if (!GIVEN) {
                    png_filter16_all(cur, left, up, upleft, f);
#pragma unroll
                    for (int t = 0; t < 5; t++) sum[t] = png_cost16(f[t], 0u);
                    // two sums to a word inside sixteen lanes (at most 32768 each)
                    uint32_t w0 = png_group_sum16(sum[0] | (sum[1] << 16), G), w1 = png_group_sum16(sum[2] | (sum[3] << 16), G);
                    sum[4] = png_group_sum16(sum[4], G);
                    sum[0] = w0 & 0xFFFF, sum[1] = w0 >> 16, sum[2] = w1 & 0xFFFF, sum[3] = w1 >> 16;
                }
            } else if (!GIVEN) {
                uint32_t cz = 0, cw = 0, uz = 0, uw = 0;  // lane q == 0: the bytes in front of its piece (the group's last lane had them)
                const int last = (int)(lane | (G - 1));
                for (uint32_t j = 0; j < m.pieces; j++) {
                    const uint64_t x = ((uint64_t)j * G + q) * 16;
                    const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                    cur = up = make_uint4(0, 0, 0, 0);
                    if (have) cur = load(r, x);
                    if (have && r > 0) up = load(r - 1, x);
                    uint32_t lz = png_from_lane_below(cur.z), lw = png_from_lane_below(cur.w);
                    uint32_t vz = png_from_lane_below(up.z), vw = png_from_lane_below(up.w);
                    if (q == 0) lz = cz, lw = cw, vz = uz, vw = uw;
                    cz = (uint32_t)__shfl((int)cur.z, last, 64), cw = (uint32_t)__shfl((int)cur.w, last, 64);
                    uz = (uint32_t)__shfl((int)up.z, last, 64), uw = (uint32_t)__shfl((int)up.w, last, 64);
                    left = png_and16(png_left16<BPP>(cur, lz, lw), mask);
                    upleft = png_and16(png_left16<BPP>(up, vz, vw), mask);
                    png_costs16(cur, left, up, upleft, sum);
                }
#pragma unroll
                for (int t = 0; t < 5; t++) sum[t] = png_group_sum16(sum[t], G);
            }
            uint32_t best = given;
            if (!GIVEN) {
                uint32_t least = 0;
#pragma unroll
                for (int t = 0; t < 5; t++) {
                    const uint32_t s = png_group_sum64(sum[t], G);
                    if (t == 0 || s < least) best = t, least = s;  // strictly smaller: the lowest type number wins a tie
                }
            }
            if (have && q == 0) {
                if (!GIVEN && m.types) m.types[r] = (uint8_t)best;
                m.filt[r * (rb + 1)] = (uint8_t)best;
            }
            const uint32_t with = best > 4 ? 0u : best;  // (a type that does not exist: the row as it is)
            if (!LOOP) {
                uint4 out;
                if (GIVEN) {
                    out = png_filter16(with, cur, left, up, upleft);
                } else {
                    out = f[0];
#pragma unroll
                    for (int t = 1; t < 5; t++)
                        if (best == (uint32_t)t) out = f[t];
                }
                if (have) store(r, (uint64_t)q * 16, out);
            } else {
                // the second walk along the row, with the type in hand
                uint32_t cz = 0, cw = 0, uz = 0, uw = 0;
                const int last = (int)(lane | (G - 1));
                for (uint32_t j = 0; j < m.pieces; j++) {
                    const uint64_t x = ((uint64_t)j * G + q) * 16;
                    const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                    cur = up = make_uint4(0, 0, 0, 0);
                    if (have) cur = load(r, x);
                    if (have && r > 0) up = load(r - 1, x);
                    uint32_t lz = png_from_lane_below(cur.z), lw = png_from_lane_below(cur.w);
                    uint32_t vz = png_from_lane_below(up.z), vw = png_from_lane_below(up.w);
                    if (q == 0) lz = cz, lw = cw, vz = uz, vw = uw;
                    cz = (uint32_t)__shfl((int)cur.z, last, 64), cw = (uint32_t)__shfl((int)cur.w, last, 64);
                    uz = (uint32_t)__shfl((int)up.z, last, 64), uw = (uint32_t)__shfl((int)up.w, last, 64);
                    left = png_and16(png_left16<BPP>(cur, lz, lw), mask);
                    upleft = png_and16(png_left16<BPP>(up, vz, vw), mask);
                    if (have) store(r, x, png_filter16(with, cur, left, up, upleft));
                }
            }
        }
    }
}

}  // namespace fdh
