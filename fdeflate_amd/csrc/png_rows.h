// png_rows.h -- what the PNG row kernels share (png_filter.hip, png_choose.hip, png_adam7.hip): the Paeth predictor,
// the branch-free predictor of a row's filter type, sixteen bytes of a row in registers, the 16-byte loads and stores
// at any alignment, whole and partial, and the shift of a value to the lane above.
#pragma once
#include "device_common.h"

namespace fdh {

// Paeth predictor (PNG specification 9.4): p = a + b - c; the neighbour closest to p, ties in the
// order a, b, c.  |p - a| = |b - c|, |p - b| = |a - c|, |p - c| = |a + b - 2c|: three
// sum-of-absolute-differences instructions on byte values.
__device__ __forceinline__ uint32_t png_paeth(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pa = __builtin_amdgcn_sad_u8(b, c, 0u), pb = __builtin_amdgcn_sad_u8(a, c, 0u);
    const uint32_t pc = __builtin_amdgcn_sad_u16(a + b, c << 1, 0u);
    const uint32_t bc = pb <= pc ? b : c;
    return (pa <= pb && pa <= pc) ? a : bc;
}

// The predictor of a row's type without branching on the type (lanes hold rows of different types):
// None / Sub / Up / Average are (a * wa + b * wb) >> sh with per-row weights, Paeth is selected over it.
struct PngMasks {
    uint32_t wa, wb, sh;
    uint32_t paeth;  // all ones for a Paeth row: the select is a bit-field insert, not a branch per byte
    __device__ explicit PngMasks(uint32_t t) : wa(t == 1 || t == 3 ? 1u : 0u), wb(t == 2 || t == 3 ? 1u : 0u), sh(t == 3 ? 1u : 0u), paeth(t == 4 ? 0xFFFFFFFFu : 0u) {}
    __device__ __forceinline__ uint32_t pred(uint32_t a, uint32_t b, uint32_t c) const {
        const uint32_t lin = (__umul24(a, wa) + __umul24(b, wb)) >> sh;
        return (png_paeth(a, b, c) & paeth) | (lin & ~paeth);
    }
};

__device__ __forceinline__ uint4 png_load16(const uint8_t* p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);  // rows start at any alignment: unaligned 16-B access (hardware-supported)
    return v;
}
__device__ __forceinline__ void png_store16(uint8_t* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }
// lane j gets lane j - 1's value (lane 0: 0): how a row hands its chunk to the row below it
__device__ __forceinline__ uint32_t png_from_lane_below(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t png_byte(const uint4& v, int k) {
    const uint32_t w = k < 4 ? v.x : (k < 8 ? v.y : (k < 12 ? v.z : v.w));
    return (w >> (8 * (k & 3))) & 0xFF;
}

// Sixteen bytes of one row.  UNFILTER: out = filt + pred(reconstructed left, up, up-left); else
// filt = raw - pred(raw left, up, up-left).  la / ua carry the last BPP bytes of this row
// (reconstructed / raw) and of the row above into the next chunk.
template <int BPP, bool UNFILTER>
__device__ __forceinline__ uint4 png_chunk(const uint4& f, const uint4& u, uint32_t (&la)[8], uint32_t (&ua)[8], const PngMasks& m) {
    uint32_t o[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t b = png_byte(u, k);
        // left / up-left neighbour: BPP bytes back, in this chunk or in the carried tail
        const uint32_t a = k >= BPP ? (UNFILTER ? o[k - BPP] : png_byte(f, k - BPP)) : la[8 - BPP + k];
        const uint32_t c = k >= BPP ? png_byte(u, k - BPP) : ua[8 - BPP + k];
        const uint32_t fv = png_byte(f, k);
        const uint32_t pr = m.pred(a, b, c);
        o[k] = (UNFILTER ? fv + pr : fv - pr) & 0xFF;
    }
#pragma unroll
    for (int k = 0; k < BPP; k++) {  // carry the tails (BPP <= 8 <= 16)
        la[8 - BPP + k] = UNFILTER ? o[16 - BPP + k] : png_byte(f, 16 - BPP + k);
        ua[8 - BPP + k] = png_byte(u, 16 - BPP + k);
    }
    uint4 r;
    r.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    r.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
    r.z = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
    r.w = o[12] | (o[13] << 8) | (o[14] << 16) | (o[15] << 24);
    return r;
}

// `valid` bytes (1..16) at p as a 16-byte chunk, never reading behind them.
// The first `valid` (< 16: else all) of sixteen bytes, the others untouched / zero: an 8-, a 4-, a 2- and a 1-byte access as
// the bits of `valid` say, not a loop over the bytes -- ONE lane of the pipeline has a row's last, partial piece in hand at
// every memory step, and a wavefront issues what one of its lanes executes (the byte loop: ~150 instructions per piece).
__device__ __forceinline__ uint4 png_load_part(const uint8_t* p, uint32_t valid) {
    if (valid >= 16) return png_load16(p);
    uint64_t lo = 0, hi = 0, part = 0;
    uint32_t at = 0, sh = 0;  // bytes read so far of this half; bits filled of `part`
    if (valid & 8) {
        __builtin_memcpy(&lo, p, 8);
        at = 8;
    }
    if (valid & 4) {
        uint32_t w;
        __builtin_memcpy(&w, p + at, 4);
        part = w;
        at += 4;
        sh = 32;
    }
    if (valid & 2) {
        uint16_t h;
        __builtin_memcpy(&h, p + at, 2);
        part |= (uint64_t)h << sh;
        at += 2;
        sh += 16;
    }
    if (valid & 1) part |= (uint64_t)p[at] << sh;
    if (valid & 8) hi = part;
    else lo = part;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__device__ __forceinline__ void png_store_part(uint8_t* p, const uint4& v, uint32_t valid) {
    if (valid >= 16) {
        png_store16(p, v);
        return;
    }
    const uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
    uint64_t rest = lo;
    uint32_t at = 0;
    if (valid & 8) {
        __builtin_memcpy(p, &lo, 8);
        rest = hi;
        at = 8;
    }
    if (valid & 4) {
        const uint32_t w = (uint32_t)rest;
        __builtin_memcpy(p + at, &w, 4);
        rest >>= 32;
        at += 4;
    }
    if (valid & 2) {
        const uint16_t h = (uint16_t)rest;
        __builtin_memcpy(p + at, &h, 2);
        rest >>= 16;
        at += 2;
    }
    if (valid & 1) p[at] = (uint8_t)rest;
}

}  // namespace fdh
