// png_expand_body.h -- the expansion of png_expand.hip and png_expand16.hip as a device function of one image, so that
// the calls of one geometry and png_mixed.hip (the geometry of each image in its fdh_png_info record) run the same code,
// and so that RGBA8 (OPX = 4 bytes per output pixel) and RGBA16 (OPX = 8) share the band loop.  png_expand.hip and
// png_expand16.hip describe it.
#pragma once
#include "device_common.h"
#include "launch.h"
#include "png_common.h"

namespace fdh {

constexpr uint32_t kExpandBand = 64;  // rows per band: one band = one image of the bench shape

// RGBA16: pixels per lane and step.  2: one 16-byte store, the wavefront's 1 KiB contiguous; 4: two stores, each 32 bytes
// apart from the next lane's.  2 is faster on every pair that was measured (DESIGN.md 3.3 has the comparison);
// -DFDH_EXPAND16_GROUP=4 builds the other shape.
#ifndef FDH_EXPAND16_GROUP
#define FDH_EXPAND16_GROUP 2
#endif
constexpr int kExpand16Group = FDH_EXPAND16_GROUP;
static_assert(kExpand16Group == 2 || kExpand16Group == 4, "whole 16-byte stores");

struct PngExpandArgs {
    const uint8_t* pix;
    const uint64_t* pix_off;   // n + 1
    uint8_t* rgba;             // RGBA8 or RGBA16, as the kernel's OPX says
    const uint64_t* rgba_off;  // n + 1
    const uint32_t* pal;       // nullable unless the colour type is 3: 256 words per image
    const uint32_t* colour;    // nullable: 4 words per image (count, key present, key R or grey | G << 16, key B)
    const uint32_t* upstream;  // nullable
    uint32_t* status;          // zeroed by the launcher
    uint64_t n;
    uint64_t row_bytes;
    uint32_t width;
};

struct ExpandKey {
    uint32_t count;    // palette entries (colour type 3)
    bool present;      // colour types 0 and 2
    uint32_t r, g, b;  // masked to the depth; r is the grey key
};

// N bytes as the compiler should load them: whole words (one load of 4, 8, 12, 16 bytes, two of 16 for 32; 1 and 2 bytes
// for the narrowest pixels), the bytes taken out of the registers afterwards
template <int N>
struct ExpandBytes {
    uint32_t w[(N + 3) / 4];
    __device__ __forceinline__ void load(const uint8_t* p) {
        if (N < 4) w[0] = 0;
        __builtin_memcpy(w, p, N);  // any alignment: the hardware takes unaligned vector accesses
    }
    __device__ __forceinline__ uint32_t byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
    // big-endian 16-bit samples to the device's order, two per instruction; half(k) is sample k afterwards
    __device__ __forceinline__ void swap16() {
#pragma unroll
        for (int k = 0; k < (N + 3) / 4; k++) w[k] = __builtin_amdgcn_perm(w[k], w[k], 0x02030001u);
    }
    __device__ __forceinline__ uint32_t half(int k) const { return (k & 1) ? w[k >> 1] >> 16 : w[k >> 1] & 0xFFFFu; }
};

template <int DEPTH, int COLOUR, int OPX = 4>
struct Expand {
    static_assert(OPX == 4 || OPX == 8, "RGBA8 or RGBA16");
    static constexpr int CH = (int)png_channels(COLOUR);
    static constexpr int BITS = (int)png_pixel_bits(DEPTH, COLOUR);  // per pixel
    static constexpr int G = OPX == 8 ? kExpand16Group : 4;          // pixels per lane and step ("quad": G of them)
    static constexpr int QUAD = BITS * G / 8 ? BITS * G / 8 : 1;     // bytes that hold G pixels (or a part of one byte)
    static constexpr uint32_t MAXV = (1u << DEPTH) - 1;
    static constexpr bool SWAPPED = OPX == 8 && DEPTH == 16;         // the wide path swaps whole words (ExpandBytes::swap16)

    static __device__ __forceinline__ uint32_t to8(uint32_t s) {
        if (DEPTH == 16) return s >> 8;
        if (DEPTH == 8) return s;
        return s * (255u / MAXV);
    }
    // PNG specification 13.12: the exact factors 65535 / (2^DEPTH - 1) = 1, 257, 4369, 21845, 65535
    static __device__ __forceinline__ uint32_t to16(uint32_t s) {
        if (DEPTH == 16) return s;
        return s * (65535u / MAXV);
    }

    // one pixel from its CH raw samples
    static __device__ __forceinline__ uint32_t pixel(const uint32_t (&s)[CH], const ExpandKey& k, const uint32_t* pal, bool& bad) {
        if (COLOUR == 3) {
            bad = bad || s[0] >= k.count;
            return pal[s[0]];
        }
        if (COLOUR == 0) {
            const uint32_t g = to8(s[0]);
            return g * 0x010101u | (k.present && s[0] == k.r ? 0u : 0xFF000000u);
        }
        if (COLOUR == 4) return to8(s[0]) * 0x010101u | to8(s[CH - 1]) << 24;
        const uint32_t rgb = to8(s[0]) | to8(s[CH > 1 ? 1 : 0]) << 8 | to8(s[CH > 2 ? 2 : 0]) << 16;
        if (COLOUR == 2) return rgb | (k.present && s[0] == k.r && s[CH > 1 ? 1 : 0] == k.g && s[CH > 2 ? 2 : 0] == k.b ? 0u : 0xFF000000u);
        return rgb | to8(s[CH - 1]) << 24;
    }

    // the same pixel as RGBA16: x = R | G << 16, y = B | A << 16.  A palette word's four bytes are scaled by 257 two at a
    // time (255 * 257 = 65535: nothing carries); the key is compared on the raw samples, all 16 bits at depth 16.
    static __device__ __forceinline__ uint2 pixel16(const uint32_t (&s)[CH], const ExpandKey& k, const uint32_t* pal, bool& bad) {
        if (COLOUR == 3) {
            bad = bad || s[0] >= k.count;
            const uint32_t w = pal[s[0]];
            return make_uint2(((w & 0xFFu) | (w & 0xFF00u) << 8) * 257u, (((w >> 16) & 0xFFu) | (w >> 24) << 16) * 257u);
        }
        if (COLOUR == 0) {
            const uint32_t g = to16(s[0]);
            return make_uint2(g * 0x00010001u, g | (k.present && s[0] == k.r ? 0u : 0xFFFF0000u));
        }
        if (COLOUR == 4) {
            const uint32_t g = to16(s[0]);
            return make_uint2(g * 0x00010001u, g | to16(s[CH - 1]) << 16);
        }
        const uint32_t rg = to16(s[0]) | to16(s[CH > 1 ? 1 : 0]) << 16, b = to16(s[CH > 2 ? 2 : 0]);
        if (COLOUR == 2) return make_uint2(rg, b | (k.present && s[0] == k.r && s[CH > 1 ? 1 : 0] == k.g && s[CH > 2 ? 2 : 0] == k.b ? 0u : 0xFFFF0000u));
        return make_uint2(rg, b | to16(s[CH - 1]) << 16);
    }

    // sample c of pixel j of the bytes q.  Below 8 bits pixel 0 starts at bit `lead` of q[0]: 0 wherever q has more than
    // one byte, so every byte index is a constant.
    template <int N>
    static __device__ __forceinline__ uint32_t sample(const ExpandBytes<N>& q, int j, int c, uint32_t lead) {
        if (SWAPPED) return q.half(j * CH + c);
        if (DEPTH == 16) return q.byte(2 * (j * CH + c)) << 8 | q.byte(2 * (j * CH + c) + 1);
        if (DEPTH == 8) return q.byte(j * CH + c);
        const uint32_t byte = q.byte(N == 1 ? 0 : (j * DEPTH) >> 3);
        return (byte >> (8 - DEPTH - ((lead + (uint32_t)j * DEPTH) & 7))) & MAXV;
    }

    // pixels x .. x + G - 1 of the run that starts at `in` (x a multiple of G): one load of QUAD bytes, 16-byte stores
    static __device__ __forceinline__ void quad(const uint8_t* in, uint64_t x, uint8_t* out, const ExpandKey& k, const uint32_t* pal, bool& bad) {
        ExpandBytes<QUAD> q;
        const uint64_t bit = x * BITS;
        q.load(in + (bit >> 3));
        if (SWAPPED) q.swap16();
        const uint32_t lead = G * BITS < 8 ? (uint32_t)bit & 7 : 0u;  // RGBA8: 4 with 1-bit pixels and an odd quad
        uint32_t o[G * OPX / 4];
#pragma unroll
        for (int j = 0; j < G; j++) {
            uint32_t s[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) s[c] = sample(q, j, c, lead);
            if constexpr (OPX == 4) {
                o[j] = pixel(s, k, pal, bad);
            } else {
                const uint2 p = pixel16(s, k, pal, bad);
                o[2 * j] = p.x;
                o[2 * j + 1] = p.y;
            }
        }
#pragma unroll
        for (int t = 0; t < G * OPX / 16; t++) {
            const uint4 v = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
            __builtin_memcpy(out + 16 * t, &v, 16);
        }
    }

    // pixel x of the run alone: the pixels in front of the first aligned store and behind the last whole quad
    static __device__ __forceinline__ void one(const uint8_t* in, uint64_t x, uint8_t* out, const ExpandKey& k, const uint32_t* pal, bool& bad) {
        constexpr int N = BITS >= 8 ? BITS / 8 : 1;
        ExpandBytes<N> q;
        const uint64_t bit = x * BITS;
        q.load(in + (bit >> 3));
        if (SWAPPED) q.swap16();
        uint32_t s[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) s[c] = sample(q, 0, c, (uint32_t)bit & 7);
        if constexpr (OPX == 4) {
            const uint32_t v = pixel(s, k, pal, bad);
            __builtin_memcpy(out, &v, 4);
        } else {
            const uint2 v = pixel16(s, k, pal, bad);
            __builtin_memcpy(out, &v, 8);
        }
    }
};

// The bands blockIdx.y, blockIdx.y + gridDim.y, .. of image i by the wavefront that calls this; `pal`: 256 words in the LDS.
template <int DEPTH, int COLOUR, int OPX = 4>
__device__ __forceinline__ void png_expand_image(const PngExpandArgs& a, uint64_t i, uint32_t lane, uint32_t* pal) {
    using E = Expand<DEPTH, COLOUR, OPX>;
    constexpr uint64_t G = E::G;
    const bool first = blockIdx.y == 0 && lane == 0;
    if (a.upstream) {
        const uint32_t up = uni(a.upstream[i]);
        if (up != 0) {
            if (first) a.status[i] = up;
            return;
        }
    }
    const uint64_t s0 = a.pix_off[i], s1 = a.pix_off[i + 1], o0 = a.rgba_off[i], o1 = a.rgba_off[i + 1];
    const uint64_t rb = a.row_bytes, width = a.width;
    const uint64_t rows = (s1 - s0) / rb;
    bool fits = rows * rb == s1 - s0 && o1 - o0 == rows * width * OPX;
    if (OPX == 8) fits = fits && (reinterpret_cast<uintptr_t>(a.rgba + o0) & 1) == 0;  // 16-bit samples in the device's order
    if (!fits) {
        if (first) a.status[i] = kPngBadSizes;
        return;
    }
    const uint64_t bands = (rows + kExpandBand - 1) / kExpandBand;
    if (blockIdx.y >= bands) return;
    ExpandKey k{256u, false, 0u, 0u, 0u};
    if (a.colour) {
        const uint32_t* c = a.colour + 4 * i;
        k.count = uni(c[0]);
        k.present = (uni(c[1]) & 1u) != 0;
        k.r = uni(c[2]) & E::MAXV;
        k.g = (uni(c[2]) >> 16) & E::MAXV;
        k.b = uni(c[3]) & E::MAXV;
    }
    if (COLOUR == 3) {
        for (uint32_t e = lane; e < 256; e += kWave) pal[e] = a.pal[i * 256 + e];
        __syncthreads();
    }
    const uint8_t* const __restrict__ img = a.pix + s0;
    uint8_t* const __restrict__ dst = a.rgba + o0;
    const bool flat = (width * E::BITS & 7) == 0;  // no padding bits: a band is one run of pixels
    const uint64_t qpr = (width + G - 1) / G;      // quads per row, the last one may be short
    bool bad = false;
    // quad qx of the run of `npix` pixels: whole, or its one to G - 1 pixels one by one
    auto item = [&](const uint8_t* in, uint8_t* out, uint64_t npix, uint64_t qx) {
        const uint64_t x = G * qx;
        if (npix - x >= G) E::quad(in, x, out + OPX * x, k, pal, bad);
        else
            for (uint64_t p = x; p < npix; p++) E::one(in, p, out + OPX * p, k, pal, bad);
    };
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kExpandBand, r1 = min(rows, r0 + kExpandBand);
        if (flat) {
            const uint64_t skip = r0 * width * E::BITS / 8;  // (whole bytes: width * BITS is a multiple of 8)
            const uint8_t* in = img + skip;
            uint8_t* out = dst + r0 * width * OPX;
            uint64_t npix = (r1 - r0) * width;
            if (E::BITS >= 8) {  // up to 16 / OPX - 1 pixels alone, so that the wide stores are aligned
                const uintptr_t at = reinterpret_cast<uintptr_t>(out);
                uint64_t head = (at & (OPX - 1)) ? 0 : ((0 - at) & 15) / OPX;
                if (head > npix) head = npix;
                if (lane < head) E::one(in, lane, out + OPX * lane, k, pal, bad);
                in += head * (E::BITS / 8);
                out += head * OPX;
                npix -= head;
            }
            const uint64_t quads = (npix + G - 1) / G;
#pragma unroll 2
            for (uint64_t qx = lane; qx < quads; qx += kWave) item(in, out, npix, qx);
        } else if (qpr >= kWave) {
            for (uint64_t r = r0; r < r1; r++)
                for (uint64_t qx = lane; qx < qpr; qx += kWave) item(img + r * rb, dst + r * width * OPX, width, qx);
        } else {
            const uint32_t q32 = (uint32_t)qpr, per = kWave / q32;  // rows per step
            const uint32_t lr = lane / q32, lq = lane - lr * q32;
            if (lr < per)
                for (uint64_t r = r0 + lr; r < r1; r += per) item(img + r * rb, dst + r * width * OPX, width, lq);
        }
    }
    if (COLOUR == 3 && __any(bad) && lane == 0) atomicOr(&a.status[i], kPngIndexOutsidePalette);
}

}  // namespace fdh
