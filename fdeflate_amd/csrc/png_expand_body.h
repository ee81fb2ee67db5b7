// png_expand_body.h -- the expansion of png_expand.hip as a device function of one image, so that png_expand.hip (one
// geometry per call) and png_mixed.hip (the geometry of each image in its fdh_png_info record) run the same code.
// png_expand.hip describes it.
#pragma once
#include "device_common.h"
#include "launch.h"
#include "png_common.h"

namespace fdh {

constexpr uint32_t kExpandBand = 64;  // rows per band: one band = one image of the bench shape

struct PngExpandArgs {
    const uint8_t* pix;
    const uint64_t* pix_off;   // n + 1
    uint8_t* rgba;
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
};

template <int DEPTH, int COLOUR>
struct Expand {
    static constexpr int CH = (int)png_channels(COLOUR);
    static constexpr int BITS = (int)png_pixel_bits(DEPTH, COLOUR);  // per pixel
    static constexpr int QUAD = BITS * 4 / 8 ? BITS * 4 / 8 : 1;  // bytes that hold four pixels (1-bit: half of one)
    static constexpr uint32_t MAXV = (1u << DEPTH) - 1;

    static __device__ __forceinline__ uint32_t to8(uint32_t s) {
        if (DEPTH == 16) return s >> 8;
        if (DEPTH == 8) return s;
        return s * (255u / MAXV);
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

    // sample c of pixel j of the bytes q.  Below 8 bits pixel 0 starts at bit `lead` of q[0]: 0 wherever q has more than
    // one byte, so every byte index is a constant.
    template <int N>
    static __device__ __forceinline__ uint32_t sample(const ExpandBytes<N>& q, int j, int c, uint32_t lead) {
        if (DEPTH == 16) return q.byte(2 * (j * CH + c)) << 8 | q.byte(2 * (j * CH + c) + 1);
        if (DEPTH == 8) return q.byte(j * CH + c);
        const uint32_t byte = q.byte(N == 1 ? 0 : (j * DEPTH) >> 3);
        return (byte >> (8 - DEPTH - ((lead + (uint32_t)j * DEPTH) & 7))) & MAXV;
    }

    // pixels x .. x + 3 of the run that starts at `in` (x a multiple of four): one load of QUAD bytes, one 16-byte store
    static __device__ __forceinline__ void quad(const uint8_t* in, uint64_t x, uint8_t* out, const ExpandKey& k, const uint32_t* pal, bool& bad) {
        ExpandBytes<QUAD> q;
        const uint64_t bit = x * BITS;
        q.load(in + (bit >> 3));
        const uint32_t lead = DEPTH == 1 ? (uint32_t)bit & 7 : 0u;  // 4 with 1-bit pixels and an odd quad
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t s[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) s[c] = sample(q, j, c, lead);
            o[j] = pixel(s, k, pal, bad);
        }
        const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
        __builtin_memcpy(out, &v, 16);
    }

    // pixel x of the run alone: the pixels in front of the first aligned store and behind the last whole quad
    static __device__ __forceinline__ void one(const uint8_t* in, uint64_t x, uint8_t* out, const ExpandKey& k, const uint32_t* pal, bool& bad) {
        constexpr int N = BITS >= 8 ? BITS / 8 : 1;
        ExpandBytes<N> q;
        const uint64_t bit = x * BITS;
        q.load(in + (bit >> 3));
        uint32_t s[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) s[c] = sample(q, 0, c, (uint32_t)bit & 7);
        const uint32_t v = pixel(s, k, pal, bad);
        __builtin_memcpy(out, &v, 4);
    }
};

// The bands blockIdx.y, blockIdx.y + gridDim.y, .. of image i by the wavefront that calls this; `pal`: 256 words in the LDS.
template <int DEPTH, int COLOUR>
__device__ __forceinline__ void png_expand_image(const PngExpandArgs& a, uint64_t i, uint32_t lane, uint32_t* pal) {
    using E = Expand<DEPTH, COLOUR>;
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
    const bool fits = rows * rb == s1 - s0 && o1 - o0 == rows * width * 4;
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
    const uint64_t qpr = (width + 3) / 4;          // quads per row, the last one may be short
    bool bad = false;
    // quad qx of the run of `npix` pixels: whole, or its one to three pixels one by one
    auto item = [&](const uint8_t* in, uint8_t* out, uint64_t npix, uint64_t qx) {
        const uint64_t x = 4 * qx;
        if (npix - x >= 4) E::quad(in, x, out + 4 * x, k, pal, bad);
        else
            for (uint64_t p = x; p < npix; p++) E::one(in, p, out + 4 * p, k, pal, bad);
    };
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kExpandBand, r1 = min(rows, r0 + kExpandBand);
        if (flat) {
            const uint64_t skip = r0 * width * E::BITS / 8;  // (whole bytes: width * BITS is a multiple of 8)
            const uint8_t* in = img + skip;
            uint8_t* out = dst + r0 * width * 4;
            uint64_t npix = (r1 - r0) * width;
            if (E::BITS >= 8) {  // up to three pixels alone, so that the wide stores are aligned
                const uintptr_t at = reinterpret_cast<uintptr_t>(out);
                uint64_t head = (at & 3) ? 0 : ((0 - at) & 15) >> 2;
                if (head > npix) head = npix;
                if (lane < head) E::one(in, lane, out + 4 * lane, k, pal, bad);
                in += head * (E::BITS / 8);
                out += head * 4;
                npix -= head;
            }
            const uint64_t quads = (npix + 3) / 4;
#pragma unroll 2
            for (uint64_t qx = lane; qx < quads; qx += kWave) item(in, out, npix, qx);
        } else if (qpr >= kWave) {
            for (uint64_t r = r0; r < r1; r++)
                for (uint64_t qx = lane; qx < qpr; qx += kWave) item(img + r * rb, dst + r * width * 4, width, qx);
        } else {
            const uint32_t q32 = (uint32_t)qpr, per = kWave / q32;  // rows per step
            const uint32_t lr = lane / q32, lq = lane - lr * q32;
            if (lr < per)
                for (uint64_t r = r0 + lr; r < r1; r += per) item(img + r * rb, dst + r * width * 4, width, lq);
        }
    }
    if (COLOUR == 3 && __any(bad) && lane == 0) atomicOr(&a.status[i], kPngIndexOutsidePalette);
}

}  // namespace fdh
