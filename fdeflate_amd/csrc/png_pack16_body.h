// png_pack16_body.h -- RGBA16 to the packed scanlines of the four pairs of depth 16 (include/fdeflate_hip_png16.h,
// fdh_png_pack16_batch) as a device function of one image, so that png_pack16.hip (one width and colour type per call)
// and png_encode16_mixed.hip (the geometry of each image in its fdh_png_info record) run the same code behind their own
// checks.  png_pack16.hip describes it; tests/png16_model.py is the authority on every value.
#pragma once
#include "device_common.h"
#include "png_common.h"

namespace fdh {

constexpr uint32_t kPack16Band = 64;  // rows per band, as kExpandBand
// Pixels per lane and step.  4: two 16-byte loads and stores of 8 .. 32 bytes; 2: one load, stores of 4 .. 16 bytes.  4 is
// the faster one here, where the narrow side is the stores; -DFDH_PACK16_GROUP=2 builds the other shape.
#ifndef FDH_PACK16_GROUP
#define FDH_PACK16_GROUP 4
#endif
constexpr int kPack16Group = FDH_PACK16_GROUP;
static_assert(kPack16Group == 2 || kPack16Group == 4, "whole 16-byte loads");

struct PngPack16Args {
    const uint8_t* rgba16;
    const uint64_t* rgba16_off;  // n + 1
    uint8_t* pix;
    const uint64_t* pix_off;     // n + 1
    const uint32_t* upstream;    // nullable
    uint32_t* status;            // zeroed by the launcher
    uint64_t n;
    uint32_t width;
};

template <int COLOUR>
struct Pack16 {
    static constexpr int CH = (int)png_channels(COLOUR);
    static constexpr int PIXEL = 2 * CH;  // bytes of one packed pixel
    static constexpr int G = kPack16Group;

    // NPIX pixels (x = R | G << 16, y = B | A << 16 each) as NPIX * CH samples of 16 bits, two to a word, then big-endian
    template <int NPIX>
    static __device__ __forceinline__ void pack(const uint32_t (&v)[2 * NPIX], uint8_t* out, bool& bad) {
        constexpr int WORDS = (NPIX * CH + 1) / 2;
        uint32_t w[WORDS];
#pragma unroll
        for (int t = 0; t < WORDS; t++) w[t] = 0;
#pragma unroll
        for (int j = 0; j < NPIX; j++) {
            const uint32_t r = v[2 * j] & 0xFFFFu, g = v[2 * j] >> 16, b = v[2 * j + 1] & 0xFFFFu, al = v[2 * j + 1] >> 16;
            if (COLOUR == 0 || COLOUR == 2) bad = bad || al != 0xFFFFu;
            if (COLOUR == 0 || COLOUR == 4) bad = bad || r != g || g != b;
            uint32_t s[CH];
            s[0] = r;
            if (COLOUR == 2 || COLOUR == 6) {
                s[CH > 1 ? 1 : 0] = g;
                s[CH > 2 ? 2 : 0] = b;
            }
            if (COLOUR == 4 || COLOUR == 6) s[CH - 1] = al;
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const int at = j * CH + c;
                w[at >> 1] |= s[c] << (16 * (at & 1));
            }
        }
#pragma unroll
        for (int t = 0; t < WORDS; t++) w[t] = __builtin_amdgcn_perm(w[t], w[t], 0x02030001u);
        __builtin_memcpy(out, w, NPIX * PIXEL);  // any alignment
    }

    // pixels x .. x + G - 1 of the run at `in`: G / 2 loads of 16 bytes, one store of G * PIXEL bytes
    static __device__ __forceinline__ void group(const uint8_t* in, uint64_t x, uint8_t* out, bool& bad) {
        uint32_t v[2 * G];
        __builtin_memcpy(v, in + 8 * x, 8 * G);
        pack<G>(v, out + x * PIXEL, bad);
    }

    static __device__ __forceinline__ void one(const uint8_t* in, uint64_t x, uint8_t* out, bool& bad) {
        uint32_t v[2];
        __builtin_memcpy(v, in + 8 * x, 8);
        pack<1>(v, out + x * PIXEL, bad);
    }
};

// Image i of the call at a.width, behind the caller's look at upstream: the slots' check, the bands blockIdx.y,
// blockIdx.y + gridDim.y, ..
template <int COLOUR>
__device__ __forceinline__ void png_pack16_image(const PngPack16Args& a, uint64_t i, uint32_t lane) {
    using P = Pack16<COLOUR>;
    constexpr uint64_t G = P::G;
    const bool first = blockIdx.y == 0 && lane == 0;
    const uint64_t s0 = a.rgba16_off[i], s1 = a.rgba16_off[i + 1], o0 = a.pix_off[i], o1 = a.pix_off[i + 1];
    const uint64_t width = a.width, rb = width * P::PIXEL;
    const uint64_t rows = (s1 - s0) / (width * 8);
    const bool fits = rows * width * 8 == s1 - s0 && o1 - o0 == rows * rb && (reinterpret_cast<uintptr_t>(a.rgba16 + s0) & 1) == 0;
    if (!fits) {
        if (first) a.status[i] = kPngBadSizes;
        return;
    }
    const uint64_t bands = (rows + kPack16Band - 1) / kPack16Band;
    const uint8_t* const __restrict__ img = a.rgba16 + s0;
    uint8_t* const __restrict__ dst = a.pix + o0;
    bool bad = false;
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kPack16Band, r1 = min(rows, r0 + kPack16Band);
        const uint8_t* in = img + r0 * width * 8;
        uint8_t* out = dst + r0 * rb;
        uint64_t npix = (r1 - r0) * width;
        const uintptr_t at = reinterpret_cast<uintptr_t>(in);  // at most one pixel alone: the wide loads are aligned
        uint64_t head = (at & 7) ? 0 : ((0 - at) & 15) >> 3;
        if (head > npix) head = npix;
        if (lane < head) P::one(in, lane, out, bad);
        in += head * 8;
        out += head * P::PIXEL;
        npix -= head;
        const uint64_t groups = (npix + G - 1) / G;
#pragma unroll 2
        for (uint64_t qx = lane; qx < groups; qx += kWave) {
            if (npix - G * qx >= G) P::group(in, G * qx, out, bad);
            else
                for (uint64_t p = G * qx; p < npix; p++) P::one(in, p, out, bad);
        }
    }
    if (__any(bad) && lane == 0) atomicOr(&a.status[i], kPngNotRepresentable);
}

}  // namespace fdh
