// png_pack16.hip -- RGBA16 to the packed scanlines of the four pairs of depth 16 (include/fdeflate_hip_png16.h,
// fdh_png_pack16_batch): the exact inverse of png_expand16.hip for colour types 0, 2, 4 and 6, samples written
// big-endian.  tests/png16_model.py is the authority on every value.
//
// One kernel per colour type, grid(n, Y), one wavefront per workgroup that takes the bands b, b + Y, .. of kPack16Band
// rows of image i, as png_pack_kernel does.  Every pair has whole bytes per pixel, so a band is ONE run of pixels.  A
// lane takes kPack16Group pixels per step: 16-byte loads, aligned wherever the slot is 8-byte aligned (at most one
// pixel alone in front), the samples that the colour type keeps moved together in registers, both samples of a word
// swapped by one v_perm_b32, and one store of the 2 .. 8 bytes per pixel they pack to -- memory is only ever written in
// whole bytes, each by one lane.  A pixel without a lossless representation (R, G, B not all equal for colour types 0
// and 4, A != 65535 for 0 and 2): one atomicOr per wavefront that saw one.
#include "device_common.h"
#include "launch.h"
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

template <int COLOUR>
__global__ __launch_bounds__(kWave) void png_pack16_kernel(PngPack16Args a) {
    using P = Pack16<COLOUR>;
    constexpr uint64_t G = P::G;
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const bool first = blockIdx.y == 0 && lane == 0;
    if (a.upstream) {
        const uint32_t up = uni(a.upstream[i]);
        if (up != 0) {
            if (first) a.status[i] = up;
            return;
        }
    }
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

// As fdh_launch_png_pack: FDH_PNG_PACK16_WAVES sets the wavefronts per image; the statuses start at kPngOk and
// kPngNotRepresentable is OR-ed in.
extern "C" int fdh_launch_png_pack16(const uint8_t* rgba16, const uint64_t* rgba16_off, uint8_t* pix, const uint64_t* pix_off,
                                     const uint32_t* upstream, uint32_t* status, uint64_t n, uint32_t width, uint32_t colour_type,
                                     hipStream_t stream) {
    if (n == 0) return 0;
    hipError_t e = hipMemsetAsync(status, 0, n * 4, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t waves = fdh::png_waves_per_image(n, "FDH_PNG_PACK16_WAVES");
    fdh::PngPack16Args a{rgba16, rgba16_off, pix, pix_off, upstream, status, n, width};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
    switch (colour_type) {
        case 0: hipLaunchKernelGGL((fdh::png_pack16_kernel<0>), grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((fdh::png_pack16_kernel<2>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((fdh::png_pack16_kernel<4>), grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL((fdh::png_pack16_kernel<6>), grid, block, 0, stream, a); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}
