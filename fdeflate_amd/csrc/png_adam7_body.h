// png_adam7_body.h -- the reconstruction and the placement of png_adam7.hip as device functions of one image, so that
// png_adam7.hip (one geometry per call, in the kernel's arguments) and png_mixed.hip (the geometry of each image in its
// fdh_png_info record) run the same code.  png_adam7.hip describes both steps.
#pragma once
#include "device_common.h"
#include "launch.h"
#include "png_common.h"
#include "png_rows.h"

namespace fdh {

struct Adam7Args {
    uint8_t* filt;
    const uint64_t* filt_off;  // n + 1
    uint8_t* pix;
    const uint64_t* pix_off;   // n + 1
    const uint8_t* method;     // nullable (all 1): 0 progressive, 1 Adam7
    const uint32_t* upstream;      // nullable: the decoder's status
    const uint32_t* upstream_len;  // nullable: the decoder's out_len
    uint32_t* status;
    uint64_t n;
    uint64_t row_bytes;  // of the picture
    uint32_t width;
    uint32_t bits;       // per pixel
};

// What both kernels know of image i: its slots, its height, its method and its status before any filter type is seen.
struct Adam7Image {
    uint64_t f0, d0, height;
    uint32_t method, status;
};

__device__ __forceinline__ Adam7Image adam7_image(const Adam7Args& a, uint64_t i) {
    Adam7Image g;
    const uint64_t f1 = a.filt_off[i + 1], d1 = a.pix_off[i + 1];
    g.f0 = a.filt_off[i];
    g.d0 = a.pix_off[i];
    g.method = a.method ? a.method[i] : 1u;
    g.height = (d1 - g.d0) / a.row_bytes;
    g.status = kPngOk;
    if (a.upstream && a.upstream[i] != 0) g.status = kPngSkipped;
    else if (a.upstream_len && (uint64_t)a.upstream_len[i] != f1 - g.f0) g.status = kPngBadSizes;
    else if (g.method > 1 || g.height * a.row_bytes != d1 - g.d0) g.status = kPngBadSizes;
    else {  // png_adam7_size(a.width, g.height, a.bits, g.method), written out: as a call all fifteen kernels compile to other code
        uint64_t total = 0;
#pragma unroll
        for (uint32_t p = 0; p < 7; p++) {
            uint64_t pw, ph;
            adam7_pass_dims(g.method, p, a.width, g.height, pw, ph);
            total += ph * (1 + png_row_bytes(pw, a.bits));  // (an empty pass: 0 rows)
        }
        if (total != f1 - g.f0) g.status = kPngBadSizes;
    }
    return g;
}

// Reconstruction of image i in place by the wavefront that calls this; `g` is what adam7_image (or the caller's own
// reading of the image's record) says of it.
template <int BPP>
__device__ __forceinline__ void adam7_recon_image(const Adam7Args& a, const Adam7Image& g, uint64_t i, uint32_t lane) {
    if (g.status != kPngOk) {
        if (lane == 0) a.status[i] = g.status;
        return;
    }
    uint64_t rows = 0;  // of all passes
#pragma unroll
    for (uint32_t p = 0; p < 7; p++) {
        uint64_t pw, ph;
        adam7_pass_dims(g.method, p, a.width, g.height, pw, ph);
        rows += ph;
    }
    uint8_t* const img = a.filt + g.f0;
    bool bad = false;
    for (uint64_t R0 = 0; R0 < rows; R0 += kWave) {
        // ---- this lane's row of the list: where it lies, how long it is, whether its pass starts with it ----
        const uint64_t R = R0 + lane;
        const bool mine = R < rows;
        uint64_t at = 0, len = 0;
        bool first = true;
        {
            uint64_t before = 0, base = 0;  // rows / bytes of the passes in front
#pragma unroll
            for (uint32_t p = 0; p < 7; p++) {
                uint64_t pw, ph;
                adam7_pass_dims(g.method, p, a.width, g.height, pw, ph);
                const uint64_t stride = 1 + png_row_bytes(pw, a.bits);
                if (R >= before && R < before + ph) {
                    at = base + (R - before) * stride + 1;
                    len = stride - 1;
                    first = R == before;
                }
                before += ph;
                base += ph * stride;
            }
        }
        uint8_t* const row = img + at;           // first filtered byte (behind the type byte)
        const uint8_t* const up = row - len - 1;  // the row above, reconstructed (lane 0 of a later band reads it)
        uint32_t t = 0;
        if (mine) t = row[-1];
        if (__ballot(mine && t > 4)) bad = true;  // (such a row is taken as type 0: the slot's contents are not specified)
        const PngMasks m(t);
        uint32_t la[8], ua[8];
#pragma unroll
        for (int k = 0; k < 8; k++) la[k] = ua[k] = 0;
        const uint32_t nchunks = mine ? (uint32_t)((len + 15) / 16) : 0u;
        const uint32_t steps = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(nchunks ? nchunks + lane : 0u), kWave - 1);
        const bool from_memory = lane == 0 && !first;
        uint4 fnext = make_uint4(0, 0, 0, 0), unext = fnext, last = fnext;
        // step s: chunk s - lane - 1 is reconstructed and chunk s - lane is loaded for the step after
        for (uint32_t s = 0; s <= steps; s++) {
            const uint32_t c = s - lane - 1;  // (wraps for the lanes that have not started)
            const bool on = mine && c < nchunks;
            const uint4 f = fnext;
            uint4 u = make_uint4(png_from_lane_below(last.x), png_from_lane_below(last.y), png_from_lane_below(last.z), png_from_lane_below(last.w));
            if (from_memory) u = unext;
            if (first) u = make_uint4(0, 0, 0, 0);
            if (mine && c + 1 < nchunks) {
                const uint64_t o = (uint64_t)(c + 1) * 16;
                const uint32_t valid = (uint32_t)min((uint64_t)16, len - o);
                fnext = png_load_part(row + o, valid);
                if (from_memory) unext = png_load_part(up + o, valid);
            }
            if (on) {
                const uint64_t o = (uint64_t)c * 16;
                last = png_chunk<BPP, true>(f, u, la, ua, m);
                png_store_part(row + o, last, (uint32_t)min((uint64_t)16, len - o));
            }
        }
        // the next band's first row reads this band's last row back
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) a.status[i] = bad ? kPngBadFilterType : kPngOk;
}

// The pass rows an even picture row y draws on, by the column's class: odd x; x % 4 == 2; x % 8 == 4; x % 8 == 0.
struct Adam7RowSources {
    const uint8_t* ptr[4];  // first pixel byte of the pass row
    uint32_t shift[4];      // log2 of the pass's column step
};

// BITS >= 8: U bytes of a pixel at a time.  BITS < 8: bit fields.
template <int BITS>
struct Adam7Place {
    static constexpr int B = (int)png_bpp(BITS);                                        // bytes per pixel
    static constexpr int U = B % 8 == 0 ? 8 : B % 4 == 0 ? 4 : B % 2 == 0 ? 2 : 1;      // bytes per load
    static constexpr int PPB = BITS >= 8 ? 1 : 8 / BITS;                                // pixels per byte

    static __device__ __forceinline__ uint32_t cls(uint64_t x) {
        const uint32_t l = (uint32_t)x & 7u;
        return (l & 1u) ? 0u : (l & 2u) ? 1u : (l & 4u) ? 2u : 3u;
    }
    // (vsel, not ?: -- hipcc turns a chain of selects over the struct's fields into an indexed load from a scratch copy of it)
    static __device__ __forceinline__ const uint8_t* pick(const Adam7RowSources& s, uint32_t k, uint32_t& shift) {
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint64_t v = reinterpret_cast<uint64_t>(s.ptr[c]);
            lo[c] = (uint32_t)v, hi[c] = (uint32_t)(v >> 32);
        }
        const bool k0 = k == 0, k1 = k == 1, k2 = k == 2;
        shift = vsel(k0, s.shift[0], vsel(k1, s.shift[1], vsel(k2, s.shift[2], s.shift[3])));
        const uint32_t l = vsel(k0, lo[0], vsel(k1, lo[1], vsel(k2, lo[2], lo[3])));
        const uint32_t h = vsel(k0, hi[0], vsel(k1, hi[1], vsel(k2, hi[2], hi[3])));
        return reinterpret_cast<const uint8_t*>(((uint64_t)h << 32) | l);
    }

    // the `valid` (1 .. 16) bytes of the picture row from byte `ob` on
    static __device__ __forceinline__ uint4 gather(const Adam7RowSources& s, uint64_t ob, uint32_t valid, uint64_t width) {
        uint32_t w[4] = {0, 0, 0, 0};
        if constexpr (BITS >= 8) {
            const uint64_t x0 = ob / B;
            const uint32_t sub0 = (uint32_t)(ob - x0 * B);
#pragma unroll
            for (int k = 0; k < 16 / U; k++) {
                if ((uint32_t)(k * U) < valid) {  // (rows are whole pixels and U divides a pixel: a unit is valid or not as a whole)
                    const uint32_t q = sub0 + k * U;
                    const uint64_t x = x0 + q / B;
                    uint32_t shift;
                    const uint8_t* p = pick(s, cls(x), shift) + (x >> shift) * B + q % B;
                    if constexpr (U == 8) {
                        uint64_t v;
                        __builtin_memcpy(&v, p, 8);
                        w[2 * k] = (uint32_t)v;
                        w[2 * k + 1] = (uint32_t)(v >> 32);
                    } else if constexpr (U == 4) {
                        uint32_t v;
                        __builtin_memcpy(&v, p, 4);
                        w[k] = v;
                    } else if constexpr (U == 2) {
                        uint16_t v;
                        __builtin_memcpy(&v, p, 2);
                        w[k / 2] |= (uint32_t)v << (16 * (k & 1));
                    } else {
                        w[k / 4] |= (uint32_t)p[0] << (8 * (k & 3));
                    }
                }
            }
        } else {
            constexpr uint32_t mask = (1u << BITS) - 1;
            uint64_t lo = 0, hi = 0;
            for (uint32_t k = 0; k < valid; k++) {
                uint32_t byte = 0;
#pragma unroll
                for (int j = 0; j < PPB; j++) {
                    const uint64_t x = (ob + k) * PPB + j;
                    if (x < width) {  // (behind the row's last pixel: padding bits, zero)
                        uint32_t shift;
                        const uint8_t* p = pick(s, cls(x), shift);
                        const uint64_t bit = (x >> shift) * BITS;
                        byte |= (((uint32_t)p[bit >> 3] >> (8 - BITS - ((uint32_t)bit & 7u))) & mask) << (8 - BITS - j * BITS);
                    }
                }
                if (k < 8) lo |= (uint64_t)byte << (8 * k);
                else hi |= (uint64_t)byte << (8 * (k - 8));
            }
            w[0] = (uint32_t)lo, w[1] = (uint32_t)(lo >> 32), w[2] = (uint32_t)hi, w[3] = (uint32_t)(hi >> 32);
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
};

constexpr uint32_t kPlaceBand = 64;  // picture rows per band: one band = one image of the bench shape

// Placement of the bands blockIdx.y, blockIdx.y + gridDim.y, .. of image i by the wavefront that calls this.  s_base and
// s_stride, seven words each in the LDS: of pass p, where its first type byte lies in the filt slot; 1 + row bytes.
template <int BITS>
__device__ __forceinline__ void adam7_place_image(const Adam7Args& a, const Adam7Image& g, uint32_t lane, uint64_t* s_base, uint64_t* s_stride) {
    if (g.status != kPngOk) return;
    const uint64_t rb = a.row_bytes, rows = g.height;
    const uint64_t bands = (rows + kPlaceBand - 1) / kPlaceBand;
    if (blockIdx.y >= bands) return;
    if (lane == 0) {
        uint64_t base = 0;
        for (uint32_t p = 0; p < 7; p++) {
            uint64_t pw, ph;
            adam7_pass_dims(g.method, p, a.width, rows, pw, ph);
            s_base[p] = base;
            s_stride[p] = 1 + png_row_bytes(pw, a.bits);
            base += ph * s_stride[p];
        }
    }
    __syncthreads();
    const uint8_t* const img = a.filt + g.f0;
    uint8_t* const dst = a.pix + g.d0;
    const uint32_t method = g.method;
    const uint64_t width = a.width;
    auto pass_row = [&](uint32_t p, uint64_t y) { return img + s_base[p] + (y >> adam7_nib(kAdam7LogDy, p)) * s_stride[p] + 1; };
    // the sixteen bytes of row y from byte 16 q on
    auto item = [&](uint64_t y, uint64_t q) {
        const uint64_t ob = q * 16;
        const uint32_t valid = (uint32_t)min((uint64_t)16, rb - ob);
        uint8_t* const out = dst + y * rb + ob;
        if (method == 0 || (y & 1)) {  // one pass row holds the whole picture row
            const uint8_t* const src = method == 0 ? img + y * (rb + 1) + 1 : pass_row(6, y);
            uint4 v = png_load_part(src + ob, valid);
            if constexpr (BITS < 8) {
                // a row of pass 7 may carry anything in its padding bits; the picture's are zero, as on the even rows
                // (a progressive image keeps them as they come, as fdh_png_unfilter_batch does)
                const uint32_t used = (uint32_t)(width * BITS) & 7u;
                if (method != 0 && used != 0 && ob + valid == rb) {
                    const uint32_t k = valid - 1, clear = ~((0xFFu >> used) << (8 * (k & 3)));
                    v.x &= k < 4 ? clear : ~0u;
                    v.y &= (k >= 4 && k < 8) ? clear : ~0u;
                    v.z &= (k >= 8 && k < 12) ? clear : ~0u;
                    v.w &= k >= 12 ? clear : ~0u;
                }
            }
            png_store_part(out, v, valid);
            return;
        }
        // passes, 0-based, by the row: odd x pass 5; then y % 4 == 2: 4 everywhere; y % 8 == 4: 3, 2, 2; y % 8 == 0: 3, 1, 0
        const uint32_t p1 = (y & 2) ? 4u : 3u, p2 = (y & 2) ? 4u : (y & 4) ? 2u : 1u, p3 = (y & 2) ? 4u : (y & 4) ? 2u : 0u;
        Adam7RowSources s;
        s.ptr[0] = pass_row(5, y), s.ptr[1] = pass_row(p1, y), s.ptr[2] = pass_row(p2, y), s.ptr[3] = pass_row(p3, y);
        s.shift[0] = 1, s.shift[1] = adam7_nib(kAdam7LogDx, p1), s.shift[2] = adam7_nib(kAdam7LogDx, p2), s.shift[3] = adam7_nib(kAdam7LogDx, p3);
        png_store_part(out, Adam7Place<BITS>::gather(s, ob, valid, width), valid);
    };
    const uint64_t cpr = (rb + 15) / 16;  // chunks per row
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kPlaceBand, r1 = min(rows, r0 + kPlaceBand);
        if (cpr >= kWave) {
            for (uint64_t y = r0; y < r1; y++)
                for (uint64_t q = lane; q < cpr; q += kWave) item(y, q);
        } else {  // rows of fewer than 64 chunks share a step
            const uint32_t c32 = (uint32_t)cpr, per = kWave / c32;
            const uint32_t lr = lane / c32, lq = lane - lr * c32;
            if (lr < per)
                for (uint64_t y = r0 + lr; y < r1; y += per) item(y, lq);
        }
    }
}

}  // namespace fdh
