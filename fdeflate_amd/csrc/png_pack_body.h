// png_pack_body.h -- PNG encode from RGBA8 (include/fdeflate_hip.h, "PNG encode from RGBA8"): what an RGBA8 image is and
// its sorted palette (png_analyse_image), and RGBA8 to the packed scanlines of a depth / colour pair (png_pack_image),
// the exact inverse of png_expand_body.h, as device functions of one image: png_pack.hip (one geometry per call) and
// png_encode_mixed.hip (the geometry of each image in its fdh_png_info record) run the same code behind their own
// checks.  tests/png_pack_model.py is the authority on every value.  png_encode16_mixed.hip runs the same two bodies on
// RGBA16 pictures (include/fdeflate_hip_png16_encode.h): PixelSource below is all that differs.
//
// Analysis: one workgroup per image, 1 .. 16 wavefronts.  The distinct pixel words live in an LDS open-addressed table
// (linear probing, insertion by compare-and-swap); a lane reads four pixels with one 16-byte load and probes only for a
// pixel that differs from the one in front of it.  The summary (opaque, grey, sample depth) is three OR-ed difference
// masks and an AND over the words.  Once more than max_colours keys are in, insertion stops and the summary goes on.
// At the end the at most 256 keys are ranked against each other in the LDS and written in ascending order: the result
// does not depend on which lane saw which pixel first.
//
// Packing: one kernel per (bit depth, colour type) pair, grid(n, Y), one wavefront per workgroup that takes the bands
// b, b + Y, .. of kPackBand rows of image i, as png_expand_kernel does.  A lane takes four pixels per step: ONE 16-byte
// load, and a store of the 0.5 .. 32 bytes they pack to.  Rows whose bits fill whole bytes have no padding: a band is
// then ONE run of pixels.  Below eight bits per pixel a lane's four pixels are 4, 8 or 16 bits: two bytes or one are
// stored by the lane itself, and the two halves of a byte of 1-bit pixels meet in the even lane through a DPP move --
// memory is only ever written in whole bytes, each by one lane.  Colour type 3: the workgroup hashes the caller's 256
// palette words into the LDS once (the lowest index of equal words wins) and a lane tries the previous pixel's answer
// before it probes.  A pixel without a lossless representation: one atomicOr per wavefront that saw one.
#pragma once
#include "device_common.h"
#include "png_common.h"

namespace fdh {

// Both tables hash a pixel word R | G << 8 | B << 16 | A << 24 the same way: the top bits of a multiplicative hash
// (fdeflate_amd/api.py names the multiplier and the analysis table's size for the tests that build collisions).
constexpr uint32_t kColourHashMul = 0x9E3779B1u;
__device__ __forceinline__ uint32_t colour_hash(uint32_t w, uint32_t bits) { return (w * kColourHashMul) >> (32 - bits); }

__device__ __forceinline__ uint32_t lds_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// ---- where the pixel words come from ----
// Both bodies below work on pixel words R | G << 8 | B << 16 | A << 24 and read them through PixelSource<SPX>, SPX the
// bytes of a pixel in memory.  4: RGBA8, the word is the pixel.  8: RGBA16 (include/fdeflate_hip_png16_encode.h), two
// words x = R | G << 16, y = B | A << 16 of samples in the device's byte order: the pixel word is their four high bytes,
// moved together by one v_perm_b32, and Seen keeps what the high bytes do not show -- which samples are not narrow (the
// two bytes differ: (w ^ (w >> 8)) & 0x00FF00FF on a word of two samples), R ^ G and G ^ B on all 16 bits, and the AND of
// the y words (alpha).  Four pixels are one 16-byte load or two.  A body that does not read a field of Seen does not
// pay for it.
template <int SPX>
struct PixelSource;

template <>
struct PixelSource<4> {
    struct Seen {};
    template <int N>
    static __device__ __forceinline__ void load(const uint8_t* in, uint64_t x, uint32_t (&v)[N], Seen&) {
        __builtin_memcpy(v, in + 4 * x, 4 * N);
    }
};

template <>
struct PixelSource<8> {
    struct Seen {
        uint32_t wide = 0;          // byte 0, 2, 1, 3: the bits in which the two bytes of an R, G, B, A differed
        uint32_t grey = 0;          // (R ^ G) | (G ^ B), 16 bits
        uint32_t all = 0xFFFFFFFFu; // AND of B | A << 16
    };
    template <int N>
    static __device__ __forceinline__ void load(const uint8_t* in, uint64_t x, uint32_t (&v)[N], Seen& s) {
        uint32_t t[2 * N];
        __builtin_memcpy(t, in + 8 * x, 8 * N);
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint32_t rg = t[2 * j], ba = t[2 * j + 1];
            s.wide |= ((rg ^ (rg >> 8)) & 0x00FF00FFu) | ((ba ^ (ba >> 8)) & 0x00FF00FFu) << 8;
            s.grey |= ((rg ^ (rg >> 16)) | ((rg >> 16) ^ ba)) & 0xFFFFu;
            s.all &= ba;
            v[j] = __builtin_amdgcn_perm(ba, rg, 0x07050301u);  // bytes 1 and 3 of rg, then of ba
        }
    }
};

// the pixels in front of the first 16-byte boundary of a run at `at`, handled alone so that the wide loads are aligned:
// up to three of four bytes, at most one of eight; none where the run is not even aligned to its own pixels
template <int SPX>
__device__ __forceinline__ uint64_t pixels_in_front(uintptr_t at) {
    return (at & (SPX - 1)) ? 0 : ((0 - at) & 15) / SPX;
}

// ---- fdh_png_analyse_batch ----
// 256 keys that count, and at most one more per lane that passed the overflow test before the count moved: 1280 of 2048.
constexpr uint32_t kAnalyseSlotBits = 11, kAnalyseSlots = 1u << kAnalyseSlotBits, kAnalyseMaxThreads = 1024;
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;  // no table slot can hold this word (opaque white): it has a flag of its own
static_assert(256 + kAnalyseMaxThreads < kAnalyseSlots, "the table never fills up");

struct PngAnalyseArgs {
    const uint8_t* rgba;
    const uint64_t* rgba_off;  // n + 1
    uint32_t* pal;             // nullable: 256 words per image
    uint32_t* colour;          // 4 words per image
    uint32_t* trns_len;
    uint32_t* summary;
    uint32_t* status;
    uint64_t n;
    uint32_t width, max_colours;
};

enum AnalyseWord { kAwCount, kAwWhite, kAwAnd, kAwGrey, kAwD4, kAwD2, kAwD1, kAwKeys, kAwTrns, kAwWords };
constexpr uint32_t kAwWide = kAwWords, kAwWords16 = kAwWords + 1;  // RGBA16: one word more, PixelSource<8>::Seen::wide

// Image i of the call; table (kAnalyseSlots words), keys (256) and sh (kAwWords; kAwWords16 where SPX is 8) are the
// workgroup's LDS.  SPX = 8 (fdh_png_analyse16_mixed_batch): a.rgba holds RGBA16 pictures; the set, the palette and the
// depth masks are those of the high bytes, opaque and grey are decided on all 16 bits, the depth is 16 once an R, G or B
// is not narrow, and a picture with any sample that is not narrow ends as one with too many colours does.
template <int SPX = 4>
__device__ __forceinline__ void png_analyse_image(const PngAnalyseArgs& a, uint64_t i, uint32_t* table, uint32_t* keys, uint32_t* sh) {
    using Src = PixelSource<SPX>;
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
    const uint64_t o0 = a.rgba_off[i], bytes = a.rgba_off[i + 1] - o0;
    if (bytes % ((uint64_t)a.width * SPX) != 0) {
        if (tid == 0) a.status[i] = kPngBadSizes;
        return;
    }
    for (uint32_t s = tid; s < kAnalyseSlots; s += T) table[s] = kEmptyKey;
    if (tid < (SPX == 8 ? kAwWords16 : kAwWords)) sh[tid] = tid == kAwAnd ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint32_t maxc = a.max_colours;
    typename Src::Seen seen;
    bool told = false;  // (SPX 8) this lane has said that it saw a sample that is not narrow
    uint32_t all = 0xFFFFFFFFu, grey = 0, d4 = 0, d2 = 0, d1 = 0;
    bool white = false;
    // every pixel: the AND of the words (alpha), R ^ G and G ^ B, and which bits of R, G, B differ from the bits that a
    // sample of 4, 2, 1 bits repeats (a multiple of 17 has equal nibbles, of 85 equal bit pairs, of 255 equal bits)
    auto note = [&](uint32_t w) {
        all &= w;
        grey |= (w ^ (w >> 8)) & 0xFFFFu;
        d4 |= ((w >> 4) ^ w) & 0x0F0F0Fu;
        d2 |= ((w >> 2) ^ w) & 0x030303u;
        d1 |= ((w >> 1) ^ w) & 0x010101u;
    };
    auto insert = [&](uint32_t w) {
        if (w == kEmptyKey) {
            if (!white && atomicExch(&sh[kAwWhite], 1u) == 0) atomicAdd(&sh[kAwCount], 1u);
            white = true;
            return;
        }
        if (lds_load(&sh[kAwCount]) > maxc) return;  // overflow is decided: only the summary goes on
        if constexpr (SPX == 8) {  // ... and so it is once the workgroup has seen a sample that is not narrow
            if (seen.wide && !told) atomicOr(&sh[kAwWide], seen.wide), told = true;
            if (lds_load(&sh[kAwWide])) return;
        }
        uint32_t h = colour_hash(w, kAnalyseSlotBits);
        for (uint32_t p = 0; p < kAnalyseSlots; p++, h = (h + 1) & (kAnalyseSlots - 1)) {
            uint32_t cur = lds_load(&table[h]);
            if (cur == kEmptyKey) {
                cur = atomicCAS(&table[h], kEmptyKey, w);
                if (cur == kEmptyKey) {
                    atomicAdd(&sh[kAwCount], 1u);
                    return;
                }
            }
            if (cur == w) return;
        }
    };
    const uint8_t* img = a.rgba + o0;
    uint64_t npix = bytes / SPX;
    {  // up to three pixels alone (one of eight bytes), so that the wide loads are aligned
        uint64_t head = pixels_in_front<SPX>(reinterpret_cast<uintptr_t>(img));
        if (head > npix) head = npix;
        if (tid < head) {
            uint32_t w[1];
            Src::load(img, tid, w, seen);
            note(w[0]);
            insert(w[0]);
        }
        img += SPX * head;
        npix -= head;
    }
    const uint64_t quads = npix / 4;
    for (uint64_t base = 0; base < quads; base += T) {  // (the same trip count in every lane: the shuffle is whole)
        const uint64_t q = base + tid;
        const bool active = q < quads;
        uint32_t v[4] = {0, 0, 0, 0};
        if (active) Src::load(img, 4 * q, v, seen);
        const uint32_t before = (uint32_t)__shfl_up((int)v[3], 1, 64);  // the last pixel of the lane in front
        if (active) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                note(v[j]);
                const bool same = j ? v[j] == v[j - 1] : (lane != 0 && v[0] == before);
                if (!same) insert(v[j]);
            }
        }
    }
    if (tid < npix - 4 * quads) {  // the last one to three pixels
        uint32_t w[1];
        Src::load(img, 4 * quads + tid, w, seen);
        note(w[0]);
        insert(w[0]);
    }
    if constexpr (SPX == 8) {  // alpha and grey on all 16 bits
        all = seen.all, grey = seen.grey;
        if (seen.wide) atomicOr(&sh[kAwWide], seen.wide);
    }
    if (all != 0xFFFFFFFFu) atomicAnd(&sh[kAwAnd], all);
    if (grey) atomicOr(&sh[kAwGrey], grey);
    if (d4) atomicOr(&sh[kAwD4], d4);
    if (d2) atomicOr(&sh[kAwD2], d2);
    if (d1) atomicOr(&sh[kAwD1], d1);
    __syncthreads();
    const uint32_t count = sh[kAwCount];
    const uint32_t wide = SPX == 8 ? sh[kAwWide] : 0u;
    const bool over = count > maxc || wide != 0;
    if (tid == 0) {
        const uint32_t depth = (wide & 0x00FFFFFFu) ? 16u : sh[kAwD4] ? 8u : sh[kAwD2] ? 4u : sh[kAwD1] ? 2u : 1u;
        const bool opaque = SPX == 8 ? (sh[kAwAnd] >> 16) == 0xFFFFu : (sh[kAwAnd] >> 24) == 0xFFu;
        a.summary[i] = (opaque ? 1u : 0u) | (sh[kAwGrey] == 0 ? 2u : 0u) | (SPX == 8 && wide == 0 ? 4u : 0u) | depth << 8;
        a.status[i] = over ? kPngTooManyColours : kPngOk;
    }
    if (over) {  // (not specified; the same words whatever the scheduling was)
        if (tid < 4) a.colour[4 * i + tid] = 0;
        if (tid == 0) a.trns_len[i] = 0;
        if (a.pal)
            for (uint32_t t = tid; t < 256; t += T) a.pal[256 * i + t] = 0xFF000000u;
        return;
    }
    for (uint32_t s = tid; s < kAnalyseSlots; s += T) {
        const uint32_t k = table[s];
        if (k != kEmptyKey) keys[atomicAdd(&sh[kAwKeys], 1u)] = k;  // (count <= max_colours <= 256 keys in all)
    }
    if (tid == 0 && sh[kAwWhite]) keys[atomicAdd(&sh[kAwKeys], 1u)] = kEmptyKey;
    __syncthreads();
    for (uint32_t t = tid; t < 256; t += T) {
        if (t < count) {
            const uint32_t k = keys[t];
            uint32_t rank = 0;
            for (uint32_t u = 0; u < count; u++) rank += keys[u] < k ? 1u : 0u;
            if (a.pal) a.pal[256 * i + rank] = k;
            if (k < 0xFF000000u) atomicAdd(&sh[kAwTrns], 1u);
        } else if (a.pal) {
            a.pal[256 * i + t] = 0xFF000000u;
        }
    }
    __syncthreads();
    if (tid < 4) a.colour[4 * i + tid] = tid == 0 ? count : 0u;
    if (tid == 0) a.trns_len[i] = sh[kAwTrns];
}

// ---- fdh_png_pack_batch ----
constexpr uint32_t kPackBand = 64;  // rows per band, as kExpandBand
constexpr uint32_t kPackSlotBits = 10, kPackSlots = 1u << kPackSlotBits, kNoIndex = 0xFFFFFFFFu;

struct PngPackArgs {
    const uint8_t* rgba;
    const uint64_t* rgba_off;  // n + 1
    uint8_t* pix;
    const uint64_t* pix_off;   // n + 1
    const uint32_t* pal;       // colour type 3: 256 words per image
    const uint32_t* colour;    // nullable: word 0 of 4 is the palette's count
    const uint32_t* upstream;  // nullable
    uint32_t* status;          // zeroed by the launcher
    uint64_t n;
    uint64_t row_bytes;
    uint32_t width;
};

// The palette of one image in the LDS: its words, and slot[h] = the lowest index whose word hashes (and probes) to h.
struct PackLut {
    const uint32_t* pal;
    const uint32_t* slot;
    uint32_t last_word, last_index;
    bool have_last;
    __device__ __forceinline__ uint32_t index(uint32_t w, bool& bad) {
        if (have_last && w == last_word) return last_index;
        uint32_t h = colour_hash(w, kPackSlotBits), found = kNoIndex;
        for (uint32_t p = 0; p < kPackSlots; p++, h = (h + 1) & (kPackSlots - 1)) {
            const uint32_t cur = slot[h];
            if (cur == kNoIndex) break;
            if (pal[cur] == w) {
                found = cur;
                break;
            }
        }
        if (found == kNoIndex) {
            bad = true;
            return 0;
        }
        have_last = true;
        last_word = w;
        last_index = found;
        return found;
    }
};

// N bytes put together in registers and stored with one memcpy (whole words where N allows)
template <int N>
struct PackBytes {
    uint32_t w[(N + 3) / 4];
    __device__ __forceinline__ PackBytes() {
#pragma unroll
        for (int k = 0; k < (N + 3) / 4; k++) w[k] = 0;
    }
    __device__ __forceinline__ void put(int k, uint32_t v) { w[k >> 2] |= v << (8 * (k & 3)); }
    __device__ __forceinline__ void store(uint8_t* p) const { __builtin_memcpy(p, w, N); }  // any alignment
};

template <int DEPTH, int COLOUR, int SPX = 4>
struct Pack {
    using Src = PixelSource<SPX>;
    using Seen = typename Src::Seen;
    static constexpr int CH = (int)png_channels(COLOUR);
    static constexpr int BITS = (int)png_pixel_bits(DEPTH, COLOUR);  // per pixel
    static constexpr int PIXEL = BITS >= 8 ? BITS / 8 : 1;           // bytes of one pixel where it has whole ones
    static constexpr uint32_t MAXV = DEPTH >= 8 ? 255u : (1u << DEPTH) - 1;

    // the sample of depth min(DEPTH, 8) that to8 takes back to v
    static __device__ __forceinline__ uint32_t from8(uint32_t v, bool& bad) {
        if (DEPTH >= 8) return v;
        const uint32_t q = v >> (8 - DEPTH);
        bad = bad || q * (255u / MAXV) != v;
        return q;
    }

    // the CH samples of the pixel word w, each eight bits or fewer
    static __device__ __forceinline__ void samples(uint32_t w, uint32_t (&s)[CH], PackLut& lut, bool& bad) {
        const uint32_t r = w & 0xFFu, g = (w >> 8) & 0xFFu, b = (w >> 16) & 0xFFu, al = w >> 24;
        if (COLOUR == 3) {
            const uint32_t idx = lut.index(w, bad);
            bad = bad || idx > MAXV;
            s[0] = idx & MAXV;
            return;
        }
        if (COLOUR == 0 || COLOUR == 2) bad = bad || al != 255u;
        if (COLOUR == 0 || COLOUR == 4) bad = bad || r != g || g != b;
        s[0] = from8(r, bad);
        if (COLOUR == 4) s[CH - 1] = al;
        if (COLOUR == 2 || COLOUR == 6) {
            s[CH > 1 ? 1 : 0] = g;
            s[CH > 2 ? 2 : 0] = b;
        }
        if (COLOUR == 6) s[CH - 1] = al;
    }

    // pixels of whole bytes: pixel w at byte `at` of o (16-bit samples are the byte twice: s * 257)
    template <int N>
    static __device__ __forceinline__ void emit(PackBytes<N>& o, int at, uint32_t w, PackLut& lut, bool& bad) {
        uint32_t s[CH];
        samples(w, s, lut, bad);
#pragma unroll
        for (int c = 0; c < CH; c++) {
            if (DEPTH == 16) {
                o.put(at + 2 * c, s[c]);
                o.put(at + 2 * c + 1, s[c]);
            } else {
                o.put(at + c, s[c]);
            }
        }
    }

    // pixels x .. x + 3 of the run at `in`: one 16-byte load (two from RGBA16), one store of 4 * PIXEL bytes
    static __device__ __forceinline__ void quad(const uint8_t* in, uint64_t x, uint8_t* out, PackLut& lut, Seen& seen, bool& bad) {
        uint32_t v[4];
        Src::load(in, x, v, seen);
        PackBytes<4 * PIXEL> o;
#pragma unroll
        for (int j = 0; j < 4; j++) emit(o, j * PIXEL, v[j], lut, bad);
        o.store(out + x * PIXEL);
    }

    static __device__ __forceinline__ void one(const uint8_t* in, uint64_t x, uint8_t* out, PackLut& lut, Seen& seen, bool& bad) {
        uint32_t w[1];
        Src::load(in, x, w, seen);
        PackBytes<PIXEL> o;
        emit(o, 0, w[0], lut, bad);
        o.store(out + x * PIXEL);
    }

    // Below eight bits: quad q of the run of npix pixels at `in` (a row, or a band without padding) as 4 * DEPTH bits,
    // most significant first, zeros for pixels behind the run; the bytes go to `out`, the run's first byte.  Every lane
    // of the wavefront comes here together, `active` or not: at depth 1 the odd lane's four bits move to the even lane.
    static __device__ __forceinline__ void narrow(const uint8_t* in, uint64_t npix, uint64_t q, bool active, uint8_t* out, PackLut& lut,
                                                  Seen& seen, bool& bad) {
        uint32_t bits = 0, have = 0;
        if (active) {
            const uint64_t x = 4 * q;
            have = npix - x >= 4 ? 4u : (uint32_t)(npix - x);
            uint32_t v[4] = {0, 0, 0, 0};
            if (have == 4) Src::load(in, x, v, seen);
            else {
#pragma unroll
                for (int j = 0; j < 3; j++) {  // (constant indices: v stays in registers)
                    if ((uint32_t)j < have) {
                        uint32_t w[1];
                        Src::load(in, x + j, w, seen);
                        v[j] = w[0];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if ((uint32_t)j < have) {
                    uint32_t s[CH];
                    samples(v[j], s, lut, bad);
                    bits |= s[0] << (DEPTH * (3 - j));
                }
            }
        }
        if constexpr (DEPTH == 4) {
            if (have >= 3) {
                const uint16_t two = (uint16_t)((bits >> 8) | (bits & 0xFFu) << 8);  // the high byte first
                __builtin_memcpy(out + 2 * q, &two, 2);
            } else if (have) {
                out[2 * q] = (uint8_t)(bits >> 8);
            }
        } else if constexpr (DEPTH == 2) {
            if (have) out[q] = (uint8_t)bits;
        } else {
            const uint32_t odd = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0xB1, 0xF, 0xF, false);  // quad_perm:[1,0,3,2]
            if (have && !(threadIdx.x & 1)) out[q >> 1] = (uint8_t)(bits << 4 | odd);
        }
    }
};

// Image i of the call at a.width and a.row_bytes, behind the caller's look at upstream: the slots' check, the bands
// blockIdx.y, blockIdx.y + gridDim.y, ..  pal (256 words) and slot (kPackSlots words where COLOUR is 3) are the
// workgroup's LDS; only colour type 3 touches them.  SPX = 8 (fdh_png_pack16_mixed_batch, the pairs below depth 16):
// a.rgba holds RGBA16 pictures at even addresses, the picture of the high bytes is packed, and a sample that is not
// narrow is a pixel without a lossless representation.
template <int DEPTH, int COLOUR, int SPX = 4>
__device__ __forceinline__ void png_pack_image(const PngPackArgs& a, uint64_t i, uint32_t lane, uint32_t* pal, uint32_t* slot) {
    using P = Pack<DEPTH, COLOUR, SPX>;
    static_assert(SPX == 4 || DEPTH <= 8, "depth 16 from RGBA16 is png_pack16_image");
    const bool first = blockIdx.y == 0 && lane == 0;
    const uint64_t s0 = a.rgba_off[i], s1 = a.rgba_off[i + 1], o0 = a.pix_off[i], o1 = a.pix_off[i + 1];
    const uint64_t rb = a.row_bytes, width = a.width;
    const uint64_t rows = (s1 - s0) / (width * SPX);
    const bool fits = rows * width * SPX == s1 - s0 && o1 - o0 == rows * rb && (SPX == 4 || (reinterpret_cast<uintptr_t>(a.rgba + s0) & 1) == 0);
    if (!fits) {
        if (first) a.status[i] = kPngBadSizes;
        return;
    }
    const uint64_t bands = (rows + kPackBand - 1) / kPackBand;
    if (blockIdx.y >= bands) return;
    if (COLOUR == 3) {
        uint32_t count = a.colour ? uni(a.colour[4 * i]) : 256u;
        if (count > 256) count = 256;
        for (uint32_t e = lane; e < 256; e += kWave) pal[e] = a.pal[i * 256 + e];
        for (uint32_t s = lane; s < kPackSlots; s += kWave) slot[s] = kNoIndex;
        __syncthreads();
        // a slot belongs to the word that claimed it for good; among equal words the lowest index stays
        for (uint32_t e = lane; e < count; e += kWave) {
            const uint32_t w = pal[e];
            uint32_t h = colour_hash(w, kPackSlotBits);
            for (uint32_t p = 0; p < kPackSlots; p++, h = (h + 1) & (kPackSlots - 1)) {
                uint32_t cur = lds_load(&slot[h]);
                if (cur == kNoIndex) {
                    cur = atomicCAS(&slot[h], kNoIndex, e);
                    if (cur == kNoIndex) break;
                }
                if (pal[cur] == w) {
                    atomicMin(&slot[h], e);
                    break;
                }
            }
        }
        __syncthreads();
    }
    PackLut lut{pal, slot, 0u, 0u, false};
    const uint8_t* const __restrict__ img = a.rgba + s0;
    uint8_t* const __restrict__ dst = a.pix + o0;
    const bool flat = (width * P::BITS & 7) == 0;  // no padding bits: a band is one run of pixels
    bool bad = false;
    typename P::Seen seen;
    for (uint64_t band = blockIdx.y; band < bands; band += gridDim.y) {
        const uint64_t r0 = band * kPackBand, r1 = min(rows, r0 + kPackBand);
        if constexpr (P::BITS >= 8) {  // (always flat)
            const uint8_t* in = img + r0 * width * SPX;
            uint8_t* out = dst + r0 * rb;
            uint64_t npix = (r1 - r0) * width;
            uint64_t head = pixels_in_front<SPX>(reinterpret_cast<uintptr_t>(in));  // alone: the wide loads are aligned
            if (head > npix) head = npix;
            if (lane < head) P::one(in, lane, out, lut, seen, bad);
            in += head * SPX;
            out += head * P::PIXEL;
            npix -= head;
            const uint64_t quads = (npix + 3) / 4;
#pragma unroll 2
            for (uint64_t qx = lane; qx < quads; qx += kWave) {
                if (npix - 4 * qx >= 4) P::quad(in, 4 * qx, out, lut, seen, bad);
                else
                    for (uint64_t p = 4 * qx; p < npix; p++) P::one(in, p, out, lut, seen, bad);
            }
        } else if (flat) {
            const uint8_t* in = img + r0 * width * SPX;
            const uint64_t npix = (r1 - r0) * width, quads = (npix + 3) / 4;
            for (uint64_t base = 0; base < quads; base += kWave)
                P::narrow(in, npix, base + lane, base + lane < quads, dst + r0 * rb, lut, seen, bad);
        } else {
            // rows with padding bits, row by row; at depth 1 a row takes an even number of lanes, so that the two
            // halves of a byte sit in an even lane and the odd one behind it
            const uint64_t qpr = (width + 3) / 4, span = DEPTH == 1 ? (qpr + 1) & ~1ull : qpr;
            if (span >= kWave) {
                for (uint64_t r = r0; r < r1; r++)
                    for (uint64_t base = 0; base < qpr; base += kWave)
                        P::narrow(img + r * width * SPX, width, base + lane, base + lane < qpr, dst + r * rb, lut, seen, bad);
            } else {
                const uint32_t s32 = (uint32_t)span, per = kWave / s32;  // rows per step
                const uint32_t lr = lane / s32, lq = lane - lr * s32;
                for (uint64_t rr = r0; rr < r1; rr += per) {
                    const uint64_t r = rr + lr;
                    const bool active = lr < per && r < r1 && lq < qpr;
                    const uint64_t ra = active ? r : r0;  // (a row that exists: nothing of it is touched)
                    P::narrow(img + ra * width * SPX, width, lq, active, dst + ra * rb, lut, seen, bad);
                }
            }
        }
    }
    if constexpr (SPX == 8) bad = bad || seen.wide != 0;
    if (__any(bad) && lane == 0) atomicOr(&a.status[i], kPngNotRepresentable);
}

}  // namespace fdh
