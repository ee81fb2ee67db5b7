// png_file.hip -- PNG files on the device: CRC-32, the framing around an IDAT stream that is already
// in place, the container scan and the IDAT gather (include/fdeflate_hip.h, "PNG files").
//
// CRC-32 (PNG specification 5.5 / annex D, zlib's crc32): polynomial 0xEDB88320 in the reflected
// bit order, register preset to all ones, result complemented.  gfx950 has no carry-less multiply, so
// the per-byte work is slice-by-4 table look-ups in the LDS; the parallelism inside a range comes from
// the algebra of the register.  Running the table algorithm from register value c over a message M
// leaves   c * x^(8|M|)  +  M(x) * x^32   (mod P, coefficients in GF(2)),   so
//     state(A || B, c) = state(A, c) * x^(8|B|)  +  state(B, 0)
// and zero bytes in FRONT of a message that starts from register 0 change nothing.  A wavefront cuts
// its span into 64 pieces of S bytes aligned to the span's END (the first piece is the short one: it
// costs nothing to think of it as zero-padded in front), every lane runs the table algorithm over its
// piece -- 16-byte loads at 16-byte-aligned addresses --, and six rounds of a tree join neighbours with
// ONE power per round, x^(8 S 2^j), the same for all lanes.  The powers come from the 32 constants
// x^(2^k) mod P, the product is a 32-step shift / xor multiply modulo P (zlib's multmodp).
//
// Nothing here allocates, synchronises or reads anything back.
#include "device_common.h"
#include "launch.h"
#include "png_chunks.h"
#include "png_common.h"

namespace fdh {

constexpr uint32_t kCrcPoly = 0xEDB88320u;

struct CrcTables {
    uint32_t t[4][256];  // slice-by-4: t[0] the classic byte table, t[k][i] = t[0] advanced over k zero bytes
    uint32_t pow2[32];   // x^(2^k) mod P, reflected (x^0 = 0x80000000)
};

constexpr uint32_t crc_mul_const(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? kCrcPoly : 0u);
    }
    return p;
}

constexpr CrcTables make_crc_tables() {
    CrcTables T{};
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? kCrcPoly : 0u);
        T.t[0][i] = c;
    }
    for (int k = 1; k < 4; k++)
        for (uint32_t i = 0; i < 256; i++) T.t[k][i] = (T.t[k - 1][i] >> 8) ^ T.t[0][T.t[k - 1][i] & 0xFF];
    uint32_t p = 0x40000000u;  // x^1
    for (int k = 0; k < 32; k++) {
        T.pow2[k] = p;
        p = crc_mul_const(p, p);
    }
    return T;
}

__device__ const CrcTables kCrc = make_crc_tables();

// a * b mod P (reflected): 32 steps of "add b where a has a coefficient, then b *= x"
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 bytes) mod P.  The order of x divides 2^32 - 1, so the exponent is reduced to 32 bits first.  `bytes` is the
// same in every lane of the wavefront: the branches are scalar.
__device__ __forceinline__ uint32_t crc_xpow8(uint64_t bytes) {
    uint64_t e = (bytes & 0x1FFFFFFFull) * 8 + (bytes >> 29);  // 8 * bytes = (bytes >> 29) * 2^32 + low part
    e = (e & 0xFFFFFFFFull) + (e >> 32);
    e = (e & 0xFFFFFFFFull) + (e >> 32);
    uint32_t n = uni((uint32_t)e);
    uint32_t p = 0x80000000u;
    for (int k = 0; n; k++, n >>= 1)
        if (n & 1) p = crc_mul(p, kCrc.pow2[k]);
    return p;
}

// The look-up tables in the LDS, COPIES times: entry (table k, byte v) of copy c at dword (k * 256 + v) * COPIES + c, and a
// lane reads copy lane % COPIES.  One copy (4 KiB) leaves the 32 lanes of a ds_read_b32 group to collide on 32 banks at
// random; 32 copies (128 KiB) give every lane a bank of its own.
template <int COPIES>
struct CrcLds {
    uint32_t t[1024 * COPIES];
    __device__ __forceinline__ void load(int tid, int nthreads) {
        const uint32_t* src = &kCrc.t[0][0];
        for (int i = tid; i < 1024 * COPIES; i += nthreads) t[i] = src[i / COPIES];
        __syncthreads();
    }
};

template <int COPIES>
struct CrcLane {
    const uint32_t* t;  // the lane's copy: &lds.t[lane % COPIES]
    __device__ __forceinline__ uint32_t at(uint32_t k, uint32_t v) const { return t[(k * 256 + v) * COPIES]; }
    __device__ __forceinline__ uint32_t byte(uint32_t c, uint32_t v) const { return (c >> 8) ^ at(0, (c ^ v) & 0xFF); }
    __device__ __forceinline__ uint32_t word(uint32_t c, uint32_t w) const {
        c ^= w;
        return at(3, c & 0xFF) ^ at(2, (c >> 8) & 0xFF) ^ at(1, (c >> 16) & 0xFF) ^ at(0, c >> 24);
    }
};

// The register after the table algorithm has run from `init` over [b, e), computed by the 64 lanes of a wavefront together
// (b, e, init the same in every lane; every lane returns the same value).  Only bytes of [b, e) are read.
template <int COPIES>
__device__ __forceinline__ uint32_t wave_crc(const CrcLane<COPIES>& T, int lane, const uint8_t* b, const uint8_t* e,
                                             uint32_t init) {
    const uintptr_t ub = reinterpret_cast<uintptr_t>(b), ue = reinterpret_cast<uintptr_t>(e);
    const uintptr_t e0 = ue & ~(uintptr_t)15;  // the last 0..15 bytes are taken one by one behind the tree
    uint32_t cw = init;
    uintptr_t tail = ub;
    if (e0 > ub) {
        const uint64_t span = e0 - ub;
        const uint64_t S = ((span + 63) / 64 + 15) & ~15ull;  // piece size: a multiple of 16, at most 64 pieces
        // pieces that hold bytes: those of lanes 64 - m .. 63 (a span is shorter than 2^36: in units of 16 bytes 32 bits do)
        const uint32_t m = ((uint32_t)((span + 15) >> 4) + (uint32_t)(S >> 4) - 1) / (uint32_t)(S >> 4);
        const uint32_t r = 63u - (uint32_t)lane;              // piece r ends r * S bytes in front of e0
        uint32_t c = 0;
        if (r < m) {
            const uintptr_t hi = e0 - r * S;
            uintptr_t p = hi - S;
            if (r == m - 1) {  // the first piece starts where the span does, with the caller's register
                p = ub;
                c = init;
                for (; p & 15; p++) c = T.byte(c, *reinterpret_cast<const uint8_t*>(p));  // (hi is aligned: p stops there at the latest)
            }
            for (; p < hi; p += 16) {
                const uint4 v = *reinterpret_cast<const uint4*>(p);
                c = T.word(c, v.x);
                c = T.word(c, v.y);
                c = T.word(c, v.z);
                c = T.word(c, v.w);
            }
        }
        // lanes without a piece hold 0 = the register of an empty message: they join like any other
        uint32_t pw = crc_xpow8(S);
        for (uint32_t d = 1; d < m; d <<= 1) {
            const uint32_t left = (uint32_t)__shfl((int)c, (lane - (int)d) & 63, 64);  // piece r + d: the bytes in front
            const uint32_t joined = crc_mul(left, pw) ^ c;
            if ((r & (2 * d - 1)) == 0) c = joined;
            if (2 * d < m) pw = crc_mul(pw, pw);
        }
        cw = (uint32_t)__shfl((int)c, 63, 64);
        tail = e0;
    }
    for (; tail < ue; tail++) cw = T.byte(cw, *reinterpret_cast<const uint8_t*>(tail));
    return cw;
}

// What piece `w` of `pieces` contributes to the CRC-32 of [b, e) continued from `seed`: the contributions of all pieces
// xor to the CRC.  Pieces are cut at 16-byte-aligned addresses; piece 0 carries the preset and the final complement.
template <int COPIES>
__device__ __forceinline__ uint32_t crc_piece(const CrcLane<COPIES>& T, int lane, const uint8_t* b, const uint8_t* e,
                                              uint32_t seed, uint32_t w, uint32_t pieces) {
    const uint8_t* wb = b;
    const uint8_t* we = e;
    if (pieces > 1) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(b) & ~(uintptr_t)15;
        const uint64_t total = reinterpret_cast<uintptr_t>(e) - a0;
        const uint64_t per = ((total + pieces - 1) / pieces + 15) & ~15ull;
        const uint64_t lo = (uint64_t)w * per, hi = lo + per;
        wb = lo >= total ? e : (w == 0 ? b : reinterpret_cast<const uint8_t*>(a0 + lo));
        we = hi >= total ? e : reinterpret_cast<const uint8_t*>(a0 + hi);
    }
    if (w != 0 && wb >= we) return 0;
    uint32_t c = wave_crc<COPIES>(T, lane, wb, we, w == 0 ? ~seed : 0u);
    if (we < e) c = crc_mul(c, crc_xpow8((uint64_t)(e - we)));
    return w == 0 ? ~c : c;
}

// ---- fdh_crc32_batch, and the IDAT checksum of fdh_png_frame_batch ----
struct CrcArgs {
    const uint8_t* data;
    const uint64_t* off;
    const uint32_t* len;   // nullable
    const uint32_t* seed;  // nullable
    uint32_t* crc;
    uint32_t* status;
    uint64_t n;
    uint32_t pieces;  // wavefronts per range; above 1 they xor into crc[i], which the host has zeroed
    // frame mode (png_status != nullptr): range i is "IDAT" + the stream of file i, prefix - 4 bytes into its slot, and the
    // sum goes to the aligned word inside the 16 bytes behind the stream (png_frame_finish_kernel picks it up there)
    const uint32_t* png_status;
    uint32_t prefix;
    // fdh_png_frame_mixed_batch (info != nullptr): the prefix is each file's own, frame_prefix
    const PngInfo* info;
    const uint32_t* colour;
    const uint32_t* trns_len;
};

constexpr uint32_t kPngPrefix = kPngFilePrefix, kPngSuffix = kPngFileSuffix;

// The bytes in front of file i's stream: the call's, or in a mixed batch (info != nullptr) what follows from the file's
// record and palette (png_encode_prefix).  Asked only for files the prefix kernel has accepted: the arrays are there
// where the colour type is 3.  The prefix kernel, the IDAT's CRC pass and the finishing kernel all ask here.
__device__ __forceinline__ uint32_t frame_prefix(const PngInfo* info, const uint32_t* colour, const uint32_t* trns_len, uint64_t i,
                                                 uint32_t call_prefix) {
    if (!info) return call_prefix;
    const bool palette = info[i].colour_type == 3;
    return png_encode_prefix(info[i].colour_type, palette ? colour[4 * i] : 0u, palette ? trns_len[i] : 0u);
}

__device__ __forceinline__ uint32_t* frame_sum_word(uint8_t* stream_end) {
    return reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(stream_end) + 3) & ~(uintptr_t)3);
}

template <int COPIES, int THREADS>
__global__ __launch_bounds__(THREADS) void crc32_ranges_kernel(CrcArgs a) {
    __shared__ CrcLds<COPIES> lds;
    lds.load((int)threadIdx.x, THREADS);
    const int lane = (int)threadIdx.x & 63;
    // (everything about the wavefront's range is the same in all its lanes: kept in scalar registers)
    const uint32_t g = blockIdx.x * (THREADS / 64) + uni(threadIdx.x >> 6);  // n * pieces < 2^32 (launch_crc)
    const uint32_t i = a.pieces == 1 ? g : g / a.pieces;
    const uint32_t w = a.pieces == 1 ? 0u : g % a.pieces;
    if (i >= a.n) return;
    CrcLane<COPIES> T{&lds.t[lane % COPIES]};
    const uint64_t o = a.off[i], slot = a.off[i + 1] - o;
    if (a.png_status) {
        if (a.png_status[i] != kPngOk) return;
        const uint32_t s = a.len[i];
        const uint8_t* b = a.data + o + (frame_prefix(a.info, a.colour, a.trns_len, i, a.prefix) - 4);
        const uint32_t c = crc_piece<COPIES>(T, lane, b, b + 4 + s, 0u, w, a.pieces);
        uint32_t* sum = frame_sum_word(const_cast<uint8_t*>(b) + 4 + s);
        if (lane == 0) {
            if (a.pieces == 1) *sum = c;
            else if (c) atomicXor(sum, c);
        }
        return;
    }
    const uint32_t L = a.len ? a.len[i] : (uint32_t)slot;
    const bool bad = (slot >> 32) != 0 || (a.len && (L == 0xFFFFFFFFu || L > slot));
    if (bad) {
        if (lane == 0 && w == 0) {
            a.crc[i] = 0;
            a.status[i] = kPngBadSizes;
        }
        return;
    }
    const uint8_t* b = a.data + o;
    const uint32_t c = crc_piece<COPIES>(T, lane, b, b + L, a.seed ? a.seed[i] : 0u, w, a.pieces);
    if (lane == 0) {
        if (w == 0) a.status[i] = kPngOk;
        if (a.pieces == 1) a.crc[i] = c;
        else if (c) atomicXor(&a.crc[i], c);
    }
}

// ---- fdh_png_frame_batch: the 41 bytes in front of the stream, the 16 behind it ----
struct FrameArgs {
    uint8_t* file;
    const uint64_t* file_off;
    const uint32_t* idat_len;
    const uint32_t* height;
    uint32_t* file_len;
    uint32_t* png_status;
    uint64_t n;
    uint32_t width, bit_depth, colour_type;
    uint32_t prefix;  // bytes in front of the stream: kPngPrefix, more with PLTE and tRNS
    // fdh_png_frame_palette_batch only
    const uint32_t* pal;
    const uint32_t* colour;
    const uint32_t* trns_len;
    uint32_t plte_entries, trns_entries;
    // fdh_png_frame_mixed_batch only: width, bit_depth, colour_type and prefix are each file's own
    const PngInfo* info;
};

__device__ __forceinline__ uint32_t crc_bitwise(uint32_t c, uint32_t v) {
    c ^= v;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    return c;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}


// what both framing calls refuse: (0xFFFFFFFF, the encoders' "slot too small", is above 2^31 - 1)
__device__ __forceinline__ bool frame_sizes_bad(uint32_t s, uint32_t h, uint64_t slot, uint32_t prefix) {
    return s == 0 || s > 0x7FFFFFFFu || (uint64_t)s + prefix + kPngSuffix > slot || h == 0 || h > 0x7FFFFFFFu;
}

// the first 33 bytes of a file: signature and IHDR (its CRC is 17 bytes of bit-at-a-time arithmetic)
__device__ __forceinline__ void put_signature_ihdr(uint8_t* f, const FrameArgs& a, uint32_t h) {
    const uint8_t head[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    for (int k = 0; k < 16; k++) f[k] = head[k];
    put_be32(f + 16, a.width);
    put_be32(f + 20, h);
    f[24] = (uint8_t)a.bit_depth;
    f[25] = (uint8_t)a.colour_type;
    f[26] = f[27] = f[28] = 0;
    uint32_t c = 0xFFFFFFFFu;
    c = crc_bitwise(c, 'I');
    c = crc_bitwise(c, 'H');
    c = crc_bitwise(c, 'D');
    c = crc_bitwise(c, 'R');
    for (int k = 3; k >= 0; k--) c = crc_bitwise(c, (a.width >> (8 * k)) & 0xFF);
    for (int k = 3; k >= 0; k--) c = crc_bitwise(c, (h >> (8 * k)) & 0xFF);
    c = crc_bitwise(c, a.bit_depth);
    c = crc_bitwise(c, a.colour_type);
    for (int k = 0; k < 3; k++) c = crc_bitwise(c, 0);
    put_be32(f + 29, ~c);
}

// a chunk's length and type
__device__ __forceinline__ void put_chunk_head(uint8_t* p, uint32_t len, char t0, char t1, char t2, char t3) {
    put_be32(p, len);
    p[4] = (uint8_t)t0;
    p[5] = (uint8_t)t1;
    p[6] = (uint8_t)t2;
    p[7] = (uint8_t)t3;
}

// One file per lane: the checks, the prefix, a zero in the word that will collect the IDAT checksum.
__global__ __launch_bounds__(256) void png_frame_prefix_kernel(FrameArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o = a.file_off[i], slot = a.file_off[i + 1] - o;
    const uint32_t s = a.idat_len[i], h = a.height[i];
    if (frame_sizes_bad(s, h, slot, kPngPrefix)) {
        a.png_status[i] = kPngBadSizes;
        a.file_len[i] = 0;
        return;
    }
    uint8_t* f = a.file + o;
    put_signature_ihdr(f, a, h);
    put_chunk_head(f + 33, s, 'I', 'D', 'A', 'T');
    *frame_sum_word(f + kPngPrefix + s) = 0;
    a.file_len[i] = s + kPngPrefix + kPngSuffix;
    a.png_status[i] = kPngOk;
}

// What stands in front of the stream of file i, written by one wavefront: signature and IHDR (a.width, a.bit_depth,
// a.colour_type), with `palette` a PLTE of E entries -- the image's `count`, then 0, 0, 0 -- and where T > 0 a tRNS of T
// alphas (then 255), the IDAT's head; a zero in the word that will collect the IDAT checksum, the file's length and status.
__device__ __forceinline__ void frame_write_prefix(const FrameArgs& a, uint64_t i, int lane, CrcLane<1>& C, uint32_t s, uint32_t h,
                                                   uint32_t count, uint32_t E, uint32_t T, uint32_t prefix, bool palette) {
    uint8_t* f = a.file + a.file_off[i];
    uint8_t* next = f + 33;
    if (lane == 0) put_signature_ihdr(f, a, h);
    if (palette) {
        const uint32_t* pal = a.pal + 256 * i;
        uint8_t* plte = next;
        if (lane == 0) put_chunk_head(plte, 3 * E, 'P', 'L', 'T', 'E');
        for (uint32_t e = (uint32_t)lane; e < E; e += 64) {
            const uint32_t w = e < count ? pal[e] : 0u;
            plte[8 + 3 * e] = (uint8_t)w;
            plte[9 + 3 * e] = (uint8_t)(w >> 8);
            plte[10 + 3 * e] = (uint8_t)(w >> 16);
        }
        next = plte + 12 + 3 * E;
        if (T) {
            if (lane == 0) put_chunk_head(next, T, 't', 'R', 'N', 'S');
            for (uint32_t e = (uint32_t)lane; e < T; e += 64) next[8 + e] = e < count ? (uint8_t)(pal[e] >> 24) : (uint8_t)255;
        }
        // the wavefront reads back what its lanes wrote: the stores are complete before the loads are issued
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t c_plte = ~wave_crc<1>(C, lane, plte + 4, plte + 8 + 3 * E, 0xFFFFFFFFu);
        if (lane == 0) put_be32(plte + 8 + 3 * E, c_plte);
        if (T) {
            const uint32_t c_trns = ~wave_crc<1>(C, lane, next + 4, next + 8 + T, 0xFFFFFFFFu);
            if (lane == 0) put_be32(next + 8 + T, c_trns);
            next += 12 + T;
        }
    }
    if (lane == 0) {
        put_chunk_head(next, s, 'I', 'D', 'A', 'T');
        *frame_sum_word(f + prefix + s) = 0;
        a.file_len[i] = s + prefix + kPngSuffix;
        a.png_status[i] = kPngOk;
    }
}

// fdh_png_frame_palette_batch: one file per wavefront, four to a workgroup that shares the CRC tables.  Lane 0 writes
// signature, IHDR and the chunk heads; the lanes together write the PLTE's E entries (the image's own, then 0, 0, 0) and
// the tRNS's T alphas (then 255), and the CRC of each chunk is wave_crc over the bytes just written.
__global__ __launch_bounds__(256) void png_frame_palette_prefix_kernel(FrameArgs a) {
    __shared__ CrcLds<1> lds;
    lds.load((int)threadIdx.x, 256);
    const int lane = (int)threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + uni(threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint64_t o = a.file_off[i], slot = a.file_off[i + 1] - o;
    const uint32_t s = uni(a.idat_len[i]), h = uni(a.height[i]);
    const uint32_t count = uni(a.colour[4 * i]), alphas = uni(a.trns_len[i]);
    const uint32_t E = a.plte_entries, T = a.trns_entries;
    const uint32_t st = frame_sizes_bad(s, h, slot, a.prefix) ? kPngBadSizes : (count == 0 || count > E) ? kPngBadPlte : alphas > T ? kPngBadTrns : kPngOk;
    if (st != kPngOk) {
        if (lane == 0) {
            a.png_status[i] = st;
            a.file_len[i] = 0;
        }
        return;
    }
    CrcLane<1> C{lds.t};
    frame_write_prefix(a, i, lane, C, s, h, count, E, T, a.prefix, true);
}

// fdh_png_frame_mixed_batch: the same wavefront per file with width, pair and palette sizes of the file's own: E is the
// image's count and T its trns_len, so no entry is padding.
__global__ __launch_bounds__(256) void png_frame_mixed_prefix_kernel(FrameArgs a) {
    __shared__ CrcLds<1> lds;
    lds.load((int)threadIdx.x, 256);
    const int lane = (int)threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + uni(threadIdx.x >> 6);
    if (i >= a.n) return;
    const PngInfo r = mixed_record(a.info, i);
    const uint64_t slot = a.file_off[i + 1] - a.file_off[i];
    const uint32_t s = uni(a.idat_len[i]);
    uint32_t st = kPngOk, count = 0, alphas = 0;
    if (!mixed_encodable(r)) st = kPngSkipped;
    else {
        const bool palette = r.colour_type == 3;
        bool bad_plte = false, bad_trns = false;
        if (palette) {
            const bool have = a.pal && a.colour && a.trns_len;
            count = have ? uni(a.colour[4 * i]) : 0u;
            alphas = have ? uni(a.trns_len[i]) : 0u;
            bad_plte = count == 0 || count > (1u << r.bit_depth);
            bad_trns = !bad_plte && alphas > count;
            if (bad_plte) count = 1;  // (the sizes are checked with the smallest prefix a palette file can have)
            if (bad_plte || bad_trns) alphas = 0;
        }
        st = frame_sizes_bad(s, r.height, slot, png_encode_prefix(r.colour_type, count, alphas)) ? kPngBadSizes
             : bad_plte ? kPngBadPlte : bad_trns ? kPngBadTrns : kPngOk;
    }
    if (st != kPngOk) {
        if (lane == 0) {
            a.png_status[i] = st;
            a.file_len[i] = 0;
        }
        return;
    }
    CrcLane<1> C{lds.t};
    FrameArgs g = a;
    g.width = r.width, g.bit_depth = r.bit_depth, g.colour_type = r.colour_type;
    frame_write_prefix(g, i, lane, C, s, r.height, count, count, alphas, png_encode_prefix(r.colour_type, count, alphas), r.colour_type == 3);
}

// One file per lane: the IDAT's CRC from the word it was summed in, then IEND.
__global__ __launch_bounds__(256) void png_frame_finish_kernel(FrameArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n || a.png_status[i] != kPngOk) return;
    uint8_t* t = a.file + a.file_off[i] + frame_prefix(a.info, a.colour, a.trns_len, i, a.prefix) + a.idat_len[i];
    const uint32_t c = *frame_sum_word(t);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    put_be32(t, c);
    for (int k = 0; k < 12; k++) t[4 + k] = iend[k];
}

// ---- fdh_png_scan_files_batch ----

struct ScanArgs {
    const uint8_t* file;
    const uint64_t* file_off;
    const uint32_t* file_len;  // nullable
    PngInfo* info;
    uint64_t n;
    bool adam7;  // FDH_PNG_FLAG_ADAM7: interlace method 1 is no finding
};


// One file per lane: the chain of chunk headers (dependent loads, a handful per file).  The first finding in file order
// is the file's status; the walk ends there, and the counts hold what came before it.
__global__ __launch_bounds__(64) void png_scan_kernel(ScanArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o = a.file_off[i], slot = a.file_off[i + 1] - o;
    const uint64_t flen = a.file_len ? (a.file_len[i] < slot ? a.file_len[i] : slot) : slot;
    const uint8_t* f = a.file + o;
    PngInfo r{};
    uint32_t st = kPngOk;
    if (flen < 8 || get_be32(f) != 0x89504E47u || get_be32(f + 4) != 0x0D0A1A0Au) st = kPngScanNoSignature;
    uint64_t pos = 8, idat = 0;
    bool seen_idat = false, idat_over = false;
    while (st == kPngOk) {
        if (pos + 12 > flen) {
            st = kPngScanTruncated;
            break;
        }
        const uint32_t len = get_be32(f + pos), type = get_be32(f + pos + 4);
        if (r.chunks == 0 && (type != kIHDR || len != 13)) {
            st = kPngScanBadIhdr;
            break;
        }
        if (pos + 12 + len > flen) {
            st = kPngScanTruncated;
            break;
        }
        if (r.chunks == 0) {
            const uint8_t* d = f + pos + 8;
            r.width = get_be32(d);
            r.height = get_be32(d + 4);
            r.bit_depth = d[8];
            r.colour_type = d[9];
            r.interlace = d[12];
            if (r.width == 0 || r.height == 0 || (r.width | r.height) >> 31 || !png_pair_ok(d[8], d[9]) || d[10] != 0 ||
                d[11] != 0 || d[12] > 1)
                st = kPngScanBadIhdr;
            else if (d[12] == 1 && !a.adam7)
                st = kPngScanInterlaced;
        } else if (type == kIDAT) {
            if (idat_over) st = kPngScanChunkStructure;
            else {
                if (!seen_idat) r.first_idat = (uint32_t)pos;
                seen_idat = true;
                idat += len;
                r.idat_chunks++;
                if (idat >> 32 || pos >> 32) st = kPngScanChunkStructure;  // (the counts are 32 bits wide)
            }
        } else {
            if (seen_idat) idat_over = true;
            if (type == kIEND) {
                if (!seen_idat) st = kPngScanChunkStructure;
            } else if (type == kPLTE) {
                if (seen_idat) st = kPngScanChunkStructure;
            } else if (!(type & 0x20000000u)) {  // an upper-case first letter: critical, and none that is known here
                st = kPngScanChunkStructure;
            }
        }
        if (st) break;
        r.chunks++;
        pos += 12ull + len;
        if (type == kIEND) break;
    }
    r.idat_bytes = (uint32_t)idat;
    r.status = st;
    a.info[i] = r;
}

// One file per workgroup, the chunks in file order, every chunk by all wavefronts of the group together: each takes a
// piece (crc_piece), the pieces meet in the LDS.  Only files the walk found sound are read; a mismatch: kPngScanCrcMismatch.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void png_verify_crc_kernel(ScanArgs a) {
    __shared__ CrcLds<1> lds;
    __shared__ uint32_t part[THREADS / 64];
    lds.load((int)threadIdx.x, THREADS);
    const uint64_t i = blockIdx.x;
    if (a.info[i].status != kPngOk) return;
    const int lane = (int)threadIdx.x & 63;
    const uint32_t w = uni(threadIdx.x >> 6);
    CrcLane<1> T{lds.t};
    const uint8_t* f = a.file + a.file_off[i];
    const uint32_t chunks = uni(a.info[i].chunks);
    uint64_t pos = 8;
    bool differs = false;
    for (uint32_t k = 0; k < chunks; k++) {
        const uint32_t len = uni(get_be32(f + pos));
        const uint8_t* b = f + pos + 4;
        const uint8_t* e = b + 4 + len;
        uint32_t c = crc_piece<1>(T, lane, b, e, 0u, w, THREADS / 64);
        if (THREADS > 64) {
            if (lane == 0) part[w] = c;
            __syncthreads();
            c = 0;
            for (int j = 0; j < THREADS / 64; j++) c ^= part[j];
            __syncthreads();
        }
        differs = differs || c != get_be32(e);
        pos += 12ull + len;
    }
    if (differs && threadIdx.x == 0) a.info[i].status = kPngScanCrcMismatch;
}

// ---- fdh_png_gather_idat_batch, fdh_png_colour_batch: the bodies are in png_chunks.h ----
template <int THREADS>
__global__ __launch_bounds__(THREADS) void png_gather_idat_kernel(GatherArgs a) {
    const uint64_t i = blockIdx.x;
    const PngInfo r = a.info[i];
    const uint64_t room = a.comp_off[i + 1] - a.comp_off[i];
    uint32_t st = kPngOk;
    if (r.status != kPngOk) st = kPngSkipped;
    else if (r.width != a.width || r.bit_depth != a.bit_depth || r.colour_type != a.colour_type) st = kPngOtherGeometry;
    else if (r.idat_bytes > room) st = kPngCompSlotTooSmall;
    png_gather_file<THREADS>(a, i, r, st);
}

__global__ __launch_bounds__(kWave) void png_colour_kernel(ColourArgs a) {
    const uint64_t i = blockIdx.x;
    const PngInfo r = a.info[i];
    const uint32_t ct = a.colour_type;
    uint32_t st = kPngOk;
    if (r.status != kPngOk) st = kPngSkipped;
    else if (r.width != a.width || r.bit_depth != a.bit_depth || r.colour_type != ct) st = kPngOtherGeometry;
    png_colour_file(a, i, threadIdx.x, r, ct, st);
}

}  // namespace fdh

// ---- launchers ----
namespace {

using fdh::kFillWaves;  // (launch.h)

hipError_t launch_crc(fdh::CrcArgs a, hipStream_t stream) {
    a.pieces = a.n >= kFillWaves ? 1u : (uint32_t)((kFillWaves + a.n - 1) / a.n);
    const int forced = fdh::env_int("FDH_CRC_PIECES", 0);  // tests / A-B
    if (forced >= 1 && forced <= 65536 && a.n * (uint64_t)forced < (1ull << 31)) a.pieces = (uint32_t)forced;
    if (a.pieces > 1 && !a.png_status) {
        hipError_t e = hipMemsetAsync(a.crc, 0, a.n * 4, stream);
        if (e != hipSuccess) return e;
    }
    const uint64_t waves = a.n * a.pieces;
    const int copies = fdh::env_int("FDH_CRC_COPIES", 1);  // tests / A-B: 1, 8 or 32 copies of the tables (measured)
    if (copies == 32) {
        hipLaunchKernelGGL((fdh::crc32_ranges_kernel<32, 1024>), dim3((unsigned)((waves + 15) / 16)), dim3(1024), 0, stream, a);
    } else if (copies == 8) {
        hipLaunchKernelGGL((fdh::crc32_ranges_kernel<8, 256>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL((fdh::crc32_ranges_kernel<1, 256>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

// what follows a framing call's prefix kernel: the IDAT's checksum into its word, then the 16 bytes behind the stream
hipError_t launch_frame_tail(const fdh::FrameArgs& a, hipStream_t stream) {
    fdh::CrcArgs c{a.file, a.file_off, a.idat_len, nullptr, nullptr, nullptr, a.n, 1, a.png_status, a.prefix, a.info, a.colour, a.trns_len};
    hipError_t e = launch_crc(c, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fdh::png_frame_finish_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int fdh_launch_crc32(const uint8_t* data, const uint64_t* off, const uint32_t* len, const uint32_t* seed,
                                uint32_t* crc, uint32_t* status, uint64_t n, hipStream_t stream) {
    fdh::CrcArgs a{data, off, len, seed, crc, status, n, 1, nullptr, 0};
    return (int)launch_crc(a, stream);
}

extern "C" int fdh_launch_png_frame(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height,
                                    uint32_t* file_len, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth,
                                    uint32_t colour_type, hipStream_t stream) {
    fdh::FrameArgs a{file, file_off, idat_len, height, file_len, png_status, n, width, bit_depth, colour_type, fdh::kPngPrefix,
                     nullptr, nullptr, nullptr, 0, 0};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(fdh::png_frame_prefix_kernel, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)launch_frame_tail(a, stream);
}

// The same three steps with a longer prefix: signature, IHDR, PLTE, tRNS and the IDAT's head in front of the stream.
extern "C" int fdh_launch_png_frame_palette(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const uint32_t* height,
                                            const uint32_t* pal, const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len,
                                            uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth, uint32_t plte_entries,
                                            uint32_t trns_entries, hipStream_t stream) {
    const uint32_t prefix = fdh::kPngPrefix + 12 + 3 * plte_entries + (trns_entries ? 12 + trns_entries : 0);
    fdh::FrameArgs a{file, file_off, idat_len, height, file_len, png_status, n, width, bit_depth, 3, prefix,
                     pal, colour, trns_len, plte_entries, trns_entries};
    hipLaunchKernelGGL(fdh::png_frame_palette_prefix_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)launch_frame_tail(a, stream);
}

// ... and with every file's own: the geometry from info[i], a PLTE / tRNS of exactly the image's entries.
extern "C" int fdh_launch_png_frame_mixed(uint8_t* file, const uint64_t* file_off, const uint32_t* idat_len, const fdh_png_info* info,
                                          const uint32_t* pal, const uint32_t* colour, const uint32_t* trns_len, uint32_t* file_len,
                                          uint32_t* png_status, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    fdh::FrameArgs a{file, file_off, idat_len, nullptr, file_len, png_status, n, 0, 0, 0, 0, pal, colour, trns_len, 0, 0, info};
    hipLaunchKernelGGL(fdh::png_frame_mixed_prefix_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)launch_frame_tail(a, stream);
}

extern "C" int fdh_launch_png_scan(const uint8_t* file, const uint64_t* file_off, const uint32_t* file_len, fdh_png_info* info,
                                   uint64_t n, int verify_crc, int adam7, hipStream_t stream) {
    fdh::ScanArgs a{file, file_off, file_len, info, n, adam7 != 0};
    hipLaunchKernelGGL(fdh::png_scan_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !verify_crc) return (int)e;
    if (n >= kFillWaves) hipLaunchKernelGGL((fdh::png_verify_crc_kernel<64>), dim3((unsigned)n), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((fdh::png_verify_crc_kernel<1024>), dim3((unsigned)n), dim3(1024), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_colour(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint32_t* pal,
                                     uint32_t* colour, uint32_t* png_status, uint64_t n, uint32_t width, uint32_t bit_depth,
                                     uint32_t colour_type, hipStream_t stream) {
    fdh::ColourArgs a{file, file_off, info, pal, colour, png_status, n, width, bit_depth, colour_type};
    hipLaunchKernelGGL(fdh::png_colour_kernel, dim3((unsigned)n), dim3(fdh::kWave), 0, stream, a);
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_gather(const uint8_t* file, const uint64_t* file_off, const fdh_png_info* info, uint8_t* comp,
                                     const uint64_t* comp_off, uint32_t* comp_len, uint32_t* png_status, uint64_t n,
                                     uint32_t width, uint32_t bit_depth, uint32_t colour_type, hipStream_t stream) {
    fdh::GatherArgs a{file, file_off, info, comp, comp_off, comp_len, png_status, n,
                      width, bit_depth, colour_type};
    if (n >= kFillWaves) hipLaunchKernelGGL((fdh::png_gather_idat_kernel<64>), dim3((unsigned)n), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((fdh::png_gather_idat_kernel<256>), dim3((unsigned)n), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}
