// deflate_stitch.hip -- joins raw-deflate pieces into zlib streams (include/fdeflate_hip_pieces.h).
//
// The pieces of an input -- written by the block writer of deflate_general.hip in piece mode, each byte-aligned, the
// non-last ones closed by the sync marker of Flush::Sync (reference src/compress/mod.rs:284-287) -- are laid end to
// end behind 78 01 and in front of the Adler-32 of the whole input.  Two kernels on the caller's stream:
//   stitch_plan_kernel   one wavefront per input: the pieces' places by an exclusive scan of their lengths, the
//                        input's checksum from the pieces' by a wave reduction, header and trailer
//   stitch_copy_kernel   one workgroup per piece at a time: the bytes, to a place of any alignment
// The plan hands every piece's place to the copy in piece_adler, which it has consumed by then, so the pair needs no
// workspace and no number from the device: the copy's grid is fixed and strides over the pieces.
// Traffic per stitched byte: one read (the piece's slot) and one write (its place); per piece 24 bytes of metadata.
#include "bit_ring.h"
#include "device_common.h"
#include "launch.h"

namespace fdh {

constexpr uint32_t kStitchFailed = 0xFFFFFFFFu;
constexpr int kCopyThreads = 256;

struct StitchArgs {
    const uint8_t* pieces;
    const uint64_t* piece_slot_off;
    const uint32_t* piece_len;
    uint32_t* piece_adler;  // in: the pieces' checksums; out: their byte positions in their streams, or kStitchFailed
    const uint64_t* piece_off;
    const uint64_t* first_piece;
    uint8_t* out;
    const uint64_t* out_off;
    uint32_t* out_len;
    uint64_t n;
};

// An Adler-32 as an element of the monoid the combine rule defines: the sums (a, b) of a run of bytes and the run's
// length mod 65521.  x . y is the checksum of x's bytes followed by y's; (1, 0, 0) is the empty run.
struct AdlerRun {
    uint32_t a, b, n;
};
__device__ __forceinline__ AdlerRun adler_join(const AdlerRun& x, const AdlerRun& y) {
    const uint64_t a1m1 = (x.a + kAdlerMod - 1) % kAdlerMod;  // A1 - 1
    AdlerRun r;
    r.a = (uint32_t)(((uint64_t)x.a + y.a + kAdlerMod - 1) % kAdlerMod);
    r.b = (uint32_t)(((uint64_t)x.b + y.b + (uint64_t)y.n * a1m1) % kAdlerMod);
    r.n = (x.n + y.n) % kAdlerMod;
    return r;
}

__global__ __launch_bounds__(kWave) void stitch_plan_kernel(StitchArgs s) {
    const uint32_t lane = threadIdx.x;
    const uint64_t i = blockIdx.x;
    const uint64_t p0 = s.first_piece[i], p1 = s.first_piece[i + 1];
    const uint64_t slot = s.out_off[i + 1] - s.out_off[i];
    // the total, and whether every piece is there
    uint64_t sum = 0;
    bool bad = p1 <= p0;
    for (uint64_t k = p0 + lane; k < p1; k += kWave) {
        const uint32_t l = s.piece_len[k];
        bad |= l == kStitchFailed || l > s.piece_slot_off[k + 1] - s.piece_slot_off[k];  // (never read past a piece's slot)
        sum += l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
    const uint64_t total = 2 + sum + 4;
    if (__any(bad) || total > slot || total > 0xFFFFFFFEull) {
        for (uint64_t k = p0 + lane; k < p1; k += kWave) s.piece_adler[k] = kStitchFailed;
        if (lane == 0) s.out_len[i] = kStitchFailed;
        return;
    }
    // 64 pieces per round: their places behind `at`, their checksums joined in order onto `whole`
    uint32_t at = 2;
    AdlerRun whole{1, 0, 0};
    for (uint64_t k0 = p0; k0 < p1; k0 += kWave) {  // (uniform: every lane takes part in the scan and the shuffles)
        const uint64_t k = k0 + lane;
        const bool live = k < p1;
        const uint32_t l = live ? s.piece_len[k] : 0u;
        AdlerRun r{1, 0, 0};
        if (live) {
            const uint32_t ad = s.piece_adler[k];
            r = AdlerRun{ad & 0xFFFF, ad >> 16, (uint32_t)((s.piece_off[k + 1] - s.piece_off[k]) % kAdlerMod)};
        }
        uint32_t round;
        const uint32_t before = wave_excl_scan_u32(l, (int)lane, round);
        if (live) s.piece_adler[k] = at + before;
        at += round;
        // lane j ends with the join of lanes j .. 63, in order: after the step `o` it holds j .. j + 2 o - 1
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            AdlerRun y;
            y.a = __shfl_down(r.a, o, kWave);
            y.b = __shfl_down(r.b, o, kWave);
            y.n = __shfl_down(r.n, o, kWave);
            if (lane + o < (uint32_t)kWave) r = adler_join(r, y);  // (behind lane 63: the empty run)
        }
        AdlerRun chunk{uni(r.a), uni(r.b), uni(r.n)};
        whole = adler_join(whole, chunk);
    }
    if (lane == 0) {
        uint8_t* o = s.out + s.out_off[i];
        o[0] = 0x78;
        o[1] = 0x01;
        uint8_t* t = o + 2 + sum;
        t[0] = (uint8_t)(whole.b >> 8);
        t[1] = (uint8_t)whole.b;
        t[2] = (uint8_t)(whole.a >> 8);
        t[3] = (uint8_t)whole.a;
        s.out_len[i] = (uint32_t)total;
    }
}

// Piece k goes to out[out_off[i] + piece_adler[k] ..), i the input whose range of first_piece holds k.  The source
// has any alignment and so has the destination: the bytes up to the destination's next 16-byte boundary go one per
// thread, the body as 16-byte stores on that alignment (the loads take the source as it lies; the hardware reads a
// misaligned 16 bytes), the rest one per thread again.  Loads stay inside the piece, stores inside its place.
__global__ __launch_bounds__(kCopyThreads) void stitch_copy_kernel(StitchArgs s) {
    const uint32_t t = threadIdx.x;
    const uint64_t p0 = s.first_piece[0], p1 = s.first_piece[s.n];
    for (uint64_t k = p0 + blockIdx.x; k < p1; k += gridDim.x) {
        const uint32_t at = s.piece_adler[k];
        if (at == kStitchFailed) continue;
        // the last input whose first piece is not behind k
        uint64_t lo = 0, hi = s.n;  // first_piece[lo] <= k < first_piece[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (s.first_piece[mid] <= k)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t len = s.piece_len[k];
        const uint8_t* __restrict__ src = s.pieces + s.piece_slot_off[k];
        uint8_t* __restrict__ dst = s.out + s.out_off[lo] + at;
        const uint32_t head = min(len, (uint32_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
        if (t < head) dst[t] = src[t];
        const uint32_t lines = (len - head) / 16, tail0 = head + 16 * lines;
        for (uint32_t v = t; v < lines; v += kCopyThreads) {
            uint4 x;
            __builtin_memcpy(&x, src + head + 16 * (uint64_t)v, 16);
            *reinterpret_cast<uint4*>(dst + head + 16 * (uint64_t)v) = x;
        }
        if (t < len - tail0) dst[tail0 + t] = src[tail0 + t];
    }
}

}  // namespace fdh

extern "C" int fdh_launch_deflate_stitch(const uint8_t* pieces, const uint64_t* piece_slot_off, const uint32_t* piece_len,
                                         uint32_t* piece_adler, const uint64_t* piece_off, const uint64_t* first_piece, uint8_t* out,
                                         const uint64_t* out_off, uint32_t* out_len, uint64_t n, hipStream_t stream) {
    if (n == 0) return 0;
    int dev = 0, cus = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return (int)e;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const fdh::StitchArgs s{pieces, piece_slot_off, piece_len, piece_adler, piece_off, first_piece, out, out_off, out_len, n};
    hipLaunchKernelGGL(fdh::stitch_plan_kernel, dim3((unsigned)n), dim3(fdh::kWave), 0, stream, s);
    // the pieces number n at the least and the host knows no more: eight workgroups per CU stride over them
    hipLaunchKernelGGL(fdh::stitch_copy_kernel, dim3((unsigned)cus * 8), dim3(fdh::kCopyThreads), 0, stream, s);
    return (int)hipGetLastError();
}
