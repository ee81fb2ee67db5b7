// png_filter.hip -- PNG scanline reconstruction ("unfilter", the step the png crate runs on the
// decoder's output) and filtering (the step in front of the ultra-fast encoder), batched.
//
// Not part of the fdeflate crate itself (its reverse dependency image-rs/image-png does it,
// reference README.md:11); the algorithm is the PNG specification's (W3C / ISO/IEC 15948 section
// 9.2 "Filter types for filter method 0", 9.4 Paeth): types 0 None, 1 Sub, 2 Up, 3 Average,
// 4 Paeth over bytes, `bpp` bytes per pixel, arithmetic modulo 256, zero to the left of the first
// pixel and above the first row.
//
// Reconstruction is serial along a row for Sub / Average / Paeth (byte x needs byte x - bpp of the
// SAME row) and serial down the rows for Up / Average / Paeth, and neighbouring rows may use
// different types: a pixel needs its left, upper and upper-left neighbours, which leaves the
// anti-diagonals of an image as the independent work.  png_wave_kernel (the default) gives an image
// to a wavefront and runs the rows of a 64-row band on the 64 lanes, skewed by one 16-byte chunk per
// row; png_filter_kernel (FDH_PNG_LANE_PER_IMAGE=1) gives an image to a lane.  Both walk rows 16
// bytes at a time in registers with static indexing, the predictor of every type computed
// branch-free and selected by per-row byte masks, so lanes whose rows have different types do not
// diverge.  Filtering has no such dependence (the predictors use raw neighbours).
#include "device_common.h"
#include "png_rows.h"

#include <hip/hip_cooperative_groups.h>

#include <algorithm>
#include <cstdlib>

namespace fdh {

struct PngArgs {
    const uint8_t* src;       // unfilter: filtered rows (type byte + row_bytes each); filter: pixels
    const uint64_t* src_off;  // n + 1
    uint8_t* dst;             // unfilter: pixels; filter: filtered rows
    const uint64_t* dst_off;  // n + 1
    const uint8_t* types;     // filter only: one type per row, all images back to back
    const uint64_t* types_off;  // filter only: n + 1
    uint32_t* status;         // 0 ok, 1 filter type > 4, 2 sizes do not fit, 3 skipped (gate)
    const uint32_t* gate;     // nullable: image i is processed only if gate[i] == 0 (the decoder's status)
    const uint32_t* gate_len; // nullable (with gate): ... and gate_len[i] (the decoded length) fills the source slot
                              // exactly: a stream that ends early leaves stale bytes behind it -> status 2
    uint64_t n;
    uint32_t row_bytes;
};

// One row of one image, walked by one lane.
template <int BPP, bool UNFILTER>
__device__ __forceinline__ void png_row(const uint8_t* in, const uint8_t* up, uint8_t* out, uint32_t row_bytes, uint32_t type) {
    const PngMasks m(type);
    uint32_t la[8], ua[8];
#pragma unroll
    for (int k = 0; k < 8; k++) la[k] = ua[k] = 0;
    uint32_t x = 0;
    for (; x + 16 <= row_bytes; x += 16) {
        const uint4 f = png_load16(in + x);
        uint4 u = make_uint4(0, 0, 0, 0);
        if (up) u = png_load16(up + x);
        png_store16(out + x, png_chunk<BPP, UNFILTER>(f, u, la, ua, m));
    }
    // the last < 16 bytes, byte by byte, the tails rotating through la / ua
    for (; x < row_bytes; x++) {
        const uint32_t b = up ? up[x] : 0u;
        const uint32_t a = la[8 - BPP], c = ua[8 - BPP];
        const uint32_t fv = in[x];
        const uint32_t pr = m.pred(a, b, c);
        const uint32_t ov = (UNFILTER ? fv + pr : fv - pr) & 0xFF;
        out[x] = (uint8_t)ov;
#pragma unroll
        for (int k = 8 - BPP; k < 7; k++) {
            la[k] = la[k + 1];
            ua[k] = ua[k + 1];
        }
        la[7] = UNFILTER ? ov : fv;
        ua[7] = b;
    }
}

// 0: process image i; 3: its stream did not decode; 2: it decoded to fewer bytes than the slot holds
__device__ __forceinline__ uint32_t png_gate(const PngArgs& a, uint64_t i) {
    if (!a.gate) return 0;
    if (a.gate[i] != 0) return 3;
    if (a.gate_len && (uint64_t)a.gate_len[i] != a.src_off[i + 1] - a.src_off[i]) return 2;
    return 0;
}

template <int BPP, bool UNFILTER>
__global__ __launch_bounds__(kWave) void png_filter_kernel(PngArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (i >= a.n) return;
    if (const uint32_t g = png_gate(a, i)) {
        a.status[i] = g;
        return;
    }
    const uint64_t s0 = a.src_off[i], s1 = a.src_off[i + 1], d0 = a.dst_off[i], d1 = a.dst_off[i + 1];
    const uint64_t rb = a.row_bytes;
    const uint64_t src_row = UNFILTER ? rb + 1 : rb, dst_row = UNFILTER ? rb : rb + 1;
    const uint64_t rows = (s1 - s0) / src_row;
    uint32_t st = 0;
    if (rows * src_row != s1 - s0 || rows * dst_row > d1 - d0) st = 2;
    if (!UNFILTER && st == 0 && a.types_off[i + 1] - a.types_off[i] < rows) st = 2;
    for (uint64_t r = 0; r < rows && st == 0; r++) {
        const uint8_t* in = a.src + s0 + r * src_row;
        uint8_t* out = a.dst + d0 + r * dst_row;
        if (UNFILTER) {
            const uint32_t t = in[0];
            if (t > 4) {
                st = 1;
                break;
            }
            png_row<BPP, true>(in + 1, r ? out - rb : nullptr, out, a.row_bytes, t);
        } else {
            const uint32_t t = a.types[a.types_off[i] + r];
            if (t > 4) {
                st = 1;
                break;
            }
            out[0] = (uint8_t)t;
            png_row<BPP, false>(in, r ? in - rb : nullptr, out + 1, a.row_bytes, t);
        }
    }
    a.status[i] = st;
}

__device__ __forceinline__ uint32_t png_from_lane_below(uint32_t x) {  // lane j gets lane j - 1's value (lane 0: 0)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}

// One image per WAVEFRONT: lane j takes row j of a band of 64 rows.  Reconstruction needs the row
// above, so the lanes run skewed by one 16-byte chunk: at step t lane j works on chunk t - j, and
// the chunk above it is what lane j - 1 produced one step earlier -- it arrives through a DPP lane
// shift, not through memory (row 0 of a later band reads the last row of the band before from the
// output).  Filtering has no such dependence (the predictors use raw neighbours): no skew, the row
// above is the chunk lane j - 1 read in the same step.  Same per-chunk arithmetic as the
// lane-per-image kernel.
//
// Memory: with 16 bytes per lane per step and the rows 1 KiB or more apart, a wavefront touches 64
// different cache lines per access and comes back to each of them eight times; with sixteen
// wavefronts per CU the lines do not survive in the caches in between, and every 16 bytes cost a
// whole line of traffic (measured: the kernel ran at the same speed with the arithmetic removed,
// and with it doubled).  So every lane moves whole 128-byte lines: eight back-to-back loads fill a
// register set one line ahead of the row's position, the set is parked in an LDS line buffer when
// the row gets there, and the output goes through a second line buffer and leaves as eight
// back-to-back stores when a line is complete.
struct PngWaveLds {
    uint4 lin[kWave][8];   // the 128-byte line of the row each lane is reading
    uint4 lout[kWave][8];  // the line each lane is producing
    uint4 lup[8];          // lane 0 of a later band: the line of the row above
};

template <int BPP, bool UNFILTER>
__global__ __launch_bounds__(kWave) void png_wave_kernel(PngArgs a) {
    __shared__ PngWaveLds lds;
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    if (const uint32_t g = png_gate(a, i)) {
        if (lane == 0) a.status[i] = g;
        return;
    }
    const uint64_t s0 = a.src_off[i], s1 = a.src_off[i + 1], d0 = a.dst_off[i], d1 = a.dst_off[i + 1];
    const uint64_t rb = a.row_bytes;
    const uint64_t src_row = UNFILTER ? rb + 1 : rb, dst_row = UNFILTER ? rb : rb + 1;
    const uint64_t rows = (s1 - s0) / src_row;
    uint32_t st = 0;
    if (rows * src_row != s1 - s0 || rows * dst_row > d1 - d0) st = 2;
    if (!UNFILTER && st == 0 && a.types_off[i + 1] - a.types_off[i] < rows) st = 2;
    const uint32_t nchunks = (uint32_t)((rb + 15) / 16);
    const uint8_t* const src_end = a.src + s1;
    const uint8_t* const dst_end = a.dst + d0 + rows * dst_row;
    // the eight 16-byte pieces of line `ln` of the row at `row`; reads stay below `end`
    auto fetch = [&](const uint8_t* row, const uint8_t* end, uint32_t ln, uint4(&regs)[8]) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t o = (uint64_t)ln * 128 + (uint64_t)k * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (o < rb) v = row + o + 16 <= end ? png_load16(row + o) : png_load_part(row + o, (uint32_t)min((uint64_t)16, rb - o));
            regs[k] = v;
        }
    };
    for (uint64_t r0 = 0; r0 < rows && st == 0; r0 += kWave) {
        const uint64_t r = r0 + lane;
        const bool have = r < rows;
        const uint8_t* in = a.src + s0 + r * src_row + (UNFILTER ? 1 : 0);
        uint8_t* out = a.dst + d0 + r * dst_row + (UNFILTER ? 0 : 1);
        uint32_t t = 0;
        if (have) t = UNFILTER ? in[-1] : a.types[a.types_off[i] + r];
        // rows from the first bad filter type on are not produced (the serial walk stops there)
        const uint64_t bad = __ballot(have && t > 4);
        uint32_t band = (uint32_t)min((uint64_t)kWave, rows - r0);
        if (bad) {
            band = (uint32_t)__builtin_ctzll(bad);
            st = 1;
        }
        const bool mine = lane < band;
        if (!UNFILTER && mine) out[-1] = (uint8_t)t;
        const PngMasks m(t);
        uint32_t la[8], ua[8];
#pragma unroll
        for (int k = 0; k < 8; k++) la[k] = ua[k] = 0;
        // the row above lane 0's row, from memory: the output of the band before / the raw input
        const bool from_memory = lane == 0 && r > 0;
        const uint8_t* const uprow = (UNFILTER ? out : in) - rb;
        const uint8_t* const upend = UNFILTER ? dst_end : src_end;
        uint4 pf[8];  // the line behind the one in lds.lin
        if (mine) {
            fetch(in, src_end, 0, pf);
#pragma unroll
            for (int k = 0; k < 8; k++) lds.lin[lane][k] = pf[k];
            fetch(in, src_end, 1, pf);
        }
        uint4 last = make_uint4(0, 0, 0, 0);  // what the lane below needs: this lane's output / input chunk
        const uint32_t steps = band ? nchunks + (UNFILTER ? band - 1 : 0) : 0;
        for (uint32_t step = 0; step < steps; step++) {
            const uint32_t c = step - (UNFILTER ? lane : 0);  // (wraps for the lanes that have not started)
            const bool on = mine && c < nchunks;
            if (on && (c & 7) == 0) {  // entering a line
                if (c) {
#pragma unroll
                    for (int k = 0; k < 8; k++) lds.lin[lane][k] = pf[k];
                    fetch(in, src_end, (c >> 3) + 1, pf);
                }
                if (from_memory) {
                    uint4 up[8];
                    fetch(uprow, upend, c >> 3, up);
#pragma unroll
                    for (int k = 0; k < 8; k++) lds.lup[k] = up[k];
                }
            }
            uint4 f = make_uint4(0, 0, 0, 0);
            if (on) f = lds.lin[lane][c & 7];
            if (!UNFILTER) last = f;
            uint4 u = make_uint4(png_from_lane_below(last.x), png_from_lane_below(last.y), png_from_lane_below(last.z), png_from_lane_below(last.w));
            if (on) {
                if (lane == 0) u = r > 0 ? lds.lup[c & 7] : make_uint4(0, 0, 0, 0);
                const uint4 o = png_chunk<BPP, UNFILTER>(f, u, la, ua, m);
                if (UNFILTER) last = o;
                lds.lout[lane][c & 7] = o;
                if ((c & 7) == 7 || c == nchunks - 1) {  // the line is complete: out it goes
                    const uint64_t base = (uint64_t)(c >> 3) * 128;
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const uint64_t o16 = base + (uint64_t)k * 16;
                        if ((uint32_t)k <= (c & 7) && o16 < rb) png_store_part(out + o16, lds.lout[lane][k], (uint32_t)min((uint64_t)16, rb - o16));
                    }
                }
            }
        }
        // the next band's first row reads this band's last row back
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) a.status[i] = st;
}

// ---- reconstruction as one pipeline over many images ------------------------------------------
//
// png_wave_kernel pays for its skew twice on small images: a band of 64 rows of N chunks takes
// N + 63 steps (half the lane-steps idle for the bench's 64-chunk rows), and because every lane
// crosses its 128-byte line boundaries at a different step, every step issues the line loads and
// stores for an eighth of the lanes (the CU's one address unit ends up the busiest unit).  Here
// the rows of `per_wave` consecutive images form ONE sequence R = 0, 1, 2, ...: row R belongs to
// lane R % 64 and starts at step (R % 64) + (R / 64) * P, P = max(N rounded up to 8, 64), so a lane
// goes from one of its rows to the next without waiting and the ramp is paid once per wavefront.
// The row above is still one lane below and one step ahead (lane 63 hands its chunks to lane 0
// through an LDS row buffer, P - 63 steps ahead); the first row of an image has no row above.
// Memory moves at wavefront-uniform steps: every eighth step each lane parks the line it fetched
// eight steps ago in its double-buffered LDS line, fetches the line it will enter next, and writes
// out the line it completed last -- eight full-width loads and stores per eight steps.
constexpr uint32_t kPipeMaxChunks = 256;  // rows up to 4 KiB (the LDS row buffer)
constexpr uint32_t kPipeMaxImages = 8;
#ifndef FDH_PNG_IN_SLOT
#define FDH_PNG_IN_SLOT 4
#endif
// 16-byte chunks per line slot of the INPUT: 64 bytes (four loads in a row to one or two lines), two buffers, 8 KiB of LDS.  With
// the stores transposed this pays (4.99 -> 4.45 ms at 8 wavefronts per CU instead of 10); before, larger input slots only lost
// occupancy, and 128 bytes still do (6.9 ms at 5 per CU).
constexpr int kSlot = FDH_PNG_IN_SLOT;
#ifndef FDH_PNG_OUT_SLOT
#define FDH_PNG_OUT_SLOT 8
#endif
// ... and of the output: 128 bytes, stored TRANSPOSED (the step loop: eight lanes to a row).  The kernel's time follows its
// occupancy and its memory instructions -- compiled without its stores it took 3.0 instead of 6.6 ms, without its loads 3.7,
// without both 2.6 --: a lane storing its own row's bytes makes 64 pieces of 16 bytes in 64 lines per instruction.  A lane
// storing 64 bytes at once (four stores in a row): 6.56 -> 6.16 ms; non-temporal stores: 14 ms; the eight rows whose 128-byte
// slot is complete at a step stored by eight lanes each, from ONE buffer per lane: 6.5 -> 5.35 ms.
constexpr int kOut = FDH_PNG_OUT_SLOT;

struct PngPipeLds {
    uint4 lin[kWave][2][kSlot];
    uint4 lout[kWave][kOut];   // (one buffer: a slot is stored at the step it is complete, before its owner's next chunk)
    uint4 rdesc[kWave][2];     // per lane, row count & 1: where the row's output starts (x, y), whether it is produced (z)
    uint64_t sbase[kPipeMaxImages + 1], dbase[kPipeMaxImages];  // offsets of the images' buffers (sbase[j + 1]: end of j's)
    uint32_t rowsum[kPipeMaxImages + 1];
    uint32_t bad[kPipeMaxImages];  // first row with a bad filter type, per image
};

struct PngPipeRow {  // one row of the sequence, as a lane sees it
    const uint8_t* in;  // first filtered byte (behind the type byte)
    uint8_t* out;
    uint32_t r, img;    // row in its image; image slot in the wavefront
    uint32_t type;
    bool valid;         // the sequence has this row
    bool produced;      // ... and it is reconstructed (no bad filter type at or before it)
};

template <int BPP>
__global__ __launch_bounds__(kWave) void png_pipe_kernel(PngArgs a, uint32_t per_wave) {
    __shared__ PngPipeLds lds;
    extern __shared__ uint4 png_rowbuf[];  // lane 63 -> lane 0: one row of chunks (sized by the launch)
    const uint32_t lane = threadIdx.x;
    const uint64_t img0 = (uint64_t)blockIdx.x * per_wave;
    const uint32_t cnt = (uint32_t)min((uint64_t)per_wave, a.n - img0);
    const uint64_t rb = a.row_bytes;
    const uint32_t N = (uint32_t)((rb + 15) / 16);
    const uint32_t P = max((N + 7) & ~7u, (uint32_t)kWave);
    // ---- the images of this wavefront: row counts, statuses ----
    uint32_t my_rows = 0, my_st = 0;
    if (lane < cnt) {
        const uint64_t i = img0 + lane;
        if (const uint32_t g = png_gate(a, i)) {
            my_st = g;
        } else {
            const uint64_t fl = a.src_off[i + 1] - a.src_off[i], pl = a.dst_off[i + 1] - a.dst_off[i];
            const uint64_t rows = fl / (rb + 1);
            if (rows * (rb + 1) != fl || rows * rb > pl) my_st = 2;
            else my_rows = (uint32_t)rows;
        }
        lds.bad[lane] = 0xFFFFFFFFu;
        lds.sbase[lane] = a.src_off[i];
        lds.dbase[lane] = a.dst_off[i];
        if (lane + 1 == cnt) lds.sbase[cnt] = a.src_off[i + 1];
    }
    {   // prefix sums of the row counts (at most eight images: by hand)
        uint32_t sum = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            if (lane == 0) lds.rowsum[j] = sum;
            sum += (uint32_t)__builtin_amdgcn_readlane((int)my_rows, (int)j);
        }
        if (lane == 0) lds.rowsum[cnt] = sum;
    }
    wave_sync();
    const uint32_t T = lds.rowsum[cnt];
    // A lane's rows come in increasing order: the image is searched on from the one of its last row.
    // (One lane starts a row at every step, so this runs at every step: kept short, and without a
    // global load on the way to the type byte's address.)
    auto describe = [&](uint32_t R, uint32_t j) -> PngPipeRow {
        PngPipeRow d{nullptr, nullptr, 0, 0, 0, false, false};
        if (R >= T) return d;
        while (lds.rowsum[j + 1] <= R) j++;  // (R < T = rowsum[cnt] ends it)
        d.r = R - lds.rowsum[j];
        d.img = j;
        d.in = a.src + lds.sbase[j] + (uint64_t)d.r * (rb + 1) + 1;
        d.out = a.dst + lds.dbase[j] + (uint64_t)d.r * rb;
        d.type = d.in[-1];
        d.valid = true;
        return d;
    };
    // reads of a row's lines stay inside its image's filtered bytes (+ the next row's, harmless)
    auto fetch = [&](const PngPipeRow& d, uint32_t ln, uint4(&regs)[kSlot]) {
        const uint8_t* const end = a.src + lds.sbase[d.img + 1];
        // A line inside the IMAGE's filtered bytes: plain loads.  (Until round 6: a line inside the ROW -- a row's last,
        // partial line went the other way, and as one lane has such a line at every memory step, every step's loads were
        // followed by that path's `s_waitcnt vmcnt(0)`: its zeros go to the registers the loads are in flight to.  What a
        // plain load reads behind the row's end are the next row's bytes: they stay in positions that are never stored.)
        if (d.valid && d.in + (uint64_t)(ln + 1) * (16 * kSlot) <= end) {
#pragma unroll
            for (int k = 0; k < kSlot; k++) regs[k] = png_load16(d.in + (uint64_t)ln * (16 * kSlot) + (uint64_t)k * 16);
            return;
        }
#pragma unroll
        for (int k = 0; k < kSlot; k++) {
            const uint64_t o = (uint64_t)ln * (16 * kSlot) + (uint64_t)k * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (d.valid && o < rb) v = d.in + o + 16 <= end ? png_load16(d.in + o) : png_load_part(d.in + o, (uint32_t)min((uint64_t)16, rb - o));
            regs[k] = v;
        }
    };
    // A lane starts its row k at step 2 * kSlot + k * P + lane and needs the description of row k + 1 there (its lines are
    // fetched ahead).  Until round 6 it was made right there -- an LDS search, 64-bit address arithmetic and the load of
    // the row's type byte, waited for on the spot -- and as ONE lane starts a row at every step, every lane of the
    // wavefront went through those ~90 instructions and that memory round trip at every step.  Now all lanes describe
    // their row k + 2 together, once per P steps (when lane 0 starts its row k), and hand the description down a
    // two-deep queue: a period of at least 64 steps lies between the load of a type byte and its use.
    PngPipeRow prev{nullptr, nullptr, 0, 0, 0, false, false}, cur = prev, next = describe(lane, 0);
    PngPipeRow nn = prev, nn2 = describe(kWave + lane, next.img);
    uint32_t cu = P - 2 * kSlot, ku = 0;  // lane 0's position in its period; the row period it is in
    // position in the period of row k (signed: negative long before the lane's first row); it reaches
    // P (= 0 of the next row) after lane + 16 steps -- two uniform steps ahead of the first chunk, one
    // to fetch its line and one to park it
    int32_t c = (int32_t)P - (int32_t)lane - 2 * kSlot;
    uint32_t k = 0xFFFFFFFFu;  // rows of this lane started so far, minus one
    uint32_t la[8], ua[8];
#pragma unroll
    for (int q = 0; q < 8; q++) la[q] = ua[q] = 0;
    PngMasks m(0);
    uint4 pf[kSlot], last = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < kSlot; q++) pf[q] = make_uint4(0, 0, 0, 0);
    const uint32_t kmax = T ? (T - 1) / kWave : 0;
    // the last slot of the last row ends before step kmax * P + 63 + 16 + (N rounded up to 8); the
    // uniform step behind that writes its line
    const uint32_t steps = T ? ((kmax * P + kWave + 2 * kSlot + ((N + 7) & ~7u) + 7) & ~7u) + 1 : 0;
    for (uint32_t step = 0; step < steps; step++) {
        if (cu == P) {  // lane 0 starts its row ku: every lane's row ku + 1 is due from now on, row ku + 2 is looked up
            cu = 0;
            nn = nn2;
            nn2 = describe((ku + 2) * kWave + lane, nn.img);
            ku++;
        }
        cu++;
        if (c == (int32_t)P) {  // this lane starts its next row
            c = 0;
            k++;
            prev = cur;
            cur = next;
            next = nn;
            if (cur.valid) {
                if (cur.type > 4) atomicMin(&lds.bad[cur.img], cur.r);
                cur.produced = cur.type <= 4 && cur.r < lds.bad[cur.img];
            }
            m = PngMasks(cur.type);
#pragma unroll
            for (int q = 0; q < 8; q++) la[q] = ua[q] = 0;
            const uint64_t op = reinterpret_cast<uint64_t>(cur.out);
            lds.rdesc[lane][k & 1] = make_uint4((uint32_t)op, (uint32_t)(op >> 32), (cur.valid && cur.produced) ? 1u : 0u, 0u);
        }
        {   // ---- write-out, TRANSPOSED.  A lane's slot of kOut chunks (128 bytes) is complete when its position is a multiple of
            //      kOut: at this step that is the lanes l = step - 2 kSlot (mod kOut), 64 / kOut rows.  Each of them is stored by the kOut
            //      lanes of its group, 16 bytes apiece: one store instruction per step, whose 64 pieces are eight runs of 128
            //      bytes (a lane storing its own row's bytes makes 64 pieces of 16 in 64 different lines).  The owner's position
            //      and row count follow from this lane's own -- positions differ by the lane distance --, where its row's output
            //      starts is in its rdesc entry.  The slot is read here, in front of the chunk its owner writes at this very
            //      step: one buffer is enough.
            wave_sync();
            const uint32_t owner = (lane & ~(uint32_t)(kOut - 1)) | ((step - 2 * kSlot) & (kOut - 1)), q = lane & (kOut - 1);  // (a lane's position is step - lane - 2 kSlot)
            int32_t co = c + (int32_t)lane - (int32_t)owner, ko = (int32_t)k;
            if (co >= (int32_t)P) {
                co -= (int32_t)P;
                ko++;
            } else if (co < 0) {
                co += (int32_t)P;
                ko--;
            }
            int32_t cfs = co - kOut;
            const bool back = cfs < 0;  // (that slot belongs to the row before)
            if (back) cfs += (int32_t)P;
            const int32_t kk = back ? ko - 1 : ko;
            const uint32_t cf = (uint32_t)cfs;
            const uint64_t o16 = (uint64_t)(cf + q) * 16;
            if (kk >= 0 && (co & (kOut - 1)) == 0 && cf + q < N && o16 < rb) {
                const uint4 ds = lds.rdesc[owner][kk & 1];
                if (ds.z) {
                    const uint4 v = lds.lout[owner][q];
                    uint8_t* const dst = reinterpret_cast<uint8_t*>(((uint64_t)ds.y << 32) | ds.x) + o16;
                    const uint32_t nb = (uint32_t)min((uint64_t)16, rb - o16);
                    if (nb == 16) png_store16(dst, v);
                    else png_store_part(dst, v, nb);
                }
            }
        }
        if ((step & (kSlot - 1)) == 0) {
            const int32_t ph = c & (kSlot - 1);
            {   // park the line fetched eight steps ago: the slot entered in (step, step + 8]
                const int32_t d1 = ph ? kSlot - ph : kSlot;
                int32_t c1 = c + d1;
                uint32_t k1 = k;
                if (c1 >= (int32_t)P) {
                    c1 -= (int32_t)P;
                    k1++;
                }
                const uint32_t par = (k1 * (P / kSlot) + ((uint32_t)c1 / kSlot)) & 1;
#pragma unroll
                for (int q = 0; q < kSlot; q++) lds.lin[lane][par][q] = pf[q];
            }
            {   // fetch the line of the slot entered in (step + 8, step + 16]
                const int32_t d2 = ph ? 2 * kSlot - ph : 2 * kSlot;
                int32_t c2 = c + d2;
                const bool wrap = c2 >= (int32_t)P;
                if (wrap) c2 -= (int32_t)P;
                const PngPipeRow& d = wrap ? next : cur;
                if ((uint32_t)c2 < N) {
                    fetch(d, (uint32_t)c2 / kSlot, pf);
                } else {
#pragma unroll
                    for (int q = 0; q < kSlot; q++) pf[q] = make_uint4(0, 0, 0, 0);
                }
            }
        }
        const uint32_t cu = (uint32_t)c;
        const bool on = cur.valid && cur.produced && cu < N;  // (cur.valid is false while c is negative)
        const uint32_t par = (k * (P / kSlot) + (cu / kSlot)) & 1;
        uint4 u = make_uint4(png_from_lane_below(last.x), png_from_lane_below(last.y), png_from_lane_below(last.z), png_from_lane_below(last.w));
        if (on) {
            const uint4 f = lds.lin[lane][par][cu & (kSlot - 1)];
            if (lane == 0) u = png_rowbuf[cu];
            if (cur.r == 0) u = make_uint4(0, 0, 0, 0);
            last = png_chunk<BPP, true>(f, u, la, ua, m);
            lds.lout[lane][cu & (kOut - 1)] = last;
            if (lane == kWave - 1) png_rowbuf[cu] = last;
        }
        c++;
    }
    if (lane < cnt) a.status[img0 + lane] = my_st ? my_st : (lds.bad[lane] != 0xFFFFFFFFu ? 1u : 0u);
}

}  // namespace fdh

// One image per wavefront by default; FDH_PNG_LANE_PER_IMAGE=1 selects the one-image-per-lane
// kernel (of use only for batches of very many images of a few rows each).
template <bool UNFILTER>
static int png_launch(const fdh::PngArgs& a, uint32_t bpp, hipStream_t stream) {
    if (a.n == 0) return 0;
    const char* e = getenv("FDH_PNG_LANE_PER_IMAGE");
    const bool per_lane = e && e[0] == '1';
    const char* e2 = getenv("FDH_PNG_NO_PIPELINE");
    // reconstruction of rows up to 4 KiB: the pipeline over several images per wavefront (more of
    // them when the batch is large enough to fill the GPU anyway)
    const bool pipe = UNFILTER && !per_lane && !(e2 && e2[0] == '1') && a.row_bytes <= 16 * fdh::kPipeMaxChunks;
    uint32_t per_wave = (uint32_t)std::min<uint64_t>(fdh::kPipeMaxImages, std::max<uint64_t>(1, a.n / 4096));
    if (const char* e3 = getenv("FDH_PNG_IMAGES_PER_WAVE")) {  // (tests: the multi-image pipeline on small batches)
        const int v = atoi(e3);
        if (v >= 1 && v <= (int)fdh::kPipeMaxImages) per_wave = (uint32_t)v;
    }
    const size_t rowbuf_bytes = (size_t)((a.row_bytes + 15) / 16) * 16;
    const dim3 block(fdh::kWave);
    const dim3 grid(per_lane ? (unsigned)((a.n + fdh::kWave - 1) / fdh::kWave) : pipe ? (unsigned)((a.n + per_wave - 1) / per_wave) : (unsigned)a.n);
#define FDH_PNG_CASE(B)                                                                                  \
    case B:                                                                                              \
        if (per_lane)                                                                                    \
            hipLaunchKernelGGL((fdh::png_filter_kernel<B, UNFILTER>), grid, block, 0, stream, a);        \
        else if (pipe)                                                                                   \
            hipLaunchKernelGGL((fdh::png_pipe_kernel<B>), grid, block, rowbuf_bytes, stream, a, per_wave); \
        else                                                                                             \
            hipLaunchKernelGGL((fdh::png_wave_kernel<B, UNFILTER>), grid, block, 0, stream, a);          \
        break;
    switch (bpp) {
        FDH_PNG_CASE(1)
        FDH_PNG_CASE(2)
        FDH_PNG_CASE(3)
        FDH_PNG_CASE(4)
        FDH_PNG_CASE(6)
        FDH_PNG_CASE(8)
        default: return -1;
    }
#undef FDH_PNG_CASE
    return (int)hipGetLastError();
}

extern "C" int fdh_launch_png_unfilter(const uint8_t* filt, const uint64_t* filt_off, uint8_t* pix, const uint64_t* pix_off,
                                       uint32_t* status, const uint32_t* gate, const uint32_t* gate_len, uint64_t n,
                                       uint32_t row_bytes, uint32_t bpp, hipStream_t stream) {
    fdh::PngArgs a{filt, filt_off, pix, pix_off, nullptr, nullptr, status, gate, gate_len, n, row_bytes};
    return png_launch<true>(a, bpp, stream);
}

extern "C" int fdh_launch_png_filter(const uint8_t* pix, const uint64_t* pix_off, const uint8_t* types,
                                     const uint64_t* types_off, uint8_t* filt, const uint64_t* filt_off, uint32_t* status,
                                     uint64_t n, uint32_t row_bytes, uint32_t bpp, hipStream_t stream) {
    fdh::PngArgs a{pix, pix_off, filt, filt_off, types, types_off, status, nullptr, nullptr, n, row_bytes};
    return png_launch<false>(a, bpp, stream);
}

// ---- filter selection: which of the five types each row is filtered with ------------------------
//
// The heuristic of the PNG specification (12.8, libpng's default): filter the row with every type,
// read each filtered byte as signed, sum the absolute values (128 counts 128), take the type with the
// smallest sum, the LOWEST type number on equal sums.  With p the predictor as an integer 0..255 the
// cost of a byte x is min(|x - p|, 256 - |x - p|) whichever way the difference wraps.
//
// Filtering uses the raw neighbours, so a row's choice depends on pixel rows r and r - 1 only: no
// skew, no serial walk.  The lanes lie ALONG the row, 16 bytes each.  A row has a group of G lanes
// (a power of two, 1..64), a wavefront works on 64 / G consecutive rows per step and walks down a
// band of kChooseBand rows of one image; the band's bytes are read front to back in runs of whole
// rows.  The row above a group's row is the chunk the group before it holds in the same step (the
// first group: what the last group held one step earlier), fetched with one cross-lane read per
// dword, so a pixel byte is loaded once and serves as "current" and as "above".  The byte `bpp` to
// the left comes from the lane below (DPP shift), not from a second, overlapping load.  Rows wider
// than 16 G bytes (J > 1 pieces per lane) loop along the row and accumulate; they read the row
// above from memory again (the registers cannot hold a row of any length; it is the row the same
// wavefront has just read).
//
// None, Sub, Up and Average are computed four bytes to a word (byte-wise subtraction in a 32-bit
// word, fold of the negative bytes, v_sad_u8 against zero plus the count of sign bits); Paeth byte by
// byte with png_paeth.  A lane's five sums over 16 bytes are at most 2048 each, sixteen lanes' at
// most 32768: two sums share a word for the four reduction steps inside a row of sixteen lanes.
namespace fdh {

constexpr uint32_t kChooseBand = 64;  // rows per band: one band = one image of the bench shape

struct PngChooseArgs {
    const uint8_t* pix;
    const uint64_t* pix_off;    // n + 1
    uint8_t* types;             // one byte per row
    const uint64_t* types_off;  // n + 1
    uint32_t* status;           // 0 ok, 2 sizes do not fit
    uint64_t n;
    uint32_t row_bytes;
    uint32_t group;             // G: lanes per row
    uint32_t pieces;            // J: 16 G-byte pieces per row
};

constexpr uint32_t kHi = 0x80808080u;

// x - p byte by byte, modulo 256
__device__ __forceinline__ uint32_t png_sub4(uint32_t x, uint32_t p) { return ((x | kHi) - (p & ~kHi)) ^ ((x ^ ~p) & kHi); }
// floor((a + b) / 2) byte by byte (the sum is not taken modulo 256)
__device__ __forceinline__ uint32_t png_avg4(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
// acc + the costs of the four filtered bytes of f: a byte v >= 128 costs 256 - v = (v ^ 0xFF) + 1
__device__ __forceinline__ uint32_t png_cost4(uint32_t f, uint32_t acc) {
    const uint32_t s = f & kHi;
    const uint32_t fold = f ^ (s | (s - (s >> 7)));
    return __builtin_amdgcn_sad_u8(fold, 0u, acc) + (uint32_t)__builtin_popcount(s);
}
// the 16 bytes that lie BPP in front of the chunk v: (tz, tw) are the last 8 bytes in front of it
template <int BPP>
__device__ __forceinline__ uint4 png_left16(const uint4& v, uint32_t tz, uint32_t tw) {
    const uint32_t s[6] = {tz, tw, v.x, v.y, v.z, v.w};
    constexpr int wi = (8 - BPP) / 4, sh = (8 - BPP) % 4;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = sh ? (uint32_t)(((((uint64_t)s[wi + k + 1]) << 32) | s[wi + k]) >> (8 * sh)) : s[wi + k];
    return make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ uint4 png_and16(const uint4& v, const uint4& m) { return make_uint4(v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w); }
// all ones in the first `valid` (0..16) bytes
__device__ __forceinline__ uint4 png_valid_mask(uint32_t valid) {
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = valid >= 4u * k + 4 ? 0xFFFFFFFFu : (valid <= 4u * k ? 0u : (1u << (8 * (valid - 4u * k))) - 1u);
    return make_uint4(m[0], m[1], m[2], m[3]);
}
// the costs of one chunk under the five types, added to sum[]: x the pixels, b the row above, a / c the bytes BPP to their left
__device__ __forceinline__ void png_costs16(const uint4& x, const uint4& a, const uint4& b, const uint4& c, uint32_t (&sum)[5]) {
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        sum[0] = png_cost4(xs[k], sum[0]);
        sum[1] = png_cost4(png_sub4(xs[k], as[k]), sum[1]);
        sum[2] = png_cost4(png_sub4(xs[k], bs[k]), sum[2]);
        sum[3] = png_cost4(png_sub4(xs[k], png_avg4(as[k], bs[k])), sum[3]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t d = __builtin_amdgcn_sad_u8(png_byte(x, k), png_paeth(png_byte(a, k), png_byte(b, k), png_byte(c, k)), 0u);
        sum[4] += min(d, 256u - d);
    }
}
template <int CTRL>
__device__ __forceinline__ uint32_t png_dpp_add(uint32_t v) { return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
// v summed over the aligned group of `group` lanes (a power of two) this lane is in; every lane gets the sum
__device__ __forceinline__ uint32_t png_group_sum16(uint32_t v, uint32_t group) {  // the steps inside 16 lanes
    if (group >= 2) v = png_dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    if (group >= 4) v = png_dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    if (group >= 8) v = png_dpp_add<0x141>(v);  // row_half_mirror: the other quad of eight lanes
    if (group >= 16) v = png_dpp_add<0x140>(v); // row_mirror: the other eight of sixteen
    return v;
}
__device__ __forceinline__ uint32_t png_group_sum64(uint32_t v, uint32_t group) {  // ... and across them
    if (group >= 32) v += (uint32_t)__shfl_xor((int)v, 16, 64);
    if (group >= 64) v += (uint32_t)__shfl_xor((int)v, 32, 64);
    return v;
}
__device__ __forceinline__ uint4 png_shfl16(const uint4& v, int src) {
    return make_uint4((uint32_t)__shfl((int)v.x, src, 64), (uint32_t)__shfl((int)v.y, src, 64), (uint32_t)__shfl((int)v.z, src, 64), (uint32_t)__shfl((int)v.w, src, 64));
}

// LOOP: rows of more than one piece per lane (J > 1).
template <int BPP, bool LOOP>
__global__ __launch_bounds__(kWave) void png_choose_kernel(PngChooseArgs a) {
    const uint64_t i = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint64_t s0 = a.pix_off[i], s1 = a.pix_off[i + 1], t0 = a.types_off[i], t1 = a.types_off[i + 1];
    const uint64_t rb = a.row_bytes;
    const uint64_t rows = (s1 - s0) / rb;
    const bool fits = rows * rb == s1 - s0 && t1 - t0 == rows;
    if (blockIdx.y == 0 && lane == 0) a.status[i] = fits ? 0u : 2u;
    if (!fits) return;
    const uint32_t G = a.group, R = kWave / G;  // lanes per row, rows per step
    const uint32_t g = lane / G, q = lane & (G - 1);
    const uint8_t* const img = a.pix + s0;
    const uint8_t* const end = a.pix + s1;
    // 16 bytes of row r at x, zero behind the row's end; never reads behind the image
    auto load = [&](uint64_t r, uint64_t x) -> uint4 {
        if (x >= rb) return make_uint4(0, 0, 0, 0);
        const uint8_t* const p = img + r * rb + x;
        const uint32_t valid = (uint32_t)min((uint64_t)16, rb - x);
        const uint4 v = p + 16 <= end ? png_load16(p) : png_load_part(p, valid);
        return png_and16(v, png_valid_mask(valid));
    };
    uint8_t* const types = a.types + t0;
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
            uint32_t sum[5] = {0, 0, 0, 0, 0};
            if (!LOOP) {
                const uint64_t x = (uint64_t)q * 16;
                const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                uint4 cur = make_uint4(0, 0, 0, 0);
                if (have) cur = load(r, x);
                // the row above: the group before this one holds it (group 0: the last group's chunk of the step before)
                uint4 up = cur;
                if (G < kWave) up = png_shfl16(g == R - 1 ? held : cur, (int)((lane - G) & (kWave - 1)));
                else up = held;
                held = cur;
                if (r == 0) up = make_uint4(0, 0, 0, 0);
                const bool first = q == 0;  // nothing to the left of the row's first pixel
                uint32_t cz = png_from_lane_below(cur.z), cw = png_from_lane_below(cur.w);
                uint32_t uz = png_from_lane_below(up.z), uw = png_from_lane_below(up.w);
                if (first) cz = cw = uz = uw = 0;
                const uint4 left = png_and16(png_left16<BPP>(cur, cz, cw), mask);
                const uint4 upleft = png_and16(png_left16<BPP>(up, uz, uw), mask);
                png_costs16(cur, left, up, upleft, sum);
                // two sums to a word inside sixteen lanes (at most 32768 each)
                uint32_t w0 = png_group_sum16(sum[0] | (sum[1] << 16), G), w1 = png_group_sum16(sum[2] | (sum[3] << 16), G);
                sum[4] = png_group_sum16(sum[4], G);
                sum[0] = w0 & 0xFFFF, sum[1] = w0 >> 16, sum[2] = w1 & 0xFFFF, sum[3] = w1 >> 16;
            } else {
                uint32_t cz = 0, cw = 0, uz = 0, uw = 0;  // lane q == 0: the bytes in front of its piece (the group's last lane had them)
                const int last = (int)(lane | (G - 1));
                for (uint32_t j = 0; j < a.pieces; j++) {
                    const uint64_t x = ((uint64_t)j * G + q) * 16;
                    const uint4 mask = png_valid_mask(x < rb ? (uint32_t)min((uint64_t)16, rb - x) : 0u);
                    uint4 cur = make_uint4(0, 0, 0, 0), up = cur;
                    if (have) cur = load(r, x);
                    if (have && r > 0) up = load(r - 1, x);
                    uint32_t lz = png_from_lane_below(cur.z), lw = png_from_lane_below(cur.w);
                    uint32_t vz = png_from_lane_below(up.z), vw = png_from_lane_below(up.w);
                    if (q == 0) lz = cz, lw = cw, vz = uz, vw = uw;
                    cz = (uint32_t)__shfl((int)cur.z, last, 64), cw = (uint32_t)__shfl((int)cur.w, last, 64);
                    uz = (uint32_t)__shfl((int)up.z, last, 64), uw = (uint32_t)__shfl((int)up.w, last, 64);
                    const uint4 left = png_and16(png_left16<BPP>(cur, lz, lw), mask);
                    const uint4 upleft = png_and16(png_left16<BPP>(up, vz, vw), mask);
                    png_costs16(cur, left, up, upleft, sum);
                }
#pragma unroll
                for (int t = 0; t < 5; t++) sum[t] = png_group_sum16(sum[t], G);
            }
            uint32_t best = 0, least = 0;
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const uint32_t s = png_group_sum64(sum[t], G);
                if (t == 0 || s < least) best = t, least = s;  // strictly smaller: the lowest type number wins a tie
            }
            if (have && q == 0) types[r] = (uint8_t)best;
        }
    }
}

}  // namespace fdh

// G = the row's chunks rounded up to a power of two, 64 at most; FDH_PNG_CHOOSE_LANES (1, 2, 4 .. 64) sets it (tests: every
// shape at every width -- narrow groups, one step per row, looped rows, and their combinations).  A wavefront takes the bands
// b, b + Y, .. of its image; Y is chosen so that a small batch of tall images still fills the GPU, FDH_PNG_CHOOSE_WAVES sets it.
extern "C" int fdh_launch_png_choose(const uint8_t* pix, const uint64_t* pix_off, uint8_t* types, const uint64_t* types_off,
                                     uint32_t* status, uint64_t n, uint32_t row_bytes, uint32_t bpp, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t chunks = (row_bytes + 15) / 16;
    uint32_t group = 1;
    while (group < fdh::kWave && group < chunks) group <<= 1;
    if (const char* e = getenv("FDH_PNG_CHOOSE_LANES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= fdh::kWave && (v & (v - 1)) == 0) group = (uint32_t)v;
    }
    uint32_t waves = (uint32_t)std::min<uint64_t>(4096, (32768 + n - 1) / n);
    if (const char* e = getenv("FDH_PNG_CHOOSE_WAVES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 65535) waves = (uint32_t)v;
    }
    const uint32_t pieces = (chunks + group - 1) / group;
    fdh::PngChooseArgs a{pix, pix_off, types, types_off, status, n, row_bytes, group, pieces};
    const dim3 block(fdh::kWave), grid((unsigned)n, waves);
#define FDH_PNG_CASE(B)                                                                           \
    case B:                                                                                       \
        if (pieces > 1) hipLaunchKernelGGL((fdh::png_choose_kernel<B, true>), grid, block, 0, stream, a); \
        else hipLaunchKernelGGL((fdh::png_choose_kernel<B, false>), grid, block, 0, stream, a);   \
        break;
    switch (bpp) {
        FDH_PNG_CASE(1)
        FDH_PNG_CASE(2)
        FDH_PNG_CASE(3)
        FDH_PNG_CASE(4)
        FDH_PNG_CASE(6)
        FDH_PNG_CASE(8)
        default: return -1;
    }
#undef FDH_PNG_CASE
    return (int)hipGetLastError();
}
