// inflate_launch.h -- what the decode launcher (inflate.hip, fdh_launch_inflate) stands on, host side only: the
// per-device state, the grid sizes, the scratch of a call, the fork / join of the side stream and launch().
// Included by inflate.hip behind its kernels (it needs their constants and nothing else of them).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include "../../include/fdeflate_hip.h"

namespace fdh {
struct CanonTables;
}

// What the landing decoder leaves over, as the kernels report it (g_tail_report): while the reports say "next to nothing"
// the call launches ONE kernel behind the landing decoder (the exact kernel, which takes any stream) instead of five (the
// interval, segment and tile decoders and the two exact kernels: each launch costs ~10 us of the chain when its list is
// empty -- 60 us of a 2.6 ms call).  The latest report decides: more than kTailFew streams left over, the long chain.
// A hint only: every stream is decoded either way, a wrong guess costs time (the exact kernel is slow).
struct TailHint {
    volatile uint32_t* rep = nullptr;  // mapped host memory
    uint32_t seen = 0;                 // rep[1] at the last look
    uint32_t seen_others = 0;          // rep[3]
    int streak = 0;
    bool short_chain = false;
    bool order_once = false;           // stream_order_kernel in one launch: the other list in no order (it has been next to empty)
    bool tried = false;
};
constexpr uint32_t kTailFew = 16;

// What the library keeps per device, under one mutex.
struct DeviceState {
    fdh::CanonTables* canon = nullptr;    // device address of g_canon, looked up by fdh_launch_canon_build (the lookup
                                          // synchronises, so it must stay off the launch path)
    uint32_t* span_pool = nullptr;        // scratch of the span decoder (never freed)
    int cus = 0;                          // compute units (0 = not asked yet)
    hipStream_t side = nullptr;           // the stream the LZ-window kernel runs on beside the canonical kernels
    hipMemPool_t scratch_pool = nullptr;  // where the calls' scratch comes from (scratch_alloc)
    TailHint tail;
};
constexpr int kMaxDevices = 64;
static DeviceState g_dev[kMaxDevices];
static std::mutex g_dev_mutex;  // guards g_dev
static int ordinal_of(const DeviceState& ds) { return (int)(&ds - g_dev); }

// The state of the calling thread's current device.
static hipError_t current_device(DeviceState** ds) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    *ds = &g_dev[dev];
    return hipSuccess;
}

// What a decode call reads of it, in one go.  `want_side`: the side stream too (created at its first use, and only
// on a device whose tables are there).
struct DeviceView {
    const fdh::CanonTables* canon;
    int cus;
    hipStream_t side;
};
static DeviceView device_view(DeviceState& ds, bool want_side) {
    std::lock_guard<std::mutex> lock(g_dev_mutex);
    if (ds.cus == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ordinal_of(ds)) != hipSuccess || v <= 0) v = 256;
        ds.cus = v;
    }
    want_side = want_side && ds.canon;
    if (want_side && !ds.side) {
        hipStream_t s2 = nullptr;
        if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess) ds.side = s2;
        else (void)hipGetLastError();
    }
    return DeviceView{ds.canon, ds.cus, want_side ? ds.side : nullptr};
}

// TailHint, read where the call is about to choose.  One launch of stream_order_kernel or two: the other list's long
// streams first takes a launch of its own for the short ones (~12 us of the chain in front of the landing decoder, spent
// in vain while that list is as good as empty -- the LZ-window kernel reports its count like the kernel behind the
// landing decoder does).
static bool hint_order_once(DeviceState& ds) {
    std::lock_guard<std::mutex> lock(g_dev_mutex);
    TailHint& h = ds.tail;
    if (!h.rep) return false;
    const uint32_t seq = h.rep[3], others = h.rep[2];
    if (seq != h.seen_others) {
        h.seen_others = seq;
        h.order_once = others <= kTailFew;
    }
    return h.order_once;
}
// ... and how many streams the landing decoder has been leaving over lately.  `report`: there is somewhere to report to.
static bool hint_short_chain(DeviceState& ds, bool* report) {
    std::lock_guard<std::mutex> lock(g_dev_mutex);
    TailHint& h = ds.tail;
    *report = h.rep != nullptr;
    if (!h.rep) return false;
    const uint32_t seq = h.rep[1], left = h.rep[0];
    if (seq != h.seen) {  // (a caller that enqueues calls faster than they run sees few reports: the latest one decides)
        h.seen = seq;
        h.streak = left > kTailFew ? 0 : h.streak + 1;
        h.short_chain = left <= kTailFew;
    }
    return h.short_chain;
}

// FDH_FLAG_SPANS: scratch of the span decoder, allocated once per device (synchronising), zero-initialised.
// nullptr: no scratch, the general kernel runs without spans.
static uint32_t* span_pool(DeviceState& ds) {
    std::lock_guard<std::mutex> lock(g_dev_mutex);
    if (!ds.span_pool) {
        const size_t bytes = ((size_t)fdh::kSpanSlots + (size_t)fdh::kSpanSlots * 2 * fdh::kSpanMaxMatches) * sizeof(uint32_t);
        uint32_t* p = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&p), bytes) == hipSuccess) {
            if (hipMemset(p, 0, fdh::kSpanSlots * sizeof(uint32_t)) == hipSuccess && hipDeviceSynchronize() == hipSuccess) ds.span_pool = p;
            else (void)hipFree(p);
        } else {
            (void)hipGetLastError();
        }
    }
    return ds.span_pool;
}

// Scratch of a call (lists, check points, records): stream-ordered allocations from a pool of the library's own that
// KEEPS what is freed (release threshold = everything).  With the device's default pool -- which hands its memory back
// at every synchronisation -- a call that followed a hipStreamSynchronize got fresh pages, and about one such call in
// ten then read ZEROS where the first kernel of the call had just written (seen on the record resume_prepare_kernel
// leaves for the kernels behind it: status "taken up at a resume point", record all zero).  Until round 5 that only
// cost time -- a stream without a record is decoded from its first byte -- and went unnoticed; with the streaming
// object's moved buffers (stream_decompressor.cpp) it decoded garbage.  Memory that stays mapped does not do it
// (tools/streamtime.py, 16 runs of ~130 calls each: 0 failures against 6 in 8), and a call no longer pays for mapping
// and unmapping its scratch.
static hipError_t scratch_alloc(DeviceState& ds, void** p, size_t bytes, hipStream_t stream) {
    hipMemPool_t pool = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_dev_mutex);
        if (!ds.scratch_pool) {
            hipMemPoolProps props = {};
            props.allocType = hipMemAllocationTypePinned;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = ordinal_of(ds);
            hipMemPool_t q = nullptr;
            const hipError_t ce = hipMemPoolCreate(&q, &props);
            if (ce != hipSuccess || !q) {  // (no fall-back to the default pool: that is the pool the zeros came from)
                (void)hipGetLastError();
                return ce != hipSuccess ? ce : hipErrorOutOfMemory;
            }
            uint64_t keep = ~0ull;
            const hipError_t se = hipMemPoolSetAttribute(q, hipMemPoolAttrReleaseThreshold, &keep);
            if (se != hipSuccess) {
                (void)hipGetLastError();
                (void)hipMemPoolDestroy(q);
                return se;
            }
            ds.scratch_pool = q;
        }
        pool = ds.scratch_pool;
    }
    return hipMallocFromPoolAsync(p, bytes, pool, stream);
}

// Grid sizes, each rule once.
static unsigned lz_blocks(uint64_t n, int cus) {  // LZ-window kernel: persistent wavefronts, FDH_LZ_WAVES_PER_CU per CU
    return (unsigned)std::min<uint64_t>(n, (uint64_t)FDH_LZ_WAVES_PER_CU * cus);
}
static unsigned s2_blocks(uint64_t n, int cus) {  // landing / interval kernel: one workgroup per CU at most
    return std::min((unsigned)((n + fdh::kS2Waves - 1) / fdh::kS2Waves), (unsigned)cus);
}
static unsigned segment_blocks(uint64_t n, int cus, bool lists) {
    const unsigned blocks = (unsigned)((n + fdh::kSegWaves - 1) / fdh::kSegWaves);
    return lists ? std::min(blocks, (unsigned)(2 * cus)) : blocks;  // persistent wavefronts: two workgroups (80 KiB of LDS each) per CU
}
static unsigned canon_blocks(uint64_t n) { return (unsigned)((n + fdh::kCanonWaves - 1) / fdh::kCanonWaves); }
// the exact kernels on a list: a grid-stride loop over persistent workgroups (16 per CU at most), so a batch that is
// all canonical costs two near-empty launches
static unsigned exact_blocks(uint64_t n) { return (unsigned)std::min<uint64_t>(n, 4096); }

// Which kernels a call with lists runs.
struct ChainPlan {
    bool seg2;     // the interval kernel in front of the segment kernel
    bool seg3;     // the landing decoder in front of the interval kernel
    bool ordered;  // stream_order_kernel in front of both: every wavefront gets several streams
    bool overlap;  // ... and the LZ-window kernel takes the streams it sorts out on the side stream
};

// The stream-ordered scratch of one call, laid out once and handed out by name; freed on the call's stream when
// the call returns.  Layout of the decode chains, in words:
//   first list | 8 words: counters of stream_order_kernel (4 classes, [4] the LZ-window kernel's hand-out) | second list
//   | order (2 n, `ordered`) | landing decoder's list (`seg3`) | what the canonical kernels leave, what the LZ-window
//   kernel leaves (`overlap`) | 16-byte aligned: the interval kernel's check points | the LZ-window kernel's items |
//   the resume records (where a kernel leaves a stream for the kernels behind it).
// A list is n + 4 words: [0] = count, [1..3] = hand-out counters, [4..] = ids.
class CallScratch {
public:
    CallScratch(uint64_t n, uint32_t flags, int cus, const ChainPlan& p, hipStream_t stream) : stream_(stream) {
        const size_t list = (size_t)(n + 4);
        first_at_ = 0;
        counters_at_ = list;
        lz_counter_at_ = counters_at_ + 4;  // (a spare word of stream_order_kernel's counters)
        second_at_ = counters_at_ + 8;
        order_at_ = second_at_ + list;
        landing_at_ = order_at_ + (p.ordered ? (size_t)(2 * n) : 0);
        canon_left_at_ = landing_at_ + (p.seg3 ? list : 0);
        lz_left_at_ = canon_left_at_ + (p.overlap ? list : 0);
        words_ = (lz_left_at_ + (p.overlap ? list : 0) + 3) & ~(size_t)3;
        ckpt_bytes_ = p.seg2 ? (size_t)s2_blocks(n, cus) * fdh::kS2Waves * fdh::kS2CkptPerWave * sizeof(uint2) : 0;
        lzck_bytes_ = (flags & FDH_FLAG_NO_LZ) ? 0 : lz_items_bytes(n, cus);
        resume_bytes_ = (size_t)n * sizeof(uint4);
    }
    // The chain of FDH_FLAG_RESUME_IN: 4 words ([2] the LZ-window kernel's hand-out) | the list of all streams
    // | its items | the records the two kernels pass between them.
    struct ResumeIn {};
    CallScratch(ResumeIn, uint64_t n, int cus, hipStream_t stream) : stream_(stream) {
        first_at_ = 4;
        lz_counter_at_ = 2;
        words_ = ((size_t)n + 8 + 3) & ~(size_t)3;
        lzck_bytes_ = lz_items_bytes(n, cus);
        resume_bytes_ = (size_t)n * sizeof(uint4);
    }
    ~CallScratch() {
        if (base_) (void)hipFreeAsync(base_, stream_);
    }
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;

    hipError_t alloc(DeviceState& ds) {
        const hipError_t e = scratch_alloc(ds, reinterpret_cast<void**>(&base_), words_ * sizeof(uint32_t) + ckpt_bytes_ + lzck_bytes_ + resume_bytes_, stream_);
        if (e != hipSuccess) base_ = nullptr;
        return e;
    }
    // The headers of the lists and the counters between them.  `whole`: one fill over the list words is cheaper than
    // three small ones (a fill is a kernel of its own on the stream); else the first header, then the counters and the
    // second header.
    hipError_t clear_headers(bool whole) {
        if (whole) return hipMemsetAsync(base_, 0, words_ * sizeof(uint32_t), stream_);
        const hipError_t e = hipMemsetAsync(base_, 0, 4 * sizeof(uint32_t), stream_);
        return e != hipSuccess ? e : hipMemsetAsync(base_ + counters_at_, 0, 12 * sizeof(uint32_t), stream_);
    }

    uint32_t* base() const { return base_; }
    uint32_t* first_list() const { return base_ + first_at_; }
    uint32_t* order_counters() const { return base_ + counters_at_; }
    uint32_t* lz_counter() const { return base_ + lz_counter_at_; }
    uint32_t* second_list() const { return base_ + second_at_; }
    uint32_t* order() const { return base_ + order_at_; }
    uint32_t* landing_list() const { return base_ + landing_at_; }
    uint32_t* canon_left() const { return base_ + canon_left_at_; }
    uint32_t* lz_left() const { return base_ + lz_left_at_; }
    uint2* checkpoints() const { return reinterpret_cast<uint2*>(bytes_at(0)); }
    uint2* lz_items() const { return reinterpret_cast<uint2*>(bytes_at(ckpt_bytes_)); }
    uint4* resume() const { return reinterpret_cast<uint4*>(bytes_at(ckpt_bytes_ + lzck_bytes_)); }

private:
    static size_t lz_items_bytes(uint64_t n, int cus) { return (size_t)lz_blocks(n, cus) * fdh::kWave * fdh::kLzMaxPhases * sizeof(uint2); }
    uint8_t* bytes_at(size_t behind_the_lists) const { return reinterpret_cast<uint8_t*>(base_ + words_) + behind_the_lists; }

    uint32_t* base_ = nullptr;
    hipStream_t stream_;
    size_t first_at_ = 0, counters_at_ = 0, lz_counter_at_ = 0, second_at_ = 0, order_at_ = 0, landing_at_ = 0, canon_left_at_ = 0, lz_left_at_ = 0;
    size_t words_ = 0, ckpt_bytes_ = 0, lzck_bytes_ = 0, resume_bytes_ = 0;
};

// The side stream beside the caller's: fork, work, join.  However the call ends, the caller's stream has waited for
// what the side stream was given before the scratch goes (or, where nothing can be waited for, the host has), and the
// events are gone.  To be declared behind the CallScratch, so that it is torn down first.
class SideFork {
public:
    SideFork(hipStream_t main, hipStream_t side) : main_(main), side_(side) {}
    ~SideFork() {
        if (pending_) (void)hipStreamWaitEvent(main_, join_, 0);
        if (sync_) (void)hipStreamSynchronize(side_);
        const hipEvent_t events[2] = {fork_, join_};
        for (hipEvent_t ev : events)
            if (ev) (void)hipEventDestroy(ev);
    }
    SideFork(const SideFork&) = delete;
    SideFork& operator=(const SideFork&) = delete;

    hipError_t fork() {  // the side stream goes on from where the caller's stream is now
        hipError_t e = hipEventCreateWithFlags(&fork_, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&join_, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(fork_, main_);
        if (e == hipSuccess) e = hipStreamWaitEvent(side_, fork_, 0);
        return e;
    }
    hipError_t record_join() {  // behind the last launch on the side stream
        const hipError_t e = hipEventRecord(join_, side_);
        pending_ = e == hipSuccess;
        return e;
    }
    hipError_t join() {  // the caller's stream goes on when the side stream has got there
        pending_ = false;
        return hipStreamWaitEvent(main_, join_, 0);
    }
    void sync_side_at_exit() { sync_ = true; }  // (the scratch is about to go and an event cannot be relied on)

private:
    hipStream_t main_, side_;
    hipEvent_t fork_ = nullptr, join_ = nullptr;
    bool pending_ = false, sync_ = false;
};

template <typename Kernel, typename... Args>
static hipError_t launch(Kernel kernel, unsigned grid, unsigned block, hipStream_t stream, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, args...);
    return hipGetLastError();
}
