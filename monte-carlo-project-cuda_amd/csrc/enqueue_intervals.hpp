// enqueue_intervals.hpp — the kernel time mcamd_enqueued_kernel_ms reports for an overlapped enqueue, as
// host arithmetic over timestamps: no HIP here, so that a stand-alone program can test it without a device.
//
// An overlapped job's simulation kernel runs on one of the context's two internal streams and may start while its
// predecessor's kernel is still running on the other.  Its start-to-end interval then covers time the predecessor has
// already been charged for.  What the job is charged is the part of its interval after the predecessor's kernel ended,
//     end_N - max(start_N, end_{N-1}),
// so the times of a run of overlapped jobs are disjoint intervals inside the time the chip was busy with them.  Two
// kernels that share the chip can also end in the other order; "predecessor" is therefore taken in the order in which
// the kernels of a run ENDED, which is the order of the enqueues whenever they ended in that order.
#pragma once

#include <cstdint>

namespace mcamd::capi {

constexpr uint32_t kEnqueueRing = 64;   // enqueues whose events a context keeps (mcamd_ctx::kRing)

// What a ring slot remembers of the overlapped enqueue that last used it.  The in-order enqueue forms do not touch it:
// a slot describes call number i (0-based, in the order of the context's enqueues) only while call == i + 1.
struct OverlapSlot {
    uint64_t call = 0;      // 1 + the number of the overlapped call that last took the slot; 0: none yet
    uint8_t lane = 0;       // which internal stream (0 or 1) ran its kernel
    bool chained = false;   // the call before it was overlapped too
};

inline uint32_t ring_slot(uint64_t call)
{
    return static_cast<uint32_t>(call % kEnqueueRing);
}

// whether call number `call`, one of the last kEnqueueRing calls, was overlapped
inline bool slot_overlapped(const OverlapSlot *ring, uint64_t call)
{
    return ring[ring_slot(call)].call == call + 1;
}

// Whether call number `call` continues a run of overlapped calls: it and the call before it were overlapped, and that
// call's events are still among the last kEnqueueRing of the n_enqueued calls so far.
inline bool continues_run(const OverlapSlot *ring, uint64_t call, uint64_t n_enqueued)
{
    if (call == 0 || call >= n_enqueued || !slot_overlapped(ring, call) || !ring[ring_slot(call)].chained) return false;
    return n_enqueued - (call - 1) <= kEnqueueRing && slot_overlapped(ring, call - 1);
}

// The part of [start, end] after pred_end, all on one clock in ms; with has_pred false, the whole interval.  Never
// negative: a job whose kernel ended before its predecessor's is charged nothing.
inline double exclusive_ms(double start, double end, bool has_pred, double pred_end)
{
    const double from = has_pred && pred_end > start ? pred_end : start;
    return end > from ? end - from : 0.0;
}

// The times of a run of n <= kEnqueueRing overlapped jobs from their kernels' intervals [start[i], end[i]] on one clock:
// taken in the order in which the kernels ended (ties: in the order of the enqueues), each is charged the part of its
// interval after the end of the one before it; the first, its whole interval.
inline void exclusive_run_ms(const double *start, const double *end, uint32_t n, double *ms)
{
    uint32_t order[kEnqueueRing];
    if (n > kEnqueueRing) n = kEnqueueRing;
    for (uint32_t i = 0; i < n; ++i) {   // insertion sort, stable: a run that ended in order costs n comparisons
        uint32_t k = i;
        for (; k > 0 && end[order[k - 1]] > end[i]; --k) order[k] = order[k - 1];
        order[k] = i;
    }
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = order[k];
        ms[i] = exclusive_ms(start[i], end[i], k > 0, k > 0 ? end[order[k - 1]] : 0.0);
    }
}

}  // namespace mcamd::capi
