// Stand-alone check of csrc/enqueue_intervals.hpp (no HIP): the time an overlapped enqueue is charged, and the ring
// bookkeeping that decides whether a job's interval is cut at its predecessor's end.  Prints one JSON line; exit
// status 1 if a case failed.  Built by tests/test_enqueue_intervals_cpu.py under the host sanitizers.
#include "enqueue_intervals.hpp"

#include <cstdio>
#include <vector>

using namespace mcamd::capi;

namespace {

int failures = 0, cases = 0;

void expect(bool ok, const char *what)
{
    ++cases;
    if (!ok) {
        ++failures;
        std::fprintf(stderr, "FAILED: %s\n", what);
    }
}

// A context's ring as capi.cpp keeps it, with the timestamps the events would hold.
struct Ring {
    OverlapSlot slot[kEnqueueRing];
    double start[kEnqueueRing] = {}, end[kEnqueueRing] = {};
    uint64_t n_enqueued = 0;

    void enqueue(bool overlapped, double s, double e)
    {
        const uint32_t k = ring_slot(n_enqueued);
        start[k] = s;
        end[k] = e;
        if (overlapped) {   // overlap_finish; an in-order enqueue leaves the slot's record alone
            slot[k].chained = n_enqueued > 0 && slot_overlapped(slot, n_enqueued - 1);
            slot[k].call = n_enqueued + 1;
            slot[k].lane = static_cast<uint8_t>(n_enqueued % 2);
        }
        ++n_enqueued;
    }
    // mcamd_enqueued_kernel_ms for one call: its own interval, or its share of the run of overlapped calls it is in
    double ms(uint64_t call) const
    {
        uint64_t b = call, e = call + 1;
        while (continues_run(slot, b, n_enqueued)) --b;
        while (continues_run(slot, e, n_enqueued)) ++e;
        if (e - b < 2) return end[ring_slot(call)] - start[ring_slot(call)];
        double s[kEnqueueRing], t[kEnqueueRing], charged[kEnqueueRing];
        for (uint64_t c = b; c < e; ++c) {
            s[c - b] = start[ring_slot(c)];
            t[c - b] = end[ring_slot(c)];
        }
        exclusive_run_ms(s, t, static_cast<uint32_t>(e - b), charged);
        return charged[call - b];
    }
};

}  // namespace

int main()
{
    // the arithmetic
    expect(exclusive_ms(10.0, 13.0, true, 9.0) == 3.0, "predecessor ended before the start: the whole interval");
    expect(exclusive_ms(10.0, 13.0, true, 10.0) == 3.0, "predecessor ended at the start");
    expect(exclusive_ms(10.0, 13.0, true, 11.5) == 1.5, "predecessor ended inside: the part after it");
    expect(exclusive_ms(10.0, 13.0, true, 13.0) == 0.0, "predecessor ended at the end: nothing");
    expect(exclusive_ms(10.0, 13.0, true, 14.0) == 0.0, "predecessor ended after the end: 0, not negative");
    expect(exclusive_ms(10.0, 13.0, false, 11.5) == 3.0, "no predecessor: the whole interval, pred_end unread");
    expect(exclusive_ms(0.0, 2.5, true, -0.25) == 2.5, "clock at the job's own start: a negative predecessor end");
    expect(exclusive_ms(0.0, 2.5, true, 0.75) == 1.75, "clock at the job's own start: a predecessor end inside");
    expect(exclusive_ms(5.0, 5.0, false, 0.0) == 0.0, "an empty interval");

    // a run of overlapped jobs: kernels of 3 ms that start 0.5 ms before the one before ends
    {
        Ring r;
        double t = 0.0, busy_from = 0.0;
        for (int i = 0; i < 10; ++i) {
            r.enqueue(true, t, t + 3.0);
            t += 2.5;
        }
        double sum = 0.0;
        for (uint64_t c = 0; c < 10; ++c) sum += r.ms(c);
        expect(r.ms(0) == 3.0, "the first of a run has no predecessor");
        expect(r.ms(1) == 2.5 && r.ms(9) == 2.5, "a later one is charged from its predecessor's end");
        expect(sum == (t - 2.5 + 3.0) - busy_from, "disjoint intervals add up to the busy time");
        expect(!r.slot[ring_slot(0)].chained && r.slot[ring_slot(1)].chained, "chained marks");
        expect(r.slot[0].lane == 0 && r.slot[1].lane == 1 && r.slot[2].lane == 0, "lanes alternate");
    }

    // an in-order call between overlapped ones breaks the chain on both sides of it
    {
        Ring r;
        r.enqueue(true, 0.0, 3.0);
        r.enqueue(false, 3.1, 3.2);   // its kernel's own interval, on the caller's stream
        r.enqueue(true, 2.0, 6.0);    // started before the in-order call: still charged whole
        r.enqueue(true, 5.0, 9.0);
        expect(r.ms(1) == 3.2 - 3.1, "an in-order call keeps its own interval");
        expect(r.ms(2) == 4.0, "overlapped after in-order: no predecessor");
        expect(r.ms(3) == 3.0, "overlapped after overlapped: cut");
        expect(!continues_run(r.slot, 1, r.n_enqueued), "in-order call is not cut");
    }

    // the ring wraps at 64: an in-order call that takes over an overlapped call's slot must not read as overlapped,
    // and the oldest kept call has lost its predecessor's events
    {
        Ring r;
        for (int i = 0; i < 64; ++i) r.enqueue(true, 2.0 * i, 2.0 * i + 3.0);
        expect(continues_run(r.slot, 1, r.n_enqueued), "call 1 of 64: predecessor 0 still kept");
        expect(r.ms(1) == 2.0, "call 1 of 64");
        r.enqueue(false, 200.0, 201.0);   // call 64 takes slot 0 from call 0
        expect(ring_slot(64) == 0, "slot of call 64");
        expect(!slot_overlapped(r.slot, 64), "call 64 is in-order although slot 0 last held an overlapped call");
        expect(!continues_run(r.slot, 1, r.n_enqueued), "call 1 of 65: predecessor 0 is gone from the ring");
        expect(r.ms(1) == 3.0, "call 1 of 65 is charged whole: end[slot 0] now belongs to call 64");
        expect(r.ms(2) == 2.0, "call 2 of 65 still cut at call 1");
        expect(r.ms(64) == 1.0, "call 64 keeps its own interval");
        r.enqueue(true, 201.0, 204.0);    // call 65 takes slot 1; its predecessor was in-order
        expect(slot_overlapped(r.slot, 65) && !r.slot[1].chained, "call 65 overlapped, not chained");
        expect(r.ms(65) == 3.0, "call 65 is charged whole");
        r.enqueue(true, 203.0, 206.5);    // call 66, slot 2
        expect(r.ms(66) == 2.5, "call 66 cut at call 65, across slots 1 and 2");
        for (int i = 0; i < 62; ++i) r.enqueue(true, 300.0 + 2.0 * i, 300.0 + 2.0 * i + 3.0);   // calls 67 .. 128
        expect(r.n_enqueued == 129 && ring_slot(128) == 0, "second wrap");
        expect(continues_run(r.slot, 128, r.n_enqueued) && r.ms(128) == 2.0, "call 128 in slot 0, cut at call 127 in slot 63");
        expect(!continues_run(r.slot, 65, r.n_enqueued) && continues_run(r.slot, 66, r.n_enqueued),
               "the oldest kept call is 65");
        expect(!continues_run(r.slot, 129, r.n_enqueued), "a call not yet enqueued");
        expect(!continues_run(r.slot, 0, r.n_enqueued), "call 0 has no predecessor");
    }

    // kernels that share the chip can end in the other order: the charge follows the order of the ends
    {
        const double s[4] = {0.0, 1.0, 8.5, 9.0}, t[4] = {10.0, 8.0, 15.0, 12.0};
        double ms[4];
        exclusive_run_ms(s, t, 4, ms);
        expect(ms[1] == 7.0, "the first to end is charged its whole interval");
        expect(ms[0] == 2.0, "its predecessor by enqueue, which ended after it: from that end on");
        expect(ms[3] == 2.0 && ms[2] == 3.0, "and so on in end order");
        expect(ms[0] > 0 && ms[1] > 0 && ms[2] > 0 && ms[3] > 0, "distinct ends: every job is charged something");
        expect(ms[0] + ms[1] + ms[2] + ms[3] <= 15.0, "disjoint: no more than first start to last end");
        const double s2[3] = {0.0, 0.1, 0.2}, t2[3] = {5.0, 5.0, 5.0};
        exclusive_run_ms(s2, t2, 3, ms);
        expect(ms[0] == 5.0 && ms[1] == 0.0 && ms[2] == 0.0, "equal ends keep the order of the enqueues");
        const double s1[1] = {3.0}, t1[1] = {4.5};
        exclusive_run_ms(s1, t1, 1, ms);
        expect(ms[0] == 1.5, "a run of one");
        Ring r;
        r.enqueue(true, 0.0, 0.31);
        r.enqueue(true, 0.01, 0.16);    // started later, ended first
        r.enqueue(false, 1.0, 1.25);
        expect(r.ms(0) == 0.31 - 0.16 && r.ms(1) == 0.16 - 0.01 && r.ms(2) == 0.25, "through the ring");
    }

    // a heap copy of the ring read through the same functions (what the sanitizers watch: no read past 64 slots)
    {
        std::vector<OverlapSlot> ring(kEnqueueRing);
        for (uint64_t c = 0; c < 1000; ++c) {
            ring[ring_slot(c)].chained = c > 0 && slot_overlapped(ring.data(), c - 1);
            ring[ring_slot(c)].call = c + 1;
            expect(continues_run(ring.data(), c, c + 1) == (c > 0), "every call of a long run but the first is cut");
        }
        expect(!continues_run(ring.data(), ~0ull, ~0ull), "the largest call number");
    }

    std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
    return failures ? 1 : 0;
}
