// batch_lanes.h -- which chain stream (lane) a new batch takes.  Pure host code: no HIP, no state of its own (api_batch.hip keeps the
// pool; scripts/native/batch_lane_policy.cpp and tests/test_batch_lane_policy.py drive the rule on the CPU).
//
// The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES in-order hardware queues by its own bookkeeping, and
// two batch chains that land on one queue serialise.  With more batches than queues sharing is unavoidable; what can be chosen is
// that it is EVEN.  So the library makes L = min(hardware queues, MAX_LANES) streams per device once, together, and hands them to
// the batches: a new batch takes the lowest-numbered lane with the fewest batches.  Without destructions batch i gets lane i mod L;
// eight batches at four queues are two per lane, at sixteen queues one per lane.
#ifndef VP8HIP_BATCH_LANES_H
#define VP8HIP_BATCH_LANES_H

namespace vp8 {

constexpr int MAX_LANES = 8;

inline int lane_count(int hw_queues) { return hw_queues < 1 ? 1 : hw_queues < MAX_LANES ? hw_queues : MAX_LANES; }

// load[l] = batches on lane l.  The lowest-numbered lane with the fewest batches (-1: no lanes).
inline int pick_lane(const int *load, int lanes) {
    int best = -1;
    for (int l = 0; l < lanes; ++l)
        if (best < 0 || load[l] < load[best]) best = l;
    return best;
}

}  // namespace vp8
#endif
