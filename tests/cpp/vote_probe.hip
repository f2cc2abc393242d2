// vote_probe.hip -- the walk-shaped loop of tests/test_vote_lowering.py: a conjunction vote, a loop-carried lane mask and a per-lane update
// under a mask, written with the vote helpers of sr_device.h (probe_masks) and, as the control, with the bool idiom they replace
// (probe_bools).  The test compiles this file to gfx950 assembly and looks at the two kernels' loops; nothing here is ever launched.
#include "sr_device.h"

using namespace sr;

extern "C" __global__ __launch_bounds__(64) void probe_masks(const float* __restrict__ in, float* __restrict__ out, int steps) {
    const int lane = threadIdx.x;
    float acc = in[lane];
    int count = 0;
    lanemask done_m = ~vote(acc >= 0.0f);
    for (int i = 0; i < steps; ++i) {
        const float v = in[64 * (i + 1) + lane];
        // !(v < acc - 4): the comparison is balloted as written and the mask complemented (NaN keeps the lane)
        const lanemask m = vote(v > 0.5f) & vote(v < acc + 2.0f) & ~vote(v < acc - 4.0f) & ~done_m;
        if (m == 0ull) continue;
        const lanemask room_m = vote(count < 7);
        if (lane_of(m & room_m)) out[64 * count + lane] = v;
        count += lane_of(m & room_m) ? 1 : 0;
        acc = lane_of(m) ? acc + v : acc;
        done_m |= vote(acc > 10.0f) | (m & ~room_m);
        if (~done_m == 0ull) break;
    }
    out[64 * 8 + lane] = acc + (float)count + (lane_of(done_m) ? 1.0f : 0.0f);
}

extern "C" __global__ __launch_bounds__(64) void probe_bools(const float* __restrict__ in, float* __restrict__ out, int steps) {
    const int lane = threadIdx.x;
    float acc = in[lane];
    int count = 0;
    bool done = !(acc >= 0.0f);
    for (int i = 0; i < steps; ++i) {
        const float v = in[64 * (i + 1) + lane];
        const bool h = v > 0.5f && v < acc + 2.0f && !(v < acc - 4.0f) && !done;
        if (__ballot(h) == 0ull) continue;
        const bool room = count < 7;
        if (h && room) out[64 * count + lane] = v;
        count += (h && room) ? 1 : 0;
        acc = h ? acc + v : acc;
        done = done || acc > 10.0f || (h && !room);
        if (__ballot(!done) == 0ull) break;
    }
    out[64 * 8 + lane] = acc + (float)count + (done ? 1.0f : 0.0f);
}
