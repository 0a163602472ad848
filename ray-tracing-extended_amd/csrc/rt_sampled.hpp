// rt_sampled.hpp — the sample-lane frame: what k_radiance, k_gather and k_visibility have in common.  Each is this frame plus a middle.
//
// An item (a ray or a point) of a sampled call takes N samples.  One launch per slice of items, no persistent loop.  An item's
// S = 16 / 4 / 1 sub-streams sit on S ADJACENT lanes (lane = item * S + sub-stream; a wave holds 64 / S items), lane k walks samples k,
// k + S, ... in increasing order and sums them from 0.  The loops are flat, ONE traversal site per trip, and a lane's next ray is made in
// the step that ends the one before, so lanes meet again at the traversal whatever their path lengths.  Hit or miss crosses the
// traversal as a value (h.id, any_hit's hit_t), never as a bool (rt_kernels.hpp, the per-lane walk, records why).
//
// The sums of an item's lanes meet in the estimator's tree of the Philox mode: four xor-exchanges per channel at lane distances 1, 2,
// 4, 8 (inside a row of 16 lanes: DPP moves, no LDS traffic).  Every lane of the wave takes part, lanes without an item carry zeros,
// and the sub-stream-0 lane stores root / N — or zeros for an item with tMax <= 0 or NaN, for which nothing is drawn or cast.
//
// The first load of (origin, tMax), `traced`, the key and the "next sample starts at the point again" step are written in each kernel:
// profiles/sampled_frame_notes.txt records what sharing them did to the generated code.
#pragma once
#include "rt_kernels.hpp"

namespace rtk {

// What the three kernels' Args have under one name each (rt_queries.hip fill_sampled, launch_slice).  The head ends at 32 bytes: with
// sample_lanes_log2 in it, it would be padded to 40 and every later argument would move (rt_query.hpp, QueryArgs, records what a moved
// argument cost), so each Args goes on with sample_lanes_log2 and the stack fields itself, at the offsets its kernel was measured with.
struct SampledHead {
    const float4* in;           // [n*2]  rt_ray: (origin, tMax) (direction or normal, -)
    float4* out;                // [n * the float4 per item of the family and mode]
    int n;
    int samples;                // N
    uint32_t seed;              // second key word
    uint32_t first_index;       // first key word of item 0 of this launch
};
struct ShadingHead { rt_params p; };    // the base before it where Trace runs (maxBounceCount, intersectMode, the environment): p stays first

// A lane's place in the layout.  idle_wave is wave-uniform — no lane of this wave has an item — and the kernel returns on it before
// lane_stack.  (The host keeps items-per-launch * S below 2^31.)
struct SampleLane {
    unsigned int item;          // of this launch
    int sub, nsub;              // sub-stream of S
    bool present, idle_wave;
    __device__ __forceinline__ bool stores() const { return present && sub == 0; }
};
template <class Args> __device__ __forceinline__ SampleLane sample_lane(const Args& A)
{
    const int sl = A.sample_lanes_log2;
    const unsigned int g = blockIdx.x * kBlock + threadIdx.x;
    SampleLane L;
    L.idle_wave = (g & ~63u) >> sl >= (unsigned)A.n;
    L.nsub = 1 << sl;
    L.item = g >> sl;
    L.sub = (int)(g & (unsigned)(L.nsub - 1));
    L.present = L.item < (unsigned)A.n;
    return L;
}

// The real SH basis of bands 0..2 on d, every product its own rounding (include/rt.h)
__device__ __forceinline__ void sh9_basis(const v3& d, float (&Y)[9])
{
    const float x = d.x, y = d.y, z = d.z;
    Y[0] = 0.28209479f;
    Y[1] = 0.48860251f * y;
    Y[2] = 0.48860251f * z;
    Y[3] = 0.48860251f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.54627421f * (x * x - y * y);
}

// The estimator's tree over NF channels: (k, k + 1) for even k, then (k, k + 2) for k = 0 mod 4, ...
template <int NF> __device__ __forceinline__ void tree_sum(float* total, int nsub)
{
    for (int off = 1; off < nsub; off <<= 1) {
#pragma unroll
        for (int k = 0; k < NF; ++k) total[k] = total[k] + __shfl_xor(total[k], off, 64);
    }
}

} // namespace rtk
