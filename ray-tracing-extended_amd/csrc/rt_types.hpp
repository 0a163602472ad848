// rt_types.hpp — the plain structs that both a kernel header and the host's context (rt_ctx.hpp) name: no kernel, no device function.
// Each stays in the namespace of the header whose kernels read it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

namespace rtg {

struct MeshXf { float px, py, pz, qx, qy, qz, qw, sx, sy, sz; };            // rt_mesh_transform (rt_geom.hpp k_transform)

} // namespace rtg

namespace rtk {

// k_cam_stream (rt_render_params): the camera of every frame of a launch, indexed by the frame's offset in the launch.  The camera fields
// of rt_params (viewParams, camLocalToWorld, worldSpaceCameraPos) in the order the camera block reads them; the last row of the matrix is
// never read.  F.p still carries every other uniform, which all frames of the launch share.
struct CamRecord {
    float4 view;                // viewParams, -
    float4 m0, m1, m2;          // rows 0..2 of camLocalToWorld
    float4 pos;                 // worldSpaceCameraPos, -
};

} // namespace rtk

namespace rtgb {

// ---- the device builder's scratch (rt_bvh_gpu.hpp host driver) -----------------------------------------------------------------------
template <class T> struct Buf {
    T* p = nullptr; size_t cap = 0;
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = std::max<size_t>(n, 1);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Workspace {
    Buf<float> top_boxes; Buf<int32_t> top_pairs;       // the host-built top of the tree (boxes out, nodes back)
    std::vector<float> h_boxes, h_top_boxes; std::vector<int32_t> h_pairs;
    Buf<uint64_t> keys0, keys1;
    Buf<uint32_t> ids0, ids1, c0, c1, tmp, block_count, block_offset, ctr;
    Buf<unsigned char> sort_tmp;
    Buf<float4> bmin, bmax;
    Buf<int2> child;
    Buf<uint2> f0, f1;
    Buf<uint32_t> t0, t1;                               // collapse: first triangle position of each frontier entry
    Buf<int> need;
    Buf<float> area;
    void release()
    {
        keys0.release(); keys1.release(); ids0.release(); ids1.release(); c0.release(); c1.release(); tmp.release(); block_count.release();
        block_offset.release(); ctr.release(); sort_tmp.release(); bmin.release(); bmax.release(); child.release(); f0.release(); f1.release();
        need.release(); area.release(); top_boxes.release(); top_pairs.release(); t0.release(); t1.release();
    }
};

} // namespace rtgb
