// tests/bvh_dump.cpp — writes the host builder's BVH4 to a file for tests/bvh_audit.py (tests/test_bvh_audit_cpu.py compiles it with
// csrc/bvh.cpp the way test_bvh_host_cpu.py compiles bvh_check.cpp).
//   bvh_dump <tris.f32: 9 floats per triangle> <out> <collapse_dp> <max_leaf> <reinsert_passes> <origin_magnitude>
// out: uint32 n_nodes, uint32 n_order, int32 maxStack, float magnitude, then n_nodes Node4 records (128 B), then n_order uint32
#include "bvh.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
    std::vector<float> v; float x; while (fread(&x, 4, 1, f) == 1) v.push_back(x); fclose(f);
    rtbvh::Bvh b; rtbvh::Tuning t;
    t.collapse_dp = atoi(argv[3]); t.max_leaf = atoi(argv[4]); t.reinsert_passes = atoi(argv[5]);
    rtbvh::build(v.data(), 9, (uint32_t)(v.size() / 9), (float)atof(argv[6]), t, b);
    FILE* o = fopen(argv[2], "wb"); if (!o) return 4;
    const uint32_t head[2] = { (uint32_t)b.nodes.size(), (uint32_t)b.order.size() };
    const int32_t stack = b.maxStack;
    fwrite(head, 4, 2, o); fwrite(&stack, 4, 1, o); fwrite(&b.magnitude, 4, 1, o);
    if (!b.nodes.empty()) fwrite(b.nodes.data(), sizeof(rtbvh::Node4), b.nodes.size(), o);
    if (!b.order.empty()) fwrite(b.order.data(), 4, b.order.size(), o);
    fclose(o);
    return 0;
}
