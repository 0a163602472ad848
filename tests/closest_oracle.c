/*
 * closest_oracle.c — closest-point queries (include/rt.h "closest-point queries": rt_closest_points) restated in plain C as a brute-force
 * loop over every sphere and every triangle a chunk addresses: the checker of tests/test_gpu_closest.py, itself pinned by
 * tests/test_closest_cpu.py (a float64 twin, hand-computed cases).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own
 * CFLAGS (oracle/Makefile, tests/checker_build.py: -ffp-contract=off, so every product and sum below rounds on its own, as the header
 * demands).  It includes nothing but the public header, through point_oracle.h: the vectors, the two keys, the miss record and the
 * record of a candidate live there, shared with the other point checkers.  The definition is the library's own, not the shader's.
 */
#include "point_oracle.h"

/* out[i] = the closest-point record of points[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).
 * prim_tests (may be NULL): candidates examined, n * (ns + addressed triangles) for the searched points.  at_best (may be NULL): per
 * point, the candidates below R * R whose key is bit-equal to the winner's, the winner among them (0: a miss; 2 or more: the tie rule
 * decided).  -3: a chunk's range leaves the triangle buffer. */
int cp_closest(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* points, int n, rt_closest* out, uint64_t* prim_tests, int32_t* at_best)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
    uint64_t tests = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : tests)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[i];
        miss(o, 0);
        if (at_best) at_best[i] = 0;
        const v3 p = ld(points[i].origin);
        const float R = points[i].tMax;
        if (!(R > 0.0f)) continue;                                  /* R <= 0 or NaN: not searched */
        const float bound = R * R;
        /* the smallest (k, kind, primitive) with k < bound */
        int have = 0, kind = 0, chunk = -1, equal = 0;
        uint32_t prim = 0;
        float best = 0.0f, bu = 0.0f, bv = 0.0f;
        for (int s = 0; s < ns; s++) {
            const float k = sphere_key(p, &spheres[s]);
            tests++;
            if (!(k < bound)) continue;
            equal = !have || k < best ? 1 : equal + (k == best);
            if (!have || k < best) { have = 1; kind = RT_HIT_SPHERE; prim = (uint32_t)s; best = k; }
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                const v3 A = ld(tris[t].posA), eAB = sub(ld(tris[t].posB), A), eAC = sub(ld(tris[t].posC), A);
                float u, v;
                const float k = triangle_key(p, A, eAB, eAC, &u, &v);
                tests++;
                if (!(k < bound)) continue;
                equal = !have || k < best ? 1 : equal + (k == best);
                if (!have || k < best || (k == best && kind == RT_HIT_TRIANGLE && t < prim)) {
                    have = 1; kind = RT_HIT_TRIANGLE; prim = t; best = k; bu = u; bv = v; chunk = m;
                }
            }
        if (!have) continue;
        if (at_best) at_best[i] = equal;
        const cand won = { .k = best, .u = bu, .v = bv, .kind = kind, .prim = prim, .chunk = chunk };
        record_point(o, p, &won, spheres, tris, chunk_mesh, 0);
    }
    if (prim_tests) *prim_tests = tests;
    return 0;
}
