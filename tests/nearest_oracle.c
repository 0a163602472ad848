/*
 * nearest_oracle.c — K-nearest point queries (include/rt.h "K-nearest queries": rt_closest_points with the options "closest_k" and
 * "closest_all") restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, a FULL sort of the
 * candidates below R * R by (k, kind, primitive), the count rule, and "the defaults leave _reserved 0".  The checker of
 * tests/test_gpu_nearest.py and tests/test_gpu_nearest_fuzz.py, itself pinned by tests/test_nearest_cpu.py (against closest_oracle.c, a
 * float64 twin, hand-computed cases, and the one-line mutants below, each of which some case must tell from the definition).  TEST
 * INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS (tests/checker_build.py: -ffp-contract=off, so every product and
 * sum rounds on its own, as the header demands).  It includes nothing but the public header, through point_oracle.h: the vectors, the
 * keys, the records, the order of the list (`before`) and the list's driver (the argument check, the sort, the count rule, the K writes)
 * live there, shared with the other point checkers.  Here: the loop and the radius predicate.
 *
 * variant: 0 the definition;
 *          1 a non-strict radius, k <= R * R;
 *          2 a tie between triangles broken by the position in the enumeration (chunk by chunk, as listed) instead of the uploaded index;
 *          3 at equal k a triangle before a sphere;
 *          4 the count capped at K under closest_all = 1;
 *          5 a streaming list that drops a candidate whose key EQUALS the K-th key once K are in.
 */
#include "point_oracle.h"

static void record(rt_closest* o, const void* p, const cand* c, const list_scene* sc, int count)
{
    record_point(o, *(const v3*)p, c, sc->spheres, sc->tris, sc->chunk_mesh, count);
}

/* out[i * K + j] = record j of points[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).
 * totals (may be NULL): per point, the number of ALL candidates below R * R, whatever K and all are.  kth_ties (may be NULL): per point,
 * 1 when the K-th and the (K+1)-th key of the full sort are bit-equal.  -3: a chunk's range leaves the triangle buffer; -4: K or all out
 * of range; -5: out of memory. */
int np_nearest(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* points, int n, int K, int all, int variant, rt_closest* out, int32_t* totals, int32_t* kth_ties)
{
    size_t addressed;
    const int bad = list_check(mi, nm, nt, K, all, &addressed);
    if (bad) return bad;
    const list_scene scene = { spheres, tris, chunk_mesh, variant };
    const tie_order order = variant == 2 ? ORDER_TIE_BY_POSITION : variant == 3 ? ORDER_TRIANGLE_FIRST : ORDER_DEFINITION;
    /* today's call leaves _reserved 0 */
    const count_rule rule = (K == 1 && all == 0) ? COUNT_ZERO : variant == 4 ? COUNT_CAPPED : COUNT_RULE;
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[(size_t)i * K];
        list_clear(o, K, totals, kth_ties, i);
        const v3 p = ld(points[i].origin);
        const float R = points[i].tMax;
        if (!(R > 0.0f)) continue;                                  /* R <= 0 or NaN: not searched */
        const float bound = R * R;
        cand* c = (cand*)malloc(sizeof(cand) * ((size_t)ns + addressed + 1));
        if (!c) { failed = 1; continue; }
        int total = 0;
        uint32_t seq = 0;
        for (int s = 0; s < ns; s++) {
            const float k = sphere_key(p, &spheres[s]);
            if (!(variant == 1 ? k <= bound : k < bound)) continue;
            const cand e = { .k = k, .kind = RT_HIT_SPHERE, .prim = (uint32_t)s, .chunk = -1, .seq = seq++, .order = order };
            c[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                const v3 A = ld(tris[t].posA), eAB = sub(ld(tris[t].posB), A), eAC = sub(ld(tris[t].posC), A);
                float u, v;
                const float k = triangle_key(p, A, eAB, eAC, &u, &v);
                if (!(variant == 1 ? k <= bound : k < bound)) continue;
                const cand e = { .k = k, .u = u, .v = v, .kind = RT_HIT_TRIANGLE, .prim = t, .chunk = m, .seq = seq++, .order = order };
                c[total++] = e;
            }
        if (variant == 5) {
            /* the candidates in enumeration order through a sorted list of K: full, it takes only a key BELOW its last */
            int listed = 0;
            for (int a = 0; a < total; a++) {
                const cand e = c[a];
                if (listed == K && !(e.k < c[K - 1].k)) continue;
                int at = listed < K ? listed : K - 1;
                while (at > 0 && before(&e, &c[at - 1])) { c[at] = c[at - 1]; at--; }   /* (slots 0 .. K-1 of c are free: a >= listed) */
                c[at] = e;
                if (listed < K) listed++;
            }
            list_write(o, c, listed, total, K, all, rule, record, &p, &scene, totals, i);
        } else list_finish(o, c, total, K, all, rule, record, &p, &scene, totals, kth_ties, i);
        free(c);
    }
    return failed ? -5 : 0;
}
