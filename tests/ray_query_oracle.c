/*
 * ray_query_oracle.c — the CPU oracle's CalculateRayCollision (RayTracing.shader:256-297) for caller-supplied rays, as rt_hit records:
 * the checker of rt_trace_rays / rt_occluded (tests/test_gpu_ray_query.py).  TEST INFRASTRUCTURE: it includes the oracle unchanged
 * and is compiled by the test with the oracle's own CFLAGS (oracle/Makefile).
 *
 * The oracle returns dst, hitPoint, normal and a material pointer.  What was hit is recovered from that pointer: a sphere's own material
 * (the sphere's index), or a chunk's (the chunk's index).  The triangle of a chunk hit is the first of that chunk, in the reference's
 * visiting order, whose RayTriangle accepts the ray at exactly that dst — the one the reference's strict '<' kept (overlapping chunk
 * ranges are refused by the library's upload, so the chunk owns it alone).
 */
#include "../oracle/rt_oracle.c"

/* hits[i] = CalculateRayCollision(rays[i]) when its dst < rays[i].tMax, else a miss (dst = +inf, indices -1, the rest 0); accel != 0:
 * triangles are found through the oracle's own search tree instead of its literal loop (the same hits, tests/test_oracle_cpu.py) */
int rq_trace(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int mode,
             const rt_ray* rays, int n, int accel, rt_hit* hits)
{
    rt_params p;
    memset(&p, 0, sizeof p);
    p.intersectMode = mode;
    scene_t sc = { &p, spheres, ns, tris, nt, mi, nm, mode, NULL };
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; i++) {
        orc_counts cnt;
        memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const hit_t h = calculate_ray_collision(&sc, o, d, &cnt);
        rt_hit* q = &hits[i];
        memset(q, 0, sizeof *q);
        q->dst = INFINITY;
        q->primitive = q->chunk = q->mesh = -1;
        if (!h.didHit || !(h.dst < r->tMax)) continue;
        q->dst = h.dst;
        q->hitPoint[0] = h.hitPoint.x; q->hitPoint[1] = h.hitPoint.y; q->hitPoint[2] = h.hitPoint.z;
        q->normal[0] = h.normal.x; q->normal[1] = h.normal.y; q->normal[2] = h.normal.z;
        const char* mat = (const char*)h.material;
        if (ns > 0 && mat >= (const char*)spheres && mat < (const char*)(spheres + ns)) {
            q->kind = RT_HIT_SPHERE;
            q->primitive = (int32_t)((mat - (const char*)spheres) / (ptrdiff_t)sizeof(rt_sphere));
            continue;
        }
        const int m = (int)((mat - (const char*)&mi[0].material) / (ptrdiff_t)sizeof(rt_meshinfo));
        q->kind = RT_HIT_TRIANGLE;
        q->chunk = m;
        for (uint32_t k = 0; k < mi[m].numTriangles; k++) {
            const uint32_t ti = mi[m].firstTriangleIndex + k;
            float dst, u, v, w;
            if (ray_triangle(o, d, &tris[ti], &dst, &u, &v, &w) && dst == h.dst) {
                q->primitive = (int32_t)ti; q->u = u; q->v = v;
                break;
            }
        }
    }
    accel_free(tree);
    (void)nt;
    return 0;
}

/* count[i] = how many candidates the literal loop could take at the bit-identical dst of rays[i]'s closest hit, the winner included: every
 * sphere RaySphere accepts and every triangle RayTriangle accepts at that dst (in FLAT_CHUNKS mode only those of chunks whose box test
 * passes) — brute force, no tree.  0 for a miss (tMax applied as rq_trace applies it).  2 or more: the tie-break decided the hit. */
int rq_candidates(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int mode,
                  const rt_ray* rays, int n, int32_t* count)
{
    rt_params p;
    memset(&p, 0, sizeof p);
    p.intersectMode = mode;
    scene_t sc = { &p, spheres, ns, tris, nt, mi, nm, mode, NULL };
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; i++) {
        orc_counts cnt;
        memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const hit_t h = calculate_ray_collision(&sc, o, d, &cnt);
        count[i] = 0;
        if (!h.didHit || !(h.dst < r->tMax)) continue;
        int32_t c = 0;
        for (int s = 0; s < ns; s++) {
            float dst;
            if (ray_sphere(o, d, v_load(spheres[s].position), spheres[s].radius, &dst) && dst == h.dst) c++;
        }
        for (int m = 0; m < nm; m++) {
            if (mode == RT_INTERSECT_FLAT_CHUNKS && !ray_bounding_box(o, d, mi[m].boundsMin, mi[m].boundsMax)) continue;
            for (uint32_t k = 0; k < mi[m].numTriangles; k++) {
                float dst, u, v, w;
                if (ray_triangle(o, d, &tris[mi[m].firstTriangleIndex + k], &dst, &u, &v, &w) && dst == h.dst) c++;
            }
        }
        count[i] = c;
    }
    (void)nt;
    return 0;
}
