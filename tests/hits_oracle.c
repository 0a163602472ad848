/*
 * hits_oracle.c — multi-hit ray queries (include/rt.h "multi-hit ray queries": rt_trace_hits) restated in plain C as brute force: per ray
 * the oracle's own ray_sphere and ray_triangle over every sphere and every chunk's triangles, the FLAT_CHUNKS rule with the oracle's
 * ray_bounding_box, the back-face and exit-root rules of the header restated with the oracle's v_dot / v_cross, every accepted hit
 * collected, sorted by (dst, kind, primitive, side) and cut at K.  No tree of any kind.  The checker of tests/test_gpu_hits.py, itself
 * pinned by tests/test_hits_cpu.py (hand-computed cases, a float64 twin, rq_trace at K = 1).  TEST INFRASTRUCTURE: it includes the
 * oracle unchanged and is compiled by the tests with the oracle's own CFLAGS (oracle/Makefile, tests/checker_build.py).
 */
#include "../oracle/rt_oracle.c"

typedef struct { float dst, u, v; int32_t kind, prim, chunk, side; } mh_cand;

/* ascending (dst, kind, primitive, side): dst as a float (-0.0f == 0.0f), front (+1) before back (-1) */
static int mh_before(const void* pa, const void* pb)
{
    const mh_cand* a = pa; const mh_cand* b = pb;
    if (a->dst < b->dst) return -1;
    if (a->dst > b->dst) return 1;
    if (a->kind != b->kind) return a->kind < b->kind ? -1 : 1;
    if (a->prim != b->prim) return a->prim < b->prim ? -1 : 1;
    if (a->side != b->side) return a->side > b->side ? -1 : 1;
    return 0;
}

/* the exit root of RaySphere's quadratic: its own a, b, c, disc, the other sign of the square root */
static int sphere_exit(v3 o, v3 d, v3 centre, float radius, float* dst_out)
{
    v3 oc = v_sub(o, centre);
    float a = v_dot(d, d);
    float b = 2.0f * v_dot(oc, d);
    float c = v_dot(oc, oc) - radius * radius;
    float disc = b * b - 4.0f * a * c;
    if (disc >= 0.0f) {
        float dst = (-b + sqrtf(disc)) / (2.0f * a);
        if (dst >= 0.0f) { *dst_out = dst; return 1; }
    }
    return 0;
}

/* the back face: ray_triangle's dst, u, v, w (it returns them whatever its verdict) under the mirrored determinant test */
static int triangle_back(v3 d, const rt_triangle* t, float dst, float u, float v, float w)
{
    const v3 A = v_load(t->posA);
    const v3 n = v_cross(v_sub(v_load(t->posB), A), v_sub(v_load(t->posC), A));
    const float det = -v_dot(d, n);
    return det <= -1e-6f && dst >= 0.0f && u >= 0.0f && v >= 0.0f && w >= 0.0f;
}

/* every accepted hit of one ray with dst < tMax, unsorted; returns their number (list holds 2 * ns + the addressed triangles) */
static int mh_collect(const rt_sphere* spheres, int ns, const rt_triangle* tris, const rt_meshinfo* mi, int nm, int intersect, int both,
                      const rt_ray* r, mh_cand* list)
{
    int total = 0;
    if (!(r->tMax > 0.0f)) return 0;                                /* tMax <= 0 or NaN: nothing is traced */
    const v3 o = v_load(r->origin), d = v_load(r->direction);
    for (int s = 0; s < ns; s++) {
        float dst;
        const v3 c = v_load(spheres[s].position);
        if (ray_sphere(o, d, c, spheres[s].radius, &dst) && dst < r->tMax) {
            const mh_cand e = { dst, 0.0f, 0.0f, RT_HIT_SPHERE, s, -1, 1 };
            list[total++] = e;
        }
        if (both && sphere_exit(o, d, c, spheres[s].radius, &dst) && dst < r->tMax) {
            const mh_cand e = { dst, 0.0f, 0.0f, RT_HIT_SPHERE, s, -1, -1 };
            list[total++] = e;
        }
    }
    for (int m = 0; m < nm; m++) {
        if (intersect == RT_INTERSECT_FLAT_CHUNKS && !ray_bounding_box(o, d, mi[m].boundsMin, mi[m].boundsMax)) continue;
        for (uint32_t k = 0; k < mi[m].numTriangles; k++) {
            const uint32_t ti = mi[m].firstTriangleIndex + k;
            float dst, u, v, w;
            int side = ray_triangle(o, d, &tris[ti], &dst, &u, &v, &w) ? 1 : 0;
            if (!side && both && triangle_back(d, &tris[ti], dst, u, v, w)) side = -1;
            if (side && dst < r->tMax) {
                const mh_cand e = { dst, u, v, RT_HIT_TRIANGLE, (int32_t)ti, m, side };
                list[total++] = e;
            }
        }
    }
    return total;
}

static void mh_empty(rt_multihit* o, int hit_count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->hitCount = hit_count;
}

static void mh_fill(rt_multihit* o, const mh_cand* e, const rt_sphere* spheres, const rt_triangle* tris, const int32_t* chunk_mesh,
                    const rt_ray* r, int hit_count)
{
    mh_empty(o, hit_count);
    const v3 org = v_load(r->origin), d = v_load(r->direction);
    const v3 hp = v_add(org, v_scale(d, e->dst));
    v3 nn;
    if (e->kind == RT_HIT_SPHERE) {
        nn = v_normalize(v_sub(hp, v_load(spheres[e->prim].position)));
    } else {
        const rt_triangle* t = &tris[e->prim];
        const float w = 1.0f - e->u - e->v;
        nn = v_normalize(v_add(v_add(v_scale(v_load(t->normalA), w), v_scale(v_load(t->normalB), e->u)), v_scale(v_load(t->normalC), e->v)));
        o->chunk = e->chunk;
        o->mesh = chunk_mesh ? chunk_mesh[e->chunk] : -1;
        o->u = e->u; o->v = e->v;
    }
    o->dst = e->dst;
    o->hitPoint[0] = hp.x; o->hitPoint[1] = hp.y; o->hitPoint[2] = hp.z;
    o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
    o->kind = e->kind;
    o->primitive = e->prim;
    o->side = e->side;
}

static int mh_scene_ok(const rt_meshinfo* mi, int nm, int nt, size_t* addressed)
{
    size_t a = 0;
    for (int m = 0; m < nm; m++) {
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return 0;
        a += mi[m].numTriangles;
    }
    *addressed = a;
    return 1;
}

/* out[i * K + j] = record j of rays[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).
 * -1: bad arguments; -3: a chunk's range leaves the triangle buffer; -4: out of memory. */
int mh_trace(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
             int intersect, const rt_ray* rays, int n, int K, int mode, int count_all, rt_multihit* out)
{
    if (n < 0 || K < 1 || K > RT_HITS_MAX || (mode != RT_HITS_FRONT && mode != RT_HITS_BOTH) || (count_all != 0 && count_all != 1)) return -1;
    size_t addressed;
    if (!mh_scene_ok(mi, nm, nt, &addressed)) return -3;
    const size_t cap = 2 * (size_t)ns + addressed + 1;
    int failed = 0;
#pragma omp parallel
    {
        mh_cand* list = malloc(cap * sizeof *list);
        if (!list) {
#pragma omp atomic write
            failed = 1;
        }
#pragma omp for schedule(dynamic, 16)
        for (int i = 0; i < n; i++) {
            if (!list) continue;
            const int total = mh_collect(spheres, ns, tris, mi, nm, intersect, mode == RT_HITS_BOTH, &rays[i], list);
            qsort(list, (size_t)total, sizeof *list, mh_before);
            const int kept = total < K ? total : K;
            const int hit_count = count_all ? total : kept;
            for (int j = 0; j < K; j++) {
                rt_multihit* o = &out[(size_t)i * K + j];
                if (j < kept) mh_fill(o, &list[j], spheres, tris, chunk_mesh, &rays[i], hit_count);
                else mh_empty(o, hit_count);
            }
        }
        free(list);
    }
    return failed ? -4 : 0;
}

/* The untruncated list of ONE ray: returns the number of accepted hits below tMax and fills the first min(total, cap) of them, sorted,
 * with hitCount = total.  Negative: as mh_trace. */
int mh_all(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
           int intersect, const rt_ray* ray, int mode, rt_multihit* out, int cap_out)
{
    if (!ray || cap_out < 0 || (mode != RT_HITS_FRONT && mode != RT_HITS_BOTH)) return -1;
    size_t addressed;
    if (!mh_scene_ok(mi, nm, nt, &addressed)) return -3;
    mh_cand* list = malloc((2 * (size_t)ns + addressed + 1) * sizeof *list);
    if (!list) return -4;
    const int total = mh_collect(spheres, ns, tris, mi, nm, intersect, mode == RT_HITS_BOTH, ray, list);
    qsort(list, (size_t)total, sizeof *list, mh_before);
    for (int j = 0; j < total && j < cap_out; j++) mh_fill(&out[j], &list[j], spheres, tris, chunk_mesh, ray, total);
    free(list);
    return total;
}
