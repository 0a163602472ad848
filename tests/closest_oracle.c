/*
 * closest_oracle.c — closest-point queries (include/rt.h "closest-point queries": rt_closest_points) restated in plain C as a brute-force
 * loop over every sphere and every triangle a chunk addresses: the checker of tests/test_gpu_closest.py, itself pinned by
 * tests/test_closest_cpu.py (a float64 twin, hand-computed cases).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own
 * CFLAGS (oracle/Makefile, tests/checker_build.py: -ffp-contract=off, so every product and sum below rounds on its own, as the header
 * demands).  It includes nothing but the public header: the definition is the library's own, not the shader's.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../include/rt.h"

typedef struct { float x, y, z; } v3;
static v3 V(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static v3 ld(const float* p) { return V(p[0], p[1], p[2]); }
static v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 scale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static v3 cross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static v3 normalize(v3 a) { const float len = sqrtf(dot(a, a)); return V(a.x / len, a.y / len, a.z / len); }

/* sphere: key and, for the winner, the record's geometric fields */
static float sphere_key(v3 p, const rt_sphere* s)
{
    const v3 m = sub(p, ld(s->position));
    const float len = sqrtf(dot(m, m));
    const float ds = fabsf(len - s->radius);
    return ds * ds;
}

/* triangle: the seven regions in the header's order, first match decides; returns the key, (u, v) through the pointers */
static float triangle_key(v3 p, const rt_triangle* t, float* pu, float* pv)
{
    const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
    const v3 ap = sub(p, A);
    const float d1 = dot(eAB, ap), d2 = dot(eAC, ap);
    const v3 bp = sub(ap, eAB);
    const float d3 = dot(eAB, bp), d4 = dot(eAC, bp);
    const v3 cp = sub(ap, eAC);
    const float d5 = dot(eAB, cp), d6 = dot(eAC, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    float u, v;
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; }
    else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); }
    else if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) { v = d43 / (d43 + d56); u = 1.0f - v; }
    else {
        const float den = (va + vb) + vc;
        u = vb / den; v = vc / den;
        u = u < 0.0f ? 0.0f : u;
        u = u > 1.0f ? 1.0f : u;
        v = v < 0.0f ? 0.0f : v;
        const float room = 1.0f - u;
        v = v > room ? room : v;
    }
    const v3 q = add(add(A, scale(eAB, u)), scale(eAC, v));
    const v3 e = sub(p, q);
    *pu = u; *pv = v;
    return dot(e, e);
}

static void miss(rt_closest* o)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
}

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
        miss(o);
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
                float u, v;
                const float k = triangle_key(p, &tris[t], &u, &v);
                tests++;
                if (!(k < bound)) continue;
                equal = !have || k < best ? 1 : equal + (k == best);
                if (!have || k < best || (k == best && kind == RT_HIT_TRIANGLE && t < prim)) {
                    have = 1; kind = RT_HIT_TRIANGLE; prim = t; best = k; bu = u; bv = v; chunk = m;
                }
            }
        if (!have) continue;
        if (at_best) at_best[i] = equal;
        o->kind = kind;
        o->primitive = (int32_t)prim;
        if (kind == RT_HIT_SPHERE) {
            const rt_sphere* s = &spheres[prim];
            const v3 c = ld(s->position), m = sub(p, c);
            const float len = sqrtf(dot(m, m));
            const v3 q = add(c, scale(m, s->radius / len));
            const v3 nn = normalize(sub(q, c));
            o->dst = fabsf(len - s->radius);
            o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
            o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
            o->side = len >= s->radius ? 1 : -1;
        } else {
            const rt_triangle* t = &tris[prim];
            const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
            const v3 q = add(add(A, scale(eAB, bu)), scale(eAC, bv));
            const v3 e = sub(p, q);
            const float sd = dot(e, cross(eAB, eAC));
            const float w = 1.0f - bu - bv;
            const v3 nn = normalize(add(add(scale(ld(t->normalA), w), scale(ld(t->normalB), bu)), scale(ld(t->normalC), bv)));
            o->dst = sqrtf(best);
            o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
            o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
            o->chunk = chunk;
            o->mesh = chunk_mesh ? chunk_mesh[chunk] : -1;
            o->u = bu; o->v = bv;
            o->side = sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0;
        }
    }
    if (prim_tests) *prim_tests = tests;
    return 0;
}
