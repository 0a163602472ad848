/*
 * nearest_oracle.c — K-nearest point queries (include/rt.h "K-nearest queries": rt_closest_points with the options "closest_k" and
 * "closest_all") restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, a FULL sort of the
 * candidates below R * R by (k, kind, primitive), the count rule, and "the defaults leave _reserved 0".  The checker of
 * tests/test_gpu_nearest.py and tests/test_gpu_nearest_fuzz.py, itself pinned by tests/test_nearest_cpu.py (against closest_oracle.c, a
 * float64 twin, hand-computed cases, and the one-line mutants below, each of which some case must tell from the definition).  TEST
 * INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS (tests/checker_build.py: -ffp-contract=off, so every product and
 * sum rounds on its own, as the header demands).  It includes nothing but the public header.
 *
 * variant: 0 the definition;
 *          1 a non-strict radius, k <= R * R;
 *          2 a tie between triangles broken by the position in the enumeration (chunk by chunk, as listed) instead of the uploaded index;
 *          3 at equal k a triangle before a sphere;
 *          4 the count capped at K under closest_all = 1;
 *          5 a streaming list that drops a candidate whose key EQUALS the K-th key once K are in.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
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

static float sphere_key(v3 p, const rt_sphere* s)
{
    const v3 m = sub(p, ld(s->position));
    const float len = sqrtf(dot(m, m));
    const float ds = fabsf(len - s->radius);
    return ds * ds;
}

/* the seven regions in the header's order, first match decides; returns the key, (u, v) through the pointers */
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

static void miss(rt_closest* o, int count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->_reserved[0] = count;
}

typedef struct { float k, u, v; int kind; uint32_t prim; int chunk; uint32_t seq; int variant; } cand;

/* ascending (k, kind, primitive): a sphere (RT_HIT_SPHERE = 1) before a triangle (RT_HIT_TRIANGLE = 2), then the lower uploaded index */
static int before(const cand* a, const cand* b)
{
    if (a->k != b->k) return a->k < b->k;
    if (a->kind != b->kind) return a->variant == 3 ? a->kind > b->kind : a->kind < b->kind;
    if (a->variant == 2 && a->kind == RT_HIT_TRIANGLE) return a->seq < b->seq;
    return a->prim < b->prim;
}
static int by_key(const void* a, const void* b)
{
    return before((const cand*)a, (const cand*)b) ? -1 : before((const cand*)b, (const cand*)a) ? 1 : 0;
}

static void record(rt_closest* o, v3 p, const cand* c, const rt_sphere* spheres, const rt_triangle* tris, const int32_t* chunk_mesh, int count)
{
    miss(o, count);
    o->kind = c->kind;
    o->primitive = (int32_t)c->prim;
    if (c->kind == RT_HIT_SPHERE) {
        const rt_sphere* s = &spheres[c->prim];
        const v3 ce = ld(s->position), m = sub(p, ce);
        const float len = sqrtf(dot(m, m));
        const v3 q = add(ce, scale(m, s->radius / len));
        const v3 nn = normalize(sub(q, ce));
        o->dst = fabsf(len - s->radius);
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->side = len >= s->radius ? 1 : -1;
    } else {
        const rt_triangle* t = &tris[c->prim];
        const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
        const v3 q = add(add(A, scale(eAB, c->u)), scale(eAC, c->v));
        const v3 e = sub(p, q);
        const float sd = dot(e, cross(eAB, eAC));
        const float w = 1.0f - c->u - c->v;
        const v3 nn = normalize(add(add(scale(ld(t->normalA), w), scale(ld(t->normalB), c->u)), scale(ld(t->normalC), c->v)));
        o->dst = sqrtf(c->k);
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->chunk = c->chunk;
        o->mesh = chunk_mesh ? chunk_mesh[c->chunk] : -1;
        o->u = c->u; o->v = c->v;
        o->side = sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0;
    }
}

/* out[i * K + j] = record j of points[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).
 * totals (may be NULL): per point, the number of ALL candidates below R * R, whatever K and all are.  kth_ties (may be NULL): per point,
 * 1 when the K-th and the (K+1)-th key of the full sort are bit-equal.  -3: a chunk's range leaves the triangle buffer; -4: K or all out
 * of range; -5: out of memory. */
int np_nearest(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* points, int n, int K, int all, int variant, rt_closest* out, int32_t* totals, int32_t* kth_ties)
{
    if (K < 1 || K > RT_HITS_MAX || (all != 0 && all != 1)) return -4;
    size_t addressed = 0;
    for (int m = 0; m < nm; m++) {
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
        addressed += mi[m].numTriangles;
    }
    const int defaults = K == 1 && all == 0;                        /* today's call: _reserved stays 0 */
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[(size_t)i * K];
        for (int j = 0; j < K; j++) miss(&o[j], 0);
        if (totals) totals[i] = 0;
        if (kth_ties) kth_ties[i] = 0;
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
            cand e = { k, 0.0f, 0.0f, RT_HIT_SPHERE, (uint32_t)s, -1, seq++, variant };
            c[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                float u, v;
                const float k = triangle_key(p, &tris[t], &u, &v);
                if (!(variant == 1 ? k <= bound : k < bound)) continue;
                cand e = { k, u, v, RT_HIT_TRIANGLE, t, m, seq++, variant };
                c[total++] = e;
            }
        int listed;
        if (variant == 5) {
            /* the candidates in enumeration order through a sorted list of K: full, it takes only a key BELOW its last */
            listed = 0;
            for (int a = 0; a < total; a++) {
                const cand e = c[a];
                if (listed == K && !(e.k < c[K - 1].k)) continue;
                int at = listed < K ? listed : K - 1;
                while (at > 0 && before(&e, &c[at - 1])) { c[at] = c[at - 1]; at--; }   /* (slots 0 .. K-1 of c are free: a >= listed) */
                c[at] = e;
                if (listed < K) listed++;
            }
        } else {
            qsort(c, (size_t)total, sizeof(cand), by_key);
            listed = total < K ? total : K;
            if (kth_ties && total > K && c[K - 1].k == c[K].k) kth_ties[i] = 1;
        }
        if (totals) totals[i] = total;
        const int capped = total < K ? total : K;
        const int count = defaults ? 0 : (all && variant != 4) ? total : capped;
        for (int j = 0; j < K; j++) {
            if (j < listed) record(&o[j], p, &c[j], spheres, tris, chunk_mesh, count);
            else miss(&o[j], count);
        }
        free(c);
    }
    return failed ? -5 : 0;
}
